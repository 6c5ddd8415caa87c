"""The device text route on the limit-shape texts of tests/golden/dtok_limits.py
against the REFERENCE's tables (tests/golden/vectors/dtok_limits.json,
make_golden.py::gen_dtok_limits), and the route every case exists to produce.

Geometry.  Blocks of 8 and 32 KB at the default launch (3 workgroups a CU:
4 KB tiles, 8 KB windows); blocks of 4 MB with one workgroup a CU (one round
of 16 KB tiles on 256 CUs) and of 8 MB (two rounds); 64 KB blocks for the
texts of many subjects.  `dtok_fused_per_cu` is set on every context the
workflow opens (it opens it on a thread of its own) -- no product knob.

Readers.  pread with the column trim (the default), pread without it, and the
file pinned in place (as tests/test_gpu_dtok.py::
test_mapped_route_with_runs_longer_than_a_block): the two untrimmed ones are
where lines longer than the kernel's window reach it.  Verdicts are read a
block late (the default) and, for the cases built around hand-backs, at once
(WOLTKA_NO_LAG=1).

Routes (ROUTES after the run; `fused` = dtok_fused, `back` =
dtok_fused_back, per file where it matters):
- every case: the kernel kept blocks (fused > 0) -- the limit shapes come in
  stretches between text it keeps (dtok_limits._mixed), so that the tables
  pin the kernel's own work next to each limit, not only the six kernels';
  where the shape exceeds a limit at that geometry it also handed blocks
  back (back > 0); the plain controls and qname_again: back == 0; no case
  plants lines for the host: host_block == 0.  The refusals: the device route
  took the blocks in front of the bad line (dtok > 0) before it raised.
- 5-8 slices of subjects (more than kFzStreams = 4 record streams, fewer than
  kMaxStreams = 8): once the subject table is that large no block goes
  through the one kernel (dtok_scan_impl: `fa.streams.n_streams <=
  kFzStreams`) -- the second sample, which knows all of them from its first
  block, has fused == back == 0 (the kernel is not even tried) and is done by
  the six kernels (dtok > 0).  With 2-4 slices it has fused > 0.
- more than 8 slices: `wk_words_begin` opens the job set unsliced
  (`w_sliced` needs streams_needed <= kMaxStreams), one record stream, and
  the first sample is reopened that way when it outgrows 8 slices
  (`words_roll`, `outgrown`).  One stream is within kFzStreams: the second
  sample's blocks go through the one kernel again (fused > 0 there).
- the first sample of every slices case names a new subject in every block:
  the kernel hands each block it tries back (its dictionary lacks the name),
  which is why these cases pin their routes on the second sample only.

The file pinned in place is checked to have been pinned (a spy on
`host_register`): that reader falls back to pread when pinning fails."""
import contextlib
import io
import os
import sys
from os.path import join

import pytest

from helpers import load_vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, join(ROOT, 'tests', 'golden'))
import dtok_limits as D  # noqa: E402

VEC = load_vectors('dtok_limits.json')
TAX = join(ROOT, 'tests', 'golden', 'data', 'taxonomy')

UNTRIMMED = ('notrim', 'mapped')
EXTRA_READERS = {'long_lines': UNTRIMMED, 'long_lines_t16': UNTRIMMED,
                 'long_runs': ('notrim',), 'names': ('mapped',),
                 'plain': ('notrim',)}
NO_LAG = ('late_subjects', 'long_runs', 'long_lines', 'long_runs_t16',
          'long_lines_t16')


def _params():
    out = []
    for name in sorted(D.CASES):
        for geo in D.CASES[name][4]:
            for reader in ('trim',) + EXTRA_READERS.get(name, ()):
                out.append((name, geo, reader, 'late'))
                if name in NO_LAG:
                    out.append((name, geo, reader, 'nolag'))
    return out


def _expect_routes(name, geo, reader, r, per_file):
    """The routes of one run (see the module's docstring)."""
    fused, back = r.get('dtok_fused', 0), r.get('dtok_fused_back', 0)
    shape = D.CASES[name][0]
    assert r.get('host_block', 0) == 0, r
    if shape == 'slices':           # (the second sample: all subjects known)
        s2 = [a - b for a, b in zip(per_file[-1], per_file[-2])]
        if name == 'slices_8':
            assert s2 == [0, 0] and r.get('dtok', 0) > 0, (r, per_file)
        else:
            assert s2[0] > 0, (r, per_file)
        return
    assert fused > 0, r
    if shape in ('plain', 'qname_again'):
        assert back == 0, r
    elif shape == 'long_lines' and reader in UNTRIMMED:
        assert back > 0, r          # (lines past the window: the trail check)
    elif shape == 'long_runs':      # (runs past kFzFwd, a tile and a block)
        assert back > 0, r
    elif shape == 'dense' and geo != 'b8k':
        # (more than kFzLines lines a window; at 8 KB blocks the windows are
        # cut short by the block's ends)
        assert back > 0, r
    elif shape == 'late_subjects':  # (handed back, then taken again)
        assert back > 0, r


@pytest.mark.parametrize('name,geo,reader,lag', _params(),
                         ids=lambda v: str(v))
def test_limit_shapes_give_the_reference_tables(tmp_path, monkeypatch, name,
                                                geo, reader, lag):
    from woltka_amd import _native as nat
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.routes import device_text
    from woltka_amd.workflow import workflow
    case = VEC[name]
    block, per_cu = D.GEOMETRY[geo]
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', block)
    if per_cu is not None:
        init = nat.Context.__init__

        def init_tuned(self, *a, **k):
            init(self, *a, **k)
            self.tune('dtok_fused_per_cu', per_cu)
        monkeypatch.setattr(nat.Context, '__init__', init_tuned)
    if reader == 'notrim':
        monkeypatch.setattr(device_text, 'TRIM', False)
    elif reader == 'mapped':
        monkeypatch.setattr(C.Engine, 'HOSTREG_MIN', 0)
        monkeypatch.setattr(C.Engine, 'HOSTREG_PIECE', 1 << 21)
        monkeypatch.setattr(C.Engine, 'HOSTREG_RATE', 0.0)
        monkeypatch.setenv('WOLTKA_HOSTREG', '1')
        pinned = []
        register = nat.Context.host_register

        def spy_register(self, address, n):
            pinned.append(n)
            return register(self, address, n)
        monkeypatch.setattr(nat.Context, 'host_register', spy_register)
    if lag == 'nolag':
        monkeypatch.setenv('WOLTKA_NO_LAG', '1')
    per_file = [(0, 0)]
    counts = nat.Context.dtok_fused_counts

    def spy(self):
        res = counts(self)
        per_file.append(tuple(res))
        return res
    monkeypatch.setattr(nat.Context, 'dtok_fused_counts', spy)

    files, kw = D.case_files(name)
    for rel, text in files.items():
        os.makedirs(os.path.dirname(tmp_path / rel), exist_ok=True)
        (tmp_path / rel).write_bytes(text.encode())

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return join(TAX, v[5:])
        if v == 'aln':
            return str(tmp_path / v)
        return v
    args = {k: real(v) for k, v in case['kwargs'].items()}
    args['output_fp'] = str(tmp_path / 'out')
    ROUTES.clear()
    if 'error' in case:
        with pytest.raises(Exception) as e:
            with contextlib.redirect_stdout(io.StringIO()):
                workflow(**args)
        assert type(e.value).__name__ == case['error']
        # (the blocks in front of the bad line went through the device)
        assert ROUTES.get('dtok', 0) > 0, dict(ROUTES)
        return
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**args)
    out = tmp_path / 'out'
    paths = ({fn: out / fn for fn in sorted(os.listdir(out))}
             if out.is_dir() else {'out': out})
    got = {fn: D.table_record(p.read_bytes()) for fn, p in paths.items()}
    assert got == case['tables']
    print('routes', name, geo, reader, lag, dict(ROUTES), per_file)
    if reader == 'mapped':
        assert pinned, 'the file was not pinned in place'
    _expect_routes(name, geo, reader, dict(ROUTES), per_file)
