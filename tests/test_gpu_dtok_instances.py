"""The two instances of the one-kernel SAM tokenizer (csrc/wk_dtok_fused.hpp)
and the predicates that were rewritten when its wave-uniform values went back
into scalar registers.

`dtok_fused_kernel` is the product's instance of the kernel's body: it does
not read `FusedArgs::ablate`.  `dtok_fused_measure_kernel` is the same body
with the measurement switches of `wk_tune("fz_ablate")`, launched exactly when
that word is not 0.  The body tests bits 1 to 512 of the word; bit 1024 is
none of them, so a pass with `fz_ablate = 1024` runs the measuring instance
with no phase left out and must give what the product's instance gives.

(The issue named `fz_ablate = 16` for that pass, as "only the short-line flag
left out".  In the kernel as it is -- and as the issue wants it kept, since
`tools/fused_ablate.py` has to measure what it measured before -- switch 16
also leaves out the whole FLAG / RNAME parse of the line pass: no line is
mapped, no record leaves, and the tables cannot be the product's.  Both
passes are run here: 1024 carries the comparison of tables, log, lines, reads
and cells; 16 is held to what holds for it -- the measuring instance is
launched, keeps every block and hands none back, and the product's instance
gives its own results again afterwards.)

The predicates: "a lane of the first wave" (the stores that clear `own[]` and
pad `info[]`, the reserving lanes of `flush_all`) is a scalar test of the
wave's index and a compare of the lane; the newlines in front of a wave's
chunks are summed with scalar compares; `submap`, `open_end` and the window
limits (32-bit forms, tests/test_dtok_limits32_host.py) are tested where they
are used.  Every case compares the one kernel with the six kernels
(WOLTKA_NO_FUSED=1) on the same files: same tables, same log."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dtok_limits as D  # noqa: E402
import test_gpu_dtok as T  # noqa: E402  (its `_run`, `_fused_sam`, `_random_sam`)
import test_gpu_dtok_exit as E  # noqa: E402  (`_per_cu`, `_spy_counts`, `_totals_context`)

TAX = os.path.join(ROOT, 'tests', 'golden', 'data', 'taxonomy')


def _tuned(monkeypatch, knobs):
    """Every context created from here on is tuned with `knobs` as they are
    at that moment (a dict the test changes between passes)."""
    from woltka_amd import _native as nat
    init = nat.Context.__init__

    def init_tuned(self, *a, **k):
        init(self, *a, **k)
        for name, value in knobs.items():
            self.tune(name, value)
    monkeypatch.setattr(nat.Context, '__init__', init_tuned)


def _two_routes(tmp_path, monkeypatch, **kw):
    """The one kernel against the six: equal tables and logs; returns the
    tables and the one-kernel run's ROUTES."""
    from woltka_amd.hostio import ROUTES
    ROUTES.clear()
    a, log_a = T._run(tmp_path, 'fused', False, **kw)
    routes_a = dict(ROUTES)
    monkeypatch.setenv('WOLTKA_NO_FUSED', '1')
    ROUTES.clear()
    b, log_b = T._run(tmp_path, 'six', False, **kw)
    assert ROUTES['dtok_fused'] == 0 and ROUTES['dtok'] > 0, dict(ROUTES)
    monkeypatch.delenv('WOLTKA_NO_FUSED')
    assert a == b
    assert log_a == log_b
    return a, routes_a


def _plain_file(rng, subjects, size):
    """Well-formed SAM text of at least `size` bytes, cut behind a line."""
    text = T._fused_sam(rng, size // 150, subjects, 'plain')
    assert len(text) >= size
    return text[:text.index('\n', size) + 1]


# ---------------------------------------------------------------------------
# the instance switch

def test_instance_switch_in_one_workflow(tmp_path, monkeypatch):
    """One SAM file of five 256 KB blocks (spans of 4 KB, one window each) in
    five passes: the product's instance, `fz_ablate = 1024` and `= 16` (the
    measuring instance: nothing left out, the line pass's parse left out),
    `fz_ablate = 0` again, WOLTKA_NO_FUSED=1.  Same tables and log in all but
    the pass of switch 16 (the module's docstring); the first four kept the
    same blocks and handed none back."""
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 18)
    knobs = {'fz_ablate': 0}
    _tuned(monkeypatch, knobs)
    per_file = E._spy_counts(monkeypatch)
    rng = random.Random('instances:switch')
    subjects = D.tax_subjects()[:90]
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(_plain_file(rng, subjects, 5 << 18))
    kw = dict(input_fp=str(indir), input_fmt='sam',
              nodes_fps=[os.path.join(TAX, 'nodes.dmp')],
              map_fps=[os.path.join(TAX, 'taxid.map')],
              ranks='none,phylum,genus')
    got, kept = [], []
    for i, ablate in enumerate((0, 1024, 16, 0)):
        knobs['fz_ablate'] = ablate
        ROUTES.clear()
        got.append(T._run(tmp_path, f'pass{i}', False, **kw))
        kept.append(per_file[-1])
        assert ROUTES['dtok_fused'] > 0, (ablate, dict(ROUTES))
    monkeypatch.setenv('WOLTKA_NO_FUSED', '1')
    ROUTES.clear()
    got.append(T._run(tmp_path, 'six', False, **kw))
    assert ROUTES['dtok_fused'] == 0 and ROUTES['dtok'] > 0, dict(ROUTES)
    monkeypatch.delenv('WOLTKA_NO_FUSED')
    print('kept', kept, 'equal to the first pass',
          [g == got[0] for g in got])
    assert got[0] == got[1], 'the measuring instance, nothing left out'
    assert got[0] == got[3], 'the product\'s instance again'
    assert got[0] == got[4], 'the six kernels'
    # (every block behind the file's first one, which is scanned the two-call
    # way; a context per pass, so the counts start at 0 each time)
    assert kept[0] == kept[1] == kept[2] == kept[3] and kept[0][0] >= 4 \
        and kept[0][1] == 0, kept


def test_instance_switch_in_one_context():
    """The same in ONE context, launch by launch: three blocks of 256 KB go
    through `dtok_scan_emit` with fz_ablate 0, 1024, 16, 0 and then through
    the six kernels (`dtok_fused` 0); lines, reads, records and cells are
    equal in all passes but that of switch 16 (the module's docstring), and
    `dtok_fused_counts` moves by one kept block per launch of either
    instance."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        job, tok, names = E._totals_context(ctx, nat)
        rng = random.Random('instances:context')
        blocks = [np.frombuffer(
            _plain_file(rng, names, 1 << 18).split('\n', 2)[2].encode(),
            np.uint8) for _ in range(3)]
        try:
            res = []
            passes = ((1, 0), (1, 1024), (1, 16), (1, 0), (0, 0))
            for fused, ablate in passes:
                ctx.tune('dtok_fused', fused)
                ctx.tune('fz_ablate', ablate)
                assert ctx.words_begin(job, 0)
                before = ctx.dtok_fused_counts()
                sums = []
                for raw in blocks:
                    status, n_lines, reads = ctx.dtok_scan_emit(
                        tok, raw, 0, raw.size)
                    assert status == 0, (fused, ablate)
                    if reads is None:
                        st, reads, _ = ctx.dtok_emit()
                        assert st == 0, (fused, ablate)
                    sums.append((n_lines, reads, ctx.words_pending()[0]))
                ctx.words_flush()
                after = ctx.dtok_fused_counts()
                cells = nat.canonical_counts(*ctx.counts_fetch())
                ctx.counts_clear()
                assert (after[0] - before[0], after[1] - before[1]) == \
                    (3 * fused, 0), (fused, ablate, before, after)
                res.append((sums, cells))
            print('instances', res[0][0])
            for (fused, ablate), (sums, cells) in zip(passes[1:], res[1:]):
                if ablate == 16:
                    continue
                assert sums == res[0][0], (fused, ablate)
                assert np.array_equal(cells[0], res[0][1][0]) and \
                    np.array_equal(cells[1], res[0][1][1])
            for raw, (n_lines, reads, _) in zip(blocks, res[0][0]):
                assert n_lines == int((raw == 10).sum()) and reads > 0
        finally:
            ctx.tune('fz_ablate', 0)
            ctx.tune('dtok_fused', 1)
            tok.close()


# ---------------------------------------------------------------------------
# the predicates that were rewritten

@pytest.mark.parametrize('slices', [1, 2, 3, 4])
def test_slices_and_waves_in_front(tmp_path, monkeypatch, slices):
    """Subject tables of 1 to 4 slices (the reserving lanes of `flush_all`:
    lane < n_streams of the first wave), `dtok_fused_per_cu` = 1 and a block
    of 16 MB read untrimmed: spans of 64 KB, four windows each, so that the
    sum of the counts of the waves in front matters in every wave of every
    window, and about 1 600 records per workgroup against kFzCap = 1 024 --
    the buffers leave once mid-kernel and once at the exit (the geometry of
    tests/test_gpu_dtok_exit.py)."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 24)
    monkeypatch.setattr(device_text, 'TRIM', False)
    E._per_cu(monkeypatch, 1)
    n_subjects = 90 if slices == 1 else slices * D.SLICE - 200
    rng = random.Random(f'instances:{slices}')
    indir = tmp_path / 'in'
    indir.mkdir()
    first = D._slices(rng, n_subjects, None)
    (indir / 'S1.sam').write_text(first)
    # (the reader's blocks: tests/test_gpu_dtok_exit.py.  One 16 MB block
    # through the one kernel: the second of a warm reader, the third of one
    # that ramps up 1, 4, 16 MB)
    warm = len(first) > 1 << 20
    out, size, q = [D.HEADER], 0, 0
    while size < (33 if warm else 22) << 20:
        for _ in range(rng.choice([1, 1, 1, 2, 3])):
            out.append(f'q{q:07d}\t0\tg{rng.randrange(n_subjects):06d}\t'
                       f'{E.TAIL}\n')
            size += 41
        q += 1
    (indir / 'S2.sam').write_text(''.join(out))
    per_file = E._spy_counts(monkeypatch)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    _, routes = _two_routes(tmp_path, monkeypatch, **kw)
    s2 = [x - y for x, y in zip(per_file[2], per_file[1])]
    print('routes', slices, routes, per_file)
    assert s2[0] >= (1 if warm else 2) and s2[1] == 0, (routes, per_file)


@pytest.mark.parametrize('how', ['trimsub', 'exclude'])
def test_subject_map_and_none(tmp_path, monkeypatch, how):
    """`--trim-sub` and `--exclude`: the kernel translates ids through
    `submap` (non-null); the same files without either option: null."""
    from woltka_amd import classify as C
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 16)
    rng = random.Random(f'instances:{how}')
    genomes = D.tax_subjects()[:50]
    subjects = [f'{g}_{k}' for g in genomes for k in (1, 2)] \
        if how == 'trimsub' else genomes
    indir = tmp_path / 'in'
    indir.mkdir()
    for s in ('S1', 'S2'):
        (indir / f'{s}.sam').write_text(T._random_sam(
            rng, 6000 if s == 'S1' else 700, subjects, paired=True,
            unmapped=True, long_names=False))
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    if how == 'trimsub':
        opt = dict(trimsub='_')
    else:
        ex = tmp_path / 'excl.txt'
        ex.write_text('\n'.join(subjects[::9]) + '\n')
        opt = dict(exclude=str(ex))
    with_map, routes = _two_routes(tmp_path, monkeypatch, **kw, **opt)
    assert routes['dtok_fused'] > 0, routes
    (tmp_path / 'plain').mkdir()
    without, routes = _two_routes(tmp_path / 'plain', monkeypatch, **kw)
    assert routes['dtok_fused'] > 0, routes
    assert with_map != without      # (the option did something)


def test_open_end(tmp_path, monkeypatch):
    """Files whose last line has no newline, in blocks of 256 KB: position
    `n` ends a line in the last block's last window."""
    from woltka_amd import classify as C
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 18)
    rng = random.Random('instances:open_end')
    subjects = D.tax_subjects()[:90]
    indir = tmp_path / 'in'
    indir.mkdir()
    for s in ('S1', 'S2'):
        text = T._fused_sam(rng, 9000 if s == 'S1' else 2500, subjects,
                            'open_end')
        assert not text.endswith('\n')
        (indir / f'{s}.sam').write_text(text)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    _, routes = _two_routes(tmp_path, monkeypatch, **kw)
    assert routes['dtok_fused'] > 0, routes
    assert routes['dtok_fused_back'] == 0, routes


def test_last_block_shorter_than_a_span(tmp_path, monkeypatch):
    """A file of three blocks of 256 KB and a rest: the last block the one
    kernel sees is shorter than 4 096 bytes -- one workgroup whose span
    reaches past the text."""
    from woltka_amd import _native as nat
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 18)
    # (untrimmed: the reader's cut is the kernel's block -- 256 KB, and what
    # is left behind the last whole one with the lines carried over to it)
    monkeypatch.setattr(device_text, 'TRIM', False)
    rng = random.Random('instances:short_block')
    subjects = D.tax_subjects()[:90]
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(_plain_file(rng, subjects,
                                              (3 << 18) + 1200))
    sizes = []
    for name in ('dtok_scan_emit', 'dtok_scan_emit_begin'):
        def spy(self, tok, buf, begin, stop, _f=getattr(nat.Context, name)):
            sizes.append(stop - begin)
            return _f(self, tok, buf, begin, stop)
        monkeypatch.setattr(nat.Context, name, spy)
    per_file = E._spy_counts(monkeypatch)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    _, routes = _two_routes(tmp_path, monkeypatch, **kw)
    print('blocks', sizes, routes, per_file)
    assert 0 < min(sizes) < 4096, sizes
    assert routes['dtok_fused'] >= 3 and routes['dtok_fused_back'] == 0, routes
