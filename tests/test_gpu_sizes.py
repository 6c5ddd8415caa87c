"""`--sizes` for plain ranks on the words route (csrc/wk_sized.hpp): the
histogram over (subject, read size) and the rows it emits against numpy, and
`woltka classify --sizes` against what the reference wrote
(tests/golden/vectors/sizes_device.json, made by
tests/golden/make_sizes_reference.py from the inputs of tests/sizes_cases.py;
cli_random.json; the bundled CPM table)."""
import contextlib
import ctypes as C
import io
import lzma
import os
from os.path import join

import numpy as np
import pytest

import sizes_cases as SC
from helpers import DATA, load_vectors

pytestmark = pytest.mark.gpu

# mirrors of csrc/wk_weigh.hpp
K_BINS_MAX_LDS = 160 * 1024 - 1024      # constexpr uint32_t kBinsMaxLds = 160 * 1024 - 1024;
K_SLICE_BINS = K_BINS_MAX_LDS // 4 - 96  # constexpr uint32_t kSliceBins = kBinsMaxLds / 4 - 96;
K_MAX_STREAMS = 8                       # constexpr int kMaxStreams = 8;
# ... and of csrc/wk_sized.hpp
K_SIZED_SUB = K_SLICE_BINS // 16        # constexpr uint32_t kSizedSub = kSliceBins / kSizedSizes;
assert K_SLICE_BINS == 40608 and K_SIZED_SUB * 16 == K_SLICE_BINS

GOLD = load_vectors('sizes_device.json')
CASES = {c['name']: c for c in SC.cases()}


# ---- the kernels, words in and rows out ------------------------------------
_HIER = {}


def _hier():
    if not _HIER:
        from woltka_amd import synth
        rng = np.random.default_rng(77)
        p = synth.lca_problem(rng, n_nodes=3000, n_subjects=50, n_reads=10,
                              with_names=False)
        _HIER['h'] = p['hier']
    return _HIER['h']


def _words(rng, n, subjects, hot=None):
    """``n`` packed records over the given subject indices, read sizes
    uniform in 1..16; ``hot`` = (subject, size, times) is one bin hit that
    often."""
    s = rng.choice(subjects, n).astype(np.uint32)
    k = rng.integers(1, 17, n).astype(np.uint32)
    if hot is not None:
        s[:hot[2]], k[:hot[2]] = hot[0], hot[1]
        mix = rng.permutation(n)
        s, k = s[mix], k[mix]
    pos = (rng.integers(0, 16, n).astype(np.uint32) % k)
    return s | (pos << np.uint32(23)) | (k << np.uint32(27))


def _expected(words, group, feats, job_feats):
    """{(feature_j(s), feature(s), j << 16 | k, group): count}"""
    s = (words & np.uint32((1 << 23) - 1)).astype(np.int64)
    k = (words >> np.uint32(27)).astype(np.int64)
    cell, cnt = np.unique(s * 32 + k, return_counts=True)
    out = {}
    for j, of in enumerate(job_feats):
        for c, n in zip(cell.tolist(), cnt.tolist()):
            key = (int(of[c >> 5]), int(feats[c >> 5]), (j << 16) | (c & 31),
                   group)
            out[key] = out.get(key, 0) + n
    return out


def _summed(rows, counts):
    out = {}
    for r, n in zip(map(tuple, rows.tolist()), counts.tolist()):
        out[r] = out.get(r, 0) + n
    return out


@pytest.mark.parametrize('three_jobs', [False, True], ids=['none', 'ranks'])
@pytest.mark.parametrize('n_subjects', [
    1, 17, K_SLICE_BINS - 1, K_SLICE_BINS, K_SLICE_BINS + 1,
    K_MAX_STREAMS * K_SLICE_BINS + 1])      # (the last: more slices than streams, the unsliced layout)
def test_rows_of_random_words(n_subjects, three_jobs):
    """~200 k records in three appends: the subject table grows between the
    first two, the third belongs to another group (its `words_begin` flushes
    the first), one fetch at the end.  One bin is hit 70 000 times; most bins
    never."""
    from woltka_amd import _native as nat
    h = _hier()
    rng = np.random.default_rng(n_subjects + 5 * three_jobs)
    with nat.Context(0) as c:
        c.set_tree(h.parent, h.last, h.rank_code)
        c.build_rank_table(0, h.rank_codes['genus'])
        c.build_rank_table(1, h.rank_codes['phylum'])
        anc = [c.get_rank_table(0), c.get_rank_table(1)]
        if three_jobs:      # subjects: nodes with a genus and a phylum, repeated
            nodes = np.flatnonzero((anc[0] >= 0) & (anc[1] >= 0))
            assert nodes.size > 100
            feats = rng.choice(nodes, n_subjects).astype(np.int32)
            jobs = [nat.Job(nat.MODE_RANK, 0, nat.F_SIZED, 0, 0.0),
                    nat.Job(nat.MODE_NONE, 0, nat.F_SIZED, 0, 0.0),
                    nat.Job(nat.MODE_RANK, 1, nat.F_SIZED, 0, 0.0)]
            job_feats = [anc[0][feats], feats, anc[1][feats]]
        else:
            feats = (np.arange(n_subjects, dtype=np.int64) * 7 + 3).astype(np.int32)
            jobs = [nat.Job(nat.MODE_NONE, 0, nat.F_SIZED, 0, 0.0)]
            job_feats = [feats]
        c.counts_reserve(1 << 12)
        n1 = max(1, n_subjects // 2)
        # the subjects the records name: at most 3000, spread over the table
        # (its first and last subject among them)
        act1 = np.unique(np.r_[0, n1 - 1, rng.integers(0, n1, 1500)])
        act2 = np.unique(np.r_[0, n_subjects - 1, n1 - 1, min(n1, n_subjects - 1),
                               rng.integers(0, n_subjects, 3000)])
        hot = (int(act2[act2.size // 2]), 7, 70_000)
        w1 = _words(rng, 40_000, act1)
        w2 = _words(rng, 110_000, act2, hot)
        w3 = _words(rng, 50_000, act2)
        c.set_subjects(feats[:n1])
        assert c.words_begin(jobs, 3)
        c.words_append(w1, 11_000)
        c.set_subjects(feats)
        assert c.words_begin(jobs, 3)
        c.words_append(w2, 30_000)
        assert c.sized_pending()[0] == 0 or n_subjects > K_MAX_STREAMS * K_SLICE_BINS   # (outgrown streams are flushed)
        assert c.words_begin(jobs, 5)
        assert c.words_pending() == (0, 0) and c.sized_pending()[0] > 0
        c.words_append(w3, 9_000)
        held = c.sized_pending()[0]
        # a buffer that is too small: the number needed, nothing written or dropped
        n = C.c_int64(0)
        small = np.full((max(held - 1, 1), 4), -7, np.int32)
        small_n = np.full(small.shape[0], -7, np.int64)
        rc = c._lib.wk_sized_fetch(
            c._h, small.ctypes.data_as(C.POINTER(C.c_int32)),
            small_n.ctypes.data_as(C.POINTER(C.c_int64)), held - 1, C.byref(n))
        assert rc == nat.E_CAPACITY and n.value > held
        assert (small == -7).all() and (small_n == -7).all()
        rows, counts = c.sized_fetch()
        assert rows.shape[0] == n.value and c.sized_pending()[0] == 0
        assert c.sized_pending()[1] >= 2
        want = _expected(np.r_[w1, w2], 3, feats, job_feats)
        want.update(_expected(w3, 5, feats, job_feats))
        assert (counts > 0).all()
        got = _summed(rows, counts)
        assert got == want
        assert max(got.values()) >= 70_000
        assert int(counts.sum()) == 200_000 * len(jobs)
        st = c.stats()
        assert st['n_reads'] == 50_000 and st['n_records'] == 200_000
        assert c.counts_fetch()[0].size == 0        # (sized jobs count nothing)
        assert c.sized_fetch()[0].shape == (0, 4)
        # job sets the flush does not take: sized next to unsized, sized jobs
        # that look at whole reads
        plain = nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)
        assert not c.words_begin([jobs[0], plain], 0)
        for mode, flags, major in ((nat.MODE_FREE, 0, 0.0), (nat.MODE_RANK, nat.F_UNIQ, 0.0),
                                   (nat.MODE_RANK, nat.F_ABOVE, 0.0), (nat.MODE_RANK, 0, 0.8),
                                   (nat.MODE_NONE, nat.F_UNIQ, 0.0)):
            assert not c.words_begin([nat.Job(mode, 0, flags | nat.F_SIZED, 0, major)], 0)


# ---- woltka classify --sizes -------------------------------------------------
def _classify(case, tmp_path, monkeypatch, block=None, no_dsizes=False,
              without_sizes=False, digits=None):
    """Run the case; returns (result as `sizes_cases.run_case` gives it, the
    routes taken)."""
    from woltka_amd import classify as Cl
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    if block is not None:
        monkeypatch.setattr(Cl.Engine, 'DTOK_BLOCK', block)
    if no_dsizes:
        monkeypatch.setenv('WOLTKA_NO_DSIZES', '1')
    else:
        monkeypatch.delenv('WOLTKA_NO_DSIZES', raising=False)
    case = dict(case, kwargs=dict(case['kwargs']))
    if without_sizes:
        del case['kwargs']['sizes']
    if digits is not None:
        case['kwargs']['digits'] = digits
    ROUTES.clear()
    os.makedirs(tmp_path, exist_ok=True)
    res = SC.run_case(workflow, case, str(tmp_path))
    return res, dict(ROUTES)


@pytest.mark.parametrize('block', [1 << 14, None], ids=['16k', 'default'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture_case(tmp_path, monkeypatch, name, block):
    """Byte for byte what the reference wrote, through the sized flush where
    the route's conditions hold."""
    assert set(GOLD) == set(CASES)
    res, routes = _classify(CASES[name], tmp_path / 'a', monkeypatch, block)
    assert res == GOLD[name]
    n = int(name.split('-')[0])
    if n <= 6:
        assert routes.get('sized_flush', 0) > 0, routes
        _, plain = _classify(CASES[name], tmp_path / 'b', monkeypatch, block,
                             without_sizes=True)
        assert routes.get('host_block', 0) == plain.get('host_block', 0), (routes, plain)
        assert plain.get('sized_flush', 0) == 0
    elif n == 7:
        assert routes.get('host_block', 0) >= 1 and routes.get('sized_flush', 0) > 0, routes
    elif n == 8:
        assert routes.get('sized_flush', 0) == 0, routes


@pytest.mark.parametrize('name', ['1-divisors', '2-paired-ranks', '7-wide-read'])
def test_both_routes_write_the_same_bytes(tmp_path, monkeypatch, name):
    """`--digits 10`: the floats of the two routes, not their roundings."""
    a, ra = _classify(CASES[name], tmp_path / 'a', monkeypatch, digits=10)
    b, rb = _classify(CASES[name], tmp_path / 'b', monkeypatch, digits=10,
                      no_dsizes=True)
    assert 'tables' in a and a == b
    assert ra.get('sized_flush', 0) > 0 and rb.get('sized_flush', 0) == 0


def _random_cases():
    """Cases of cli_random.json within the route's limits: `--sizes`, a
    directory of plain or gzip files, plain ranks, nothing per read."""
    out = []
    for i, c in enumerate(load_vectors('cli_random.json')):
        kw = c['kwargs']
        ranks = (kw.get('ranks') or 'none').split(',')
        if kw.get('sizes') and kw['input_fp'] == 'aln' and \
                'tables' in c['expect'] and \
                not c['want_maps'] and not c.get('want_cov') and \
                not any(kw.get(k) for k in ('demux', 'samples', 'strata_dir', 'coords_fp', 'uniq',
                                            'major', 'above', 'map_rank')) and \
                'free' not in ranks and \
                all(os.path.splitext(f)[1] not in ('.bz2', '.xz')
                    for f in c['files'] if f.startswith('aln/')):
            out.append(i)
    return out


def test_there_is_a_random_case_within_the_limits():
    assert _random_cases()


@pytest.mark.parametrize('i', _random_cases())
def test_reference_written_random_case(tmp_path, i):
    from test_gpu_cli_random import write_case_file
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    case = load_vectors('cli_random.json')[i]
    for rel, text in case['files'].items():
        write_case_file(tmp_path / rel, text)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return join(DATA, 'taxonomy', v[5:])
        if isinstance(v, str) and (v in case['files'] or v == 'aln'):
            return str(tmp_path / v)
        return v
    args = {k: real(v) for k, v in case['kwargs'].items()}
    args['output_fp'] = str(tmp_path / 'out')
    ROUTES.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**args)
    expect = case['expect']['tables']
    if len(expect) == 1 and 'out' in expect:
        got = {'out': (tmp_path / 'out').read_text()}
    else:
        got = {fn: (tmp_path / 'out' / fn).read_text()
               for fn in sorted(os.listdir(tmp_path / 'out'))}
    assert got == expect
    assert ROUTES['sized_flush'] > 0, dict(ROUTES)


def test_bt2sho_cpm_from_plain_sam(tmp_path, monkeypatch):
    """The reference's own CPM recipe (golden bt2sho.order.cpm.tsv) on the
    bundled SAM files, decompressed: the device tokenises them and the sized
    flush makes their rows.  (The 62 subjects all have every rank and a size;
    the largest read has 13 subjects.)"""
    import filecmp
    from click.testing import CliRunner
    from woltka_amd.cli import classify_cmd
    from woltka_amd.hostio import ROUTES
    monkeypatch.delenv('WOLTKA_NO_DSIZES', raising=False)
    src = join(DATA, 'align', 'bt2sho')
    indir = tmp_path / 'bt2sho'
    indir.mkdir()
    for fn in sorted(os.listdir(src)):
        assert fn.endswith('.sam.xz')
        with lzma.open(join(src, fn)) as f:
            (indir / fn[:-3]).write_bytes(f.read())
    tax = join(DATA, 'taxonomy')
    out = str(tmp_path / 'output.tsv')
    ROUTES.clear()
    res = CliRunner().invoke(classify_cmd, [
        '--input', str(indir), '--names', join(tax, 'names.dmp'),
        '--nodes', join(tax, 'nodes.dmp'), '--map', join(tax, 'taxid.map'),
        '--rank', 'order', '--sizes', join(tax, 'length.map'),
        '--scale', '1M', '--digits', '3', '--output', out, '--no-exe'])
    assert res.exit_code == 0, res.output + repr(res.exception)
    assert filecmp.cmp(out, join(DATA, 'output', 'bt2sho.order.cpm.tsv'),
                       shallow=False)
    print(dict(ROUTES))
    assert ROUTES['sized_flush'] > 0 and ROUTES['dtok_fused'] > 0, dict(ROUTES)
