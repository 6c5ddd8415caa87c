"""Subject coverage (`--outcov`) on the device text route: the coverage pile's
kernels (csrc/wk_cover.hpp) against the reference's range.merge_ranges, and the
command line against the reference workflow's <sample>.cov files and profiles
(tests/golden/vectors/cover_device.json, coverage.json).  Everything compares
exact integers / bytes; wherever the device route is claimed, `ROUTES` says
that it ran and that no block was left to the host tokenizer."""
import contextlib
import io
import json
import lzma
import os
import sys
from os.path import join

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, join(ROOT, 'tests'))
from helpers import DATA, load_vectors      # noqa: E402
import test_cover_host as T                 # noqa: E402

GOLD = load_vectors('cover_device.json')
with open(join(DATA, '..', 'vectors', 'coverage.json')) as _fh:
    COVERAGE = json.load(_fh)
ALN = join(DATA, 'align')


@pytest.fixture
def pile(ctx):
    """The session's context with an empty coverage pile of the default
    size; given up afterwards (`wk_dtok_emit`'s refusals are as before)."""
    ctx.set_option('cover_cap_rows', 0)
    ctx.cover_begin(0)
    yield ctx
    ctx.set_option('cover_cap_rows', 0)
    ctx.cover_begin(-1)


def _merged_through(ctx, key, beg, end, pieces, cap=0):
    """The rows through `wk_cover_add` in `pieces` pieces of uneven size;
    what spills is united with the rest by the numpy mirror (pinned to the
    reference by tests/test_ranges.py and tests/test_cover_host.py)."""
    from woltka_amd.ranges import merge_intervals
    ctx.set_option('cover_cap_rows', cap)
    ctx.cover_begin(0)
    rng = np.random.default_rng(pieces)
    cuts = np.sort(rng.integers(0, key.size + 1, pieces - 1))
    cuts = np.concatenate([[0], cuts, [key.size]])
    spilled, spills = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        spills += ctx.cover_add(key[lo:hi], beg[lo:hi], end[lo:hi],
                                spill=lambda *cols: spilled.append(cols))
    got = ctx.cover_fetch()
    if spilled:
        got = merge_intervals(*(np.concatenate(c).astype(np.int64)
                                for c in zip(*(spilled + [got]))))
    return got, spills


def test_every_golden_merge_case_in_one_pile(pile):
    keys, begs, ends, want = [], [], [], {}
    for i, case in enumerate(COVERAGE['merges']):
        flat = case['ranges']
        keys += [i * 7 + 1] * (len(flat) // 2)
        begs += flat[0::2]
        ends += flat[1::2]
        if case['merged']:
            want[i * 7 + 1] = case['merged']
    perm = np.random.default_rng(1).permutation(len(keys))
    pile.cover_add(np.asarray(keys, np.int32)[perm],
                   np.asarray(begs, np.int32)[perm],
                   np.asarray(ends, np.int32)[perm])
    k, b, e = pile.cover_fetch()
    got = {}
    for kk, bb, ee in zip(k.tolist(), b.tolist(), e.tolist()):
        got.setdefault(kk, []).extend((bb, ee))
    assert got == want
    # the issue's example: touching ranges merge, a row without a span too
    pile.cover_reset()
    flat = [1, 3, 2, 4, 6, 8, 7, 9, 4, 4, 10, 9, 9, 12]
    pile.cover_add([5] * 7, flat[0::2], flat[1::2])
    k, b, e = pile.cover_fetch()
    assert (k.tolist(), b.tolist(), e.tolist()) == ([5, 5], [1, 6], [4, 12])


@pytest.mark.parametrize('order', ['as generated', 'sorted', 'reversed'])
@pytest.mark.parametrize('cap', ['default', 'sixteenth'])
def test_two_million_rows_match_merge_ranges(ctx, order, cap):
    gold = GOLD['merge']
    key, beg, end = T.cover_rows()
    assert key.size == gold['rows']
    if order != 'as generated':
        o = np.lexsort((end, beg, key))
        if order == 'reversed':
            o = o[::-1]
        key, beg, end = key[o], beg[o], end[o]
    try:
        got, spills = _merged_through(
            ctx, key, beg, end, 13,
            0 if cap == 'default' else key.size // 16)
    finally:
        ctx.set_option('cover_cap_rows', 0)
        ctx.cover_begin(-1)
    print(f'{order}, {cap}: {got[0].size} ranges, {spills} spills')
    assert spills == 0 if cap == 'default' else spills > 0
    assert got[0].size == gold['n_ranges']
    assert T.rows_digest(*got) == gold['sha256']


def test_small_fetch_is_an_error_and_reset_starts_over(pile):
    from woltka_amd import _native as nat
    import ctypes as C
    rng = np.random.default_rng(9)
    key = rng.integers(0, 50, 5000).astype(np.int32)
    beg = rng.integers(-100, 100000, 5000).astype(np.int32)
    end = (beg + rng.integers(0, 5, 5000)).astype(np.int32)
    # no "ex" block has been scanned
    n, full = C.c_int64(0), C.c_int(0)
    assert pile._lib.wk_dtok_cover_append(pile._h, C.byref(n),
                                          C.byref(full)) == nat.E_STATE
    pile.cover_add(key, beg, end)
    first = pile.cover_fetch()
    assert first[0].size > 1000
    small = [np.empty(first[0].size - 1, np.int32) for _ in range(3)]
    rc = pile._lib.wk_cover_fetch(pile._h, *(
        x.ctypes.data_as(C.POINTER(C.c_int32)) for x in small), small[0].size)
    assert rc == nat.E_CAPACITY
    # other rows in between, then the same rows after a reset
    pile.cover_add(key[::-1], end[::-1], (end + 7)[::-1])
    pile.cover_reset()
    assert pile.cover_fetch()[0].size == 0
    pile.cover_add(key, beg, end)
    again = pile.cover_fetch()
    with nat.Context(0) as fresh:
        fresh.cover_begin(0)
        fresh.cover_add(key, beg, end)
        other = fresh.cover_fetch()
    for a, b, c in zip(first, again, other):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- the command line ---------------------------------------------------------

def _workflow(**kw):
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    ROUTES.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**kw)
    return dict(ROUTES)


def _on_device(routes, blocks=1):
    assert routes.get('dcover', 0) >= blocks, routes
    assert routes.get('host_block', 0) == 0, routes
    assert routes.get('dcover_flush', 0) >= 1, routes


@pytest.mark.parametrize('block', [1 << 26, 1 << 14])
@pytest.mark.parametrize('case', T.RUN_CASES, ids=T.run_label)
def test_runs_match_the_reference_on_the_device_route(tmp_path, monkeypatch,
                                                      case, block):
    from woltka_amd import classify as C
    monkeypatch.delenv('WOLTKA_NO_DCOVER', raising=False)
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', block)
    indir = str(tmp_path / 'aln')
    T.write_inputs(case, indir)
    routes = _workflow(**T.run_kwargs(case, indir, str(tmp_path)))
    assert T.run_digests(str(tmp_path)) == GOLD['runs'][T.run_label(case)]
    # every block of every file: nothing for the host tokenizer in these
    _on_device(routes, T.TEXT_SAMPLES * (1 if block == 1 << 26 else 50))
    assert routes['dcover_flush'] == T.TEXT_SAMPLES, routes


@pytest.mark.parametrize('case', [T.RUN_CASES[0], T.RUN_CASES[5],
                                  T.RUN_CASES[9]], ids=T.run_label)
def test_runs_with_a_pile_that_spills(tmp_path, monkeypatch, case):
    from woltka_amd import classify as C
    monkeypatch.delenv('WOLTKA_NO_DCOVER', raising=False)
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 20)
    monkeypatch.setattr(C.Engine, 'COVER_CAP_ROWS', 4096)
    indir = str(tmp_path / 'aln')
    T.write_inputs(case, indir)
    routes = _workflow(**T.run_kwargs(case, indir, str(tmp_path)))
    assert T.run_digests(str(tmp_path)) == GOLD['runs'][T.run_label(case)]
    _on_device(routes, T.TEXT_SAMPLES)
    assert routes.get('dcover_spill', 0) > 0, routes


def _read_cov(dir_):
    return {x[:-4]: open(join(dir_, x)).read()
            for x in sorted(os.listdir(dir_))}


def _profile(path):
    with open(path) as fh:
        head = fh.readline().rstrip('\n').split('\t')[1:]
        got = {s: {} for s in head}
        for line in fh:
            row = line.rstrip('\n').split('\t')
            for s, v in zip(head, row[1:]):
                if v != '0':
                    got[s][row[0]] = int(v)
    return got


def _plain_bowtie2(tmp_path):
    indir = tmp_path / 'bowtie2'
    indir.mkdir()
    for fn in sorted(os.listdir(join(ALN, 'bowtie2'))):
        with lzma.open(join(ALN, 'bowtie2', fn), 'rb') as src, \
                open(indir / fn[:-3], 'wb') as dst:
            dst.write(src.read())
    return str(indir)


@pytest.mark.parametrize('name,covfmt', [('bowtie2', None),
                                         ('bowtie2_gff', 'gff')])
def test_bundled_bowtie2_as_plain_sam(tmp_path, monkeypatch, name, covfmt):
    monkeypatch.delenv('WOLTKA_NO_DCOVER', raising=False)
    gold = COVERAGE['runs'][name]
    routes = _workflow(input_fp=_plain_bowtie2(tmp_path),
                       output_fp=str(tmp_path / 'out.tsv'),
                       outcov_dir=str(tmp_path / 'cov'), outcov_fmt=covfmt)
    assert _read_cov(str(tmp_path / 'cov')) == gold['cov']
    assert _profile(tmp_path / 'out.tsv') == gold['profile']
    _on_device(routes, 5)


def test_exclude_and_demux_keep_the_host_route(tmp_path, monkeypatch):
    monkeypatch.delenv('WOLTKA_NO_DCOVER', raising=False)
    # `--exclude`: the golden of tests/test_gpu_cli.py's case, plain text here
    indir = tmp_path / 'bt2sho'
    indir.mkdir()
    for fn in sorted(os.listdir(join(ALN, 'bt2sho'))):
        opener = lzma.open if fn.endswith('.xz') else open
        with opener(join(ALN, 'bt2sho', fn), 'rb') as src, \
                open(indir / (fn[:-3] if fn.endswith('.xz') else fn),
                     'wb') as dst:
            dst.write(src.read())
    routes = _workflow(input_fp=str(indir), exclude='G000215745',
                       output_fp=str(tmp_path / 'a.tsv'),
                       outcov_dir=str(tmp_path / 'cova'))
    assert routes.get('dcover', 0) == 0 and \
        routes.get('dcover_flush', 0) == 0, routes
    gold = COVERAGE['runs']['bt2sho_exclude']
    assert _read_cov(str(tmp_path / 'cova')) == gold['cov']
    assert _profile(tmp_path / 'a.tsv') == gold['profile']
    # `--demux`: a multiplexed file, two of its samples
    mux = tmp_path / 'mux.sam'
    with open(mux, 'w') as out:
        for i in range(1, 6):
            with lzma.open(join(ALN, 'bowtie2', f'S0{i}.sam.xz'), 'rt') as f:
                for line in f:
                    if line[0] != '@':
                        out.write(f'S0{i}_{line}')
    ids = tmp_path / 'ids.txt'
    ids.write_text('S02\nS04\n')
    routes = _workflow(input_fp=str(mux), demux=True, samples=str(ids),
                       output_fp=str(tmp_path / 'b.tsv'),
                       outcov_dir=str(tmp_path / 'covb'))
    assert routes.get('dcover', 0) == 0 and \
        routes.get('dcover_flush', 0) == 0, routes
    gold = COVERAGE['runs']['bowtie2']['cov']
    assert _read_cov(str(tmp_path / 'covb')) == {
        s: gold[s] for s in ('S02', 'S04')}


def test_switch_keeps_todays_route_and_the_bytes(tmp_path, monkeypatch):
    monkeypatch.setenv('WOLTKA_NO_DCOVER', '1')
    case = T.RUN_CASES[1]
    indir = str(tmp_path / 'aln')
    T.write_inputs(case, indir)
    routes = _workflow(**T.run_kwargs(case, indir, str(tmp_path)))
    assert routes.get('dcover', 0) == 0 and \
        routes.get('dcover_flush', 0) == 0, routes
    assert T.run_digests(str(tmp_path)) == GOLD['runs'][T.run_label(case)]
