"""The read maps under demultiplexing the device writes
(csrc/wk_readmap_demux.hpp: the demux variants of the two formatters' kernels
and the partition readmap_demux_*; `_run_dreads_demux` and
`_device_maps_demux` of routes/device_text.py) against the reference's own
text: tests/golden/vectors/readmap_demux_device.json holds what
`workflow.workflow(..., outmap_dir=...)` of the reference wrote for the cases
of tests/readmap_demux_cases.py (tests/golden/make_readmap_demux_reference.py).
tests/test_readmap_demux_host.py holds the host route to the same texts.

a. the partition alone (`Context.readmap_demux_partition`) against
   `numpy.argsort(kind='stable')` and `cumsum`: 1, tile - 1, tile, tile + 1
   and 3 tiles + 1 reads, 17 and 34 tiles (the column scan's strips of several
   tiles), all lengths 0, lengths 0 interleaved, one sample, a
   sample per read, ids sparse in 0 .. 65 535, reads without a line; the
   capacity option one below tiles x samples: refused, nothing written;
b. whole commands -- every kind of job set, `--unassigned`, `--name-as-id`,
   `--trim-sub`, `--exclude`, `--samples`, all four formats, mates, gzip,
   `--zipmap none`, a directory under `--demux`, 66 samples over 8 KB blocks
   -- with the route asserted (`ROUTES['dreads_demux']`, and no other key
   that counts blocks of the device text route), and once more with
   ``WOLTKA_NO_DDEMUXMAPS=1``;
c. blocks handed to the host inside one file: a read of 4096 subjects in the
   middle block, a sample table that is full from the second block on, a
   partition whose capacity no block meets."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_demux_cases as T         # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('readmap_demux_device.json')
T.check_gold(GOLD)
CLI = {c['name']: c for c in T.cli_cases()}
assert set(GOLD['cli']) == {c['gold'] for c in CLI.values()}
PART = T.partition_cases()
# the keys that count blocks of the device text route (tests/cli_routes_cases.py)
BLOCK_KEYS = ('dtok', 'dtok_maps', 'dreads_maps', 'dreads_lists', 'dcover',
              'ddemux', 'dhits', 'dhits_strata', 'dhits_demux',
              'dreads_strata')


# ---- a. the partition -------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from woltka_amd import _native as nat
    assert nat.READMAP_DEMUX_TILE == T.TILE
    c = nat.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('name', list(PART))
def test_partition_is_the_stable_sort_by_sample(ctx, name):
    samp, length = PART[name]
    ctx.set_option('readmap_demux_cap', 0)
    status, off, seg, total = ctx.readmap_demux_partition(samp, length)
    want_off, want_seg, want_total = T.partition_model(samp, length)
    assert status == 0
    assert total == want_total
    assert np.array_equal(seg, want_seg), (seg[:4], want_seg[:4])
    assert np.array_equal(off, want_off), \
        np.flatnonzero(off != want_off)[:8]
    # (once more: no state of the first run is in the second)
    again = ctx.readmap_demux_partition(samp, length)
    assert again[0] == 0 and np.array_equal(again[1], off) and \
        np.array_equal(again[2], seg) and again[3] == total


def test_partition_beyond_its_capacity_is_refused(ctx):
    samp, length = PART[f'n{3 * T.TILE + 1}']
    tiles, cols = 4, np.unique(samp).size
    try:
        ctx.set_option('readmap_demux_cap', tiles * cols - 1)
        assert ctx.readmap_demux_partition(samp, length) == \
            (1, None, None, None)
        # ... and nothing is written: the entry itself, on arrays filled
        # beforehand
        import ctypes as C
        fill = np.uint64(0xA5A5A5A5A5A5A5A5)
        off = np.full(samp.size, fill, dtype=np.uint64)
        seg = np.full((cols, 3), fill, dtype=np.uint64)
        k, total, st = C.c_int32(-7), C.c_uint64(int(fill)), C.c_int(-7)
        u64p = C.POINTER(C.c_uint64)
        rc = ctx._lib.wk_readmap_demux_partition(
            ctx._h, samp.ctypes.data_as(C.POINTER(C.c_int32)),
            length.ctypes.data_as(u64p), samp.size, off.ctypes.data_as(u64p),
            seg.ctypes.data_as(u64p), cols, C.byref(k), C.byref(total),
            C.byref(st))
        assert rc == 0 and st.value == 1
        assert (off == fill).all() and (seg == fill).all()
        assert k.value == -7 and total.value == int(fill)
        ctx.set_option('readmap_demux_cap', tiles * cols)
        status, off, _, _ = ctx.readmap_demux_partition(samp, length)
        assert status == 0 and \
            np.array_equal(off, T.partition_model(samp, length)[0])
    finally:
        ctx.set_option('readmap_demux_cap', 0)


# ---- b. commands ------------------------------------------------------------------
def _run(case, tmp_path, monkeypatch, cap=None):
    from woltka_amd import _native as nat
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    for var in ('WOLTKA_NO_DTOK', 'WOLTKA_NO_DDEMUX'):
        monkeypatch.delenv(var, raising=False)
    if case['block']:
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', case['block'])
    if case['max_samples'] or cap is not None:
        begin = nat.Context.demux_begin

        def options(self, on=True):
            if case['max_samples']:
                self.set_option('demux_max_samples', case['max_samples'])
            if cap is not None:
                self.set_option('readmap_demux_cap', cap)
            return begin(self, on)
        monkeypatch.setattr(nat.Context, 'demux_begin', options)
    ROUTES.clear()
    got = T.run_cli(workflow, case, str(tmp_path))
    return got, dict(ROUTES)


def _check(name, got):
    want = GOLD['cli'][CLI[name]['gold']]
    assert sorted(got['maps']) == sorted(want['maps'])
    for k, text in sorted(got['maps'].items()):
        T.compare(text, want['maps'][k], f'{name} {k}')
    assert got['tables'] == want['tables']


@pytest.mark.parametrize('name', list(CLI))
def test_commands_write_the_reference_maps(tmp_path, monkeypatch, name):
    case = CLI[name]
    monkeypatch.delenv('WOLTKA_NO_DDEMUXMAPS', raising=False)
    got, routes = _run(case, tmp_path, monkeypatch)
    _check(name, got)
    blocks = T.n_blocks(case)
    print(name, 'blocks', blocks, 'dreads_demux',
          routes.get('dreads_demux', 0), 'host_block',
          routes.get('host_block', 0))
    assert routes.get('dreads_demux', 0) > 0, routes
    assert not any(routes.get(k) for k in BLOCK_KEYS), routes
    if case['host_blocks'] is None:
        # (the table is full from the second block on: the rest is the host's)
        assert routes['dreads_demux'] == 1 and \
            routes.get('host_block', 0) == blocks - 1 > 1, routes
    else:
        assert routes.get('host_block', 0) == case['host_blocks'], routes
        if blocks is not None:
            assert routes['dreads_demux'] == blocks - case['host_blocks'], \
                routes


@pytest.mark.parametrize('name', list(CLI))
def test_commands_write_the_same_maps_with_the_route_off(tmp_path,
                                                         monkeypatch, name):
    monkeypatch.setenv('WOLTKA_NO_DDEMUXMAPS', '1')
    got, routes = _run(CLI[name], tmp_path, monkeypatch)
    _check(name, got)
    assert routes.get('dreads_demux', 0) == 0, routes
    assert not any(routes.get(k) for k in BLOCK_KEYS), routes


# ---- c. hand-offs -----------------------------------------------------------------
@pytest.mark.parametrize('name', ['late', 'late-lists'])
def test_a_partition_no_block_fits_leaves_the_file_to_the_host(
        tmp_path, monkeypatch, name):
    """`readmap_demux_cap` = 1: every block of more than one sample is
    refused at its staging (status 4), before anything is counted; the files
    and the tables are the reference's."""
    monkeypatch.delenv('WOLTKA_NO_DDEMUXMAPS', raising=False)
    got, routes = _run(CLI[name], tmp_path, monkeypatch, cap=1)
    _check(name, got)
    assert routes.get('dreads_demux', 0) == 0 and \
        routes.get('host_block', 0) == T.n_blocks(CLI[name]), routes


def test_device_and_host_blocks_share_the_files_in_order(tmp_path,
                                                         monkeypatch):
    """Every second block is refused (the capacity alternates between none
    and the default): the runs of the device blocks and the lines of the host
    blocks land in the same files, in file order."""
    from woltka_amd import _native as nat
    monkeypatch.delenv('WOLTKA_NO_DDEMUXMAPS', raising=False)
    stage = nat.Context.dtok_stage_reads_samples
    calls = []

    def every_other(self):
        calls.append(len(calls))
        self.set_option('readmap_demux_cap', len(calls) % 2)
        return stage(self)
    monkeypatch.setattr(nat.Context, 'dtok_stage_reads_samples', every_other)
    got, routes = _run(CLI['late-lists'], tmp_path, monkeypatch)
    _check('late-lists', got)
    assert routes.get('dreads_demux', 0) == 2 == routes.get('host_block', 0), \
        routes
