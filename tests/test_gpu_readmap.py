"""The read maps the device writes (csrc/wk_readmap.hpp: readmap_len_kernel,
the u64_tile_* scan, readmap_write_kernel; `_sync_map_tables` and
`_device_maps` of routes/device_text.py) against the reference's own text:
tests/golden/vectors/readmap_device.json holds what `workflow.workflow(...,
outmap_dir=...)` of the reference wrote for the cases of
tests/readmap_cases.py (tests/golden/make_readmap_reference.py).  The random CLI
vectors never reach this writer (every one of their `--outmap` cases takes a
host route), and the other tests that do compare it with this package's own
host formatter: this module is where `dtok_maps` meets the reference.
tests/test_readmap_host.py holds the host formatters to the same texts.

a. whole commands, with the route asserted from the case's construction.
   The map ring of `_device_maps` is watched (`_watch`): every call of
   `dtok_readmap` says whether its text lay inside the ring's buffer, every
   buffer taken is counted, and so is every time the ring had none to give.
   In `blocks` the compressor is held back until that has happened, so the
   wait of the 6-buffer ring runs; in its 4 KB-slot variant no text fits and
   no buffer is ever taken;
b. single blocks through `Context.dtok_readmap` with tables built by the plain
   model of readmap_cases (`tables_of`), among them blocks of 1 .. 2 097 153
   reads: the edges of the scan's tiles of 256 reads and of the 8192 tiles
   after which `tile_scan_kernel` carries;
c. the fixture still holds the edges the cases are made for (checked when the
   module is imported, on the CPU).

A count of 16 cannot come from the device: a read has at most 16 subjects
there, and 16 subjects of one taxon make a line without counts.  `digits` goes
up to 15; the `:16` is the 17-subject read of `handoff-big`, which the host
formats into the same file."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_cases as T               # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('readmap_device.json')
T.check_gold(GOLD)                      # (c)
CLI = {c['name']: c for c in T.cli_cases()}
assert set(GOLD['cli']) == set(CLI) and \
    set(GOLD['blocks']) == set(T.block_cases())
GENUS = T.genus_of()


# ---- a. commands ------------------------------------------------------------------
def _watch(monkeypatch, hold):
    """Spies on the map ring and on `dtok_readmap`.  Returns {'dry': times the
    ring had no buffer free, 'takes': buffers handed to a text, 'inside': what
    every `dtok_readmap` said}.  ``hold``: no gzip member is made before the
    ring has run dry once (then the wait loop of `_device_maps` has to drain
    the writer to go on; 30 s at the most, so that a ring that never runs dry
    fails the assertion on 'dry' and hangs nothing)."""
    import threading
    from woltka_amd import _native as nat
    from woltka_amd import classify as C
    from woltka_amd import hostio, pgzip
    seen = {'dry': 0, 'takes': 0, 'inside': []}
    dry = threading.Event()
    ring = hostio.StageRing

    def is_map_ring(r):
        return len(r._bufs) == 6 and \
            r.layout.get('text', (None, 0))[1] == C.Engine.MAP_TEXT_SLOT
    try_current, take, readmap = ring.try_current, ring.take, \
        nat.Context.dtok_readmap

    def spy_try(self):
        got = try_current(self)
        if got is None and is_map_ring(self):
            seen['dry'] += 1
            dry.set()
        return got

    def spy_take(self):
        if is_map_ring(self):
            seen['takes'] += 1
        return take(self)

    def spy_readmap(self, job, out=None):
        text, inside = readmap(self, job, out=out)
        seen['inside'].append(bool(inside))
        return text, inside
    monkeypatch.setattr(ring, 'try_current', spy_try)
    monkeypatch.setattr(ring, 'take', spy_take)
    monkeypatch.setattr(nat.Context, 'dtok_readmap', spy_readmap)
    if hold:
        member = pgzip.member

        def held(data, *a, **kw):
            dry.wait(30)
            return member(data, *a, **kw)
        monkeypatch.setattr(pgzip, 'member', held)
    return seen


@pytest.mark.parametrize('name', list(CLI))
def test_commands_write_the_reference_maps(tmp_path, monkeypatch, name):
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    case = CLI[name]
    monkeypatch.delenv('WOLTKA_NO_DTOK', raising=False)
    if case['block']:
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', case['block'])
    if case['slot']:
        monkeypatch.setattr(C.Engine, 'MAP_TEXT_SLOT', case['slot'])
    seen = _watch(monkeypatch, hold=name == 'blocks')
    ROUTES.clear()
    got = T.run_cli(workflow, case, str(tmp_path))
    routes = dict(ROUTES)
    want = GOLD['cli'][name]
    assert sorted(got['maps']) == sorted(want['maps'])
    for k, text in sorted(got['maps'].items()):
        T.compare(text, want['maps'][k], f'{name} {k}',
                  model=lambda: T.model_maps(case)[k])
    assert got['tables'] == want['tables']
    blocks = T.n_blocks(case)
    print(name, 'blocks', blocks, 'dtok_maps', routes.get('dtok_maps', 0),
          'host_block', routes.get('host_block', 0), 'ring dry', seen['dry'],
          'taken', seen['takes'], 'texts', len(seen['inside']))
    # one text per device block and rank; inside the ring's buffer, which is
    # then taken, unless the slot is smaller than any block's text
    texts = routes.get('dtok_maps', 0) * len(case['kwargs']['ranks'].split(','))
    assert len(seen['inside']) == texts > 0
    if case['slot']:
        assert not any(seen['inside']) and seen['takes'] == 0
    else:
        assert all(seen['inside']) and seen['takes'] == texts
    if name == 'blocks':
        assert seen['dry'] > 0      # the 6 buffers were all out, and the run went on
    if case['route'] == 'device':
        assert routes.get('dtok_maps', 0) == blocks and \
            routes.get('host_block', 0) == 0, routes
    elif name == 'handoff-big':
        # the block of the read of 17 subjects, and only it
        assert routes.get('host_block', 0) == 1 and \
            routes.get('dtok_maps', 0) == blocks - 1, routes
    else:
        # from the block that brings the subject without a genus
        first = T.block_of(case, T.MISSING.encode())
        assert routes.get('dtok_maps', 0) == first > 0 and \
            routes.get('host_block', 0) == blocks - first > 0, routes


# ---- b. the direct door -------------------------------------------------------------
class Device:
    """One context and one tokenizer for the whole module: the tokenizer's
    dictionary grows from case to case, and every case's tables cover all of
    it, as `_sync_map_tables` does."""

    def __init__(self):
        from woltka_amd import _native as nat
        self.nat = nat
        self.ctx = nat.Context(0)
        self.tok = nat.Tokenizer(2)
        self.ctx.counts_reserve(1 << 16)
        self.jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)]
        self.subjects = []

    def emit(self, text, fmt):
        """One block: scanned, its subjects registered, its records appended
        under one rank-none job (what `_run_dtok` does in front of
        `dtok_emit`).  Returns the number of reads."""
        ctx, nat = self.ctx, self.nat
        arr = np.frombuffer(text, dtype=np.uint8)
        ctx.dtok_format(fmt)
        ctx.dtok_keep_reads(True)
        ok, begin, stop, _ = nat.Tokenizer.sam_span(arr, True, fmt == 'sam',
                                                    fmt, False)
        assert ok and stop == arr.size
        status, n_lines = ctx.dtok_scan(self.tok, arr, begin, stop)
        assert status == 0 and n_lines > 0
        self.subjects.extend(self.tok.new_subjects())
        ctx.set_subjects(np.arange(len(self.subjects), dtype=np.int32))
        assert ctx.words_begin(self.jobs, 0)
        status, n_reads, _ = ctx.dtok_emit()
        assert status == 0
        return n_reads

    def maps(self, job, tax, namedic=None, subjects=None):
        slot, order, shown = T.tables_of(
            self.subjects if subjects is None else subjects, tax, namedic)
        self.ctx.readmap_tables(job, slot, order, shown)
        return self.ctx.dtok_readmap(job)[0].tobytes()

    def done(self):
        self.ctx.words_flush()
        self.ctx.counts_clear()

    def close(self):
        self.tok.close()
        self.ctx.close()


@pytest.fixture(scope='module')
def dev():
    d = Device()
    yield d
    d.close()


def _door_case(name):
    case = CLI[name]
    (rel,) = [k for k in case['files'] if k.startswith('aln/')]
    return (case['files'][rel], case['kwargs']['input_fmt'],
            T.names_of() if case['kwargs'].get('name_as_id') else None)


@pytest.mark.parametrize('name', T.DOOR_CASES)
def test_one_block_gives_the_reference_text(dev, name):
    """A job with `genus` tables next to one with `none`, both after one
    emit."""
    text, fmt, namedic = _door_case(name)
    gold = GOLD['cli'][name]['maps']
    n_reads = dev.emit(text, fmt)
    try:
        none = dev.maps(0, None, namedic)
        genus = dev.maps(1, GENUS, namedic)
        again = dev.ctx.dtok_readmap(0)[0].tobytes()
    finally:
        dev.done()
    assert n_reads == gold['none/S.txt'].count('\n')
    T.compare(none, gold['none/S.txt'], f'{name} none')
    T.compare(genus, gold['genus/S.txt'], f'{name} genus')
    assert again == none and none != genus


@pytest.mark.parametrize('name', list(T.block_cases()))
def test_block_sizes_around_the_tiles_of_the_scan(dev, name):
    n = T.block_cases()[name]
    want = GOLD['blocks'][name]
    assert dev.emit(T.block_text(n), 'map') == n
    try:
        got = dev.maps(0, GENUS)
    finally:
        dev.done()
    have = T.digest(got)
    print(name, have['bytes'], have['lines'], have['sha256'])
    assert (have['bytes'], have['lines']) == (want['bytes'], want['lines'])
    T.compare(got, want, name, model=lambda: T.block_map_text(n))
    assert have['sha256'] == want['sha256']


def test_readmap_refuses_what_it_promises_to_refuse(dev):
    """`dtok_readmap` before any block is emitted, and with tables that cover
    fewer subjects than the context has (WK_E_STATE)."""
    ctx = dev.ctx
    ctx.dtok_keep_reads(False)          # (forgets the block emitted last)
    ctx.dtok_keep_reads(True)
    with pytest.raises(RuntimeError, match='no block emitted'):
        ctx.dtok_readmap(0)
    text, fmt, _ = _door_case('digits')
    dev.emit(text, fmt)
    try:
        assert len(dev.subjects) > 1
        with pytest.raises(RuntimeError, match='cover'):
            dev.maps(2, GENUS, subjects=dev.subjects[:-1])
        T.compare(dev.maps(2, GENUS), GOLD['cli']['digits']['maps']['genus/S.txt'],
                  'digits genus, full tables')
    finally:
        dev.done()
