"""The read maps of whole-read assignments the device writes
(csrc/wk_readmap_reads.hpp: readmap_leaders_kernel, readmap_reads_len_kernel,
the u64_tile_* scan, readmap_reads_write_kernel; `_run_dreads_maps`,
`_sync_shown` and `_device_maps` of routes/device_text.py) against the
reference's own text: tests/golden/vectors/readmap_reads_device.json holds
what `workflow.workflow(..., outmap_dir=...)` of the reference wrote for the
cases of tests/readmap_reads_cases.py
(tests/golden/make_readmap_reads_reference.py).
tests/test_readmap_reads_host.py holds the host formatter to the same texts.

a. whole commands -- `--rank free`, `--uniq`, `--above`, `--major`, one and
   three ranks, with and without `--unassigned`, `--name-as-id`, all four
   formats, gzip, `--trim-sub`, `--exclude`, `--zipmap none`, many blocks with
   a shown-text table that grows until the last one, a read of 4096 subjects
   handed to the host, a map ring no text fits -- with the route asserted
   from the case's construction (`ROUTES['dreads_maps']`, which today's code
   never counts), and once more with ``WOLTKA_NO_DREADMAPS=1``;
b. single blocks through `dtok_stage_reads_plain`, `classify_staged_keep`,
   `readmap_reads_tables` and `dtok_readmap_reads` on one context: 1 .. 65 537
   reads (the edges of the scan's tiles of 256 reads, and one past a tile of
   tiles), a block in which no read is assigned, one in which only the last
   is; the table extended between two blocks; the codes of `classify_staged`
   with a host pointer on the same staged chunk."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_reads_cases as T         # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('readmap_reads_device.json')
T.check_gold(GOLD)
CLI = {c['name']: c for c in T.cli_cases()}
assert set(GOLD['cli']) == {c['gold'] for c in CLI.values()} and \
    set(GOLD['blocks']) == set(T.block_cases())


# ---- a. commands ------------------------------------------------------------------
def _spy(monkeypatch):
    """What every `dtok_readmap_reads` said about its text lying inside the
    map ring's buffer."""
    from woltka_amd import _native as nat
    inside = []
    readmap = nat.Context.dtok_readmap_reads

    def spy(self, job, out=None):
        text, ok = readmap(self, job, out=out)
        inside.append(bool(ok))
        return text, ok
    monkeypatch.setattr(nat.Context, 'dtok_readmap_reads', spy)
    return inside


def _run(case, tmp_path, monkeypatch):
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    monkeypatch.delenv('WOLTKA_NO_DTOK', raising=False)
    if case['block']:
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', case['block'])
    if case['slot']:
        monkeypatch.setattr(C.Engine, 'MAP_TEXT_SLOT', case['slot'])
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
    monkeypatch.delenv('WOLTKA_NO_DREADMAPS', raising=False)
    inside = _spy(monkeypatch)
    got, routes = _run(case, tmp_path, monkeypatch)
    _check(name, got)
    n_files = sum(k.startswith('aln/') for k in case['files'])
    blocks = T.n_blocks(case)
    print(name, 'blocks', blocks, 'dreads_maps', routes.get('dreads_maps', 0),
          'host_block', routes.get('host_block', 0), 'texts', len(inside))
    assert routes.get('host_block', 0) == case['host_blocks'], routes
    assert routes.get('dtok_maps', 0) == 0, routes
    if blocks is None:
        assert routes.get('dreads_maps', 0) >= n_files, routes
    else:
        assert routes.get('dreads_maps', 0) == blocks - case['host_blocks'] \
            > 0, routes
    # one text per device block and rank; inside the ring's buffer unless the
    # slot is smaller than any block's text
    assert len(inside) == routes['dreads_maps'] * len(T.map_ranks(case))
    if case['slot']:
        assert not any(inside)
    else:
        assert all(inside)


@pytest.mark.parametrize('name', list(CLI))
def test_commands_write_the_same_maps_with_the_route_off(tmp_path,
                                                         monkeypatch, name):
    monkeypatch.setenv('WOLTKA_NO_DREADMAPS', '1')
    got, routes = _run(CLI[name], tmp_path, monkeypatch)
    _check(name, got)
    assert routes.get('dreads_maps', 0) == 0, routes


def test_plain_jobs_keep_their_route(tmp_path, monkeypatch):
    """A set of plain jobs only is `dtok_maps`' as before."""
    monkeypatch.delenv('WOLTKA_NO_DREADMAPS', raising=False)
    case = dict(CLI['genus-uniq'])
    case['kwargs'] = dict(case['kwargs'], uniq=False)
    _, routes = _run(case, tmp_path, monkeypatch)
    assert routes.get('dreads_maps', 0) == 0, routes


# ---- b. the direct door -------------------------------------------------------------
class Device:
    """One context and one tokenizer for the whole module: the tokenizer's
    dictionary grows from block to block, a subject's feature is its index,
    and the shown-text table is extended by the names a block brings, as
    `_sync_shown` does."""

    def __init__(self):
        from woltka_amd import _native as nat
        self.nat = nat
        self.ctx = nat.Context(0)
        self.tok = nat.Tokenizer(2)
        self.ctx.counts_reserve(1 << 18)
        self.ctx.dtok_format('map')
        self.subjects = []
        self.shown = 0

    def jobs(self, unassigned=False):
        nat = self.nat
        return [nat.Job(nat.MODE_NONE, 0, nat.F_UNIQ |
                        (nat.F_UNASSIGNED if unassigned else 0), 0, 0.0)]

    def table(self, names, first):
        enc = [x.encode() for x in names]
        off = np.zeros(len(enc) + 1, dtype=np.uint32)
        np.cumsum([len(x) for x in enc], out=off[1:])
        self.ctx.readmap_reads_tables(
            first, np.frombuffer(b''.join(enc), dtype=np.uint8), off)

    def stage(self, text, extend=True):
        """One block: scanned, its subjects registered and shown, staged as
        the classify chunk.  Returns the number of reads."""
        ctx, nat = self.ctx, self.nat
        arr = np.frombuffer(text, dtype=np.uint8)
        ok, begin, stop, _ = nat.Tokenizer.sam_span(arr, True, False, 'map',
                                                    False)
        assert ok and stop == arr.size
        status, n_lines = ctx.dtok_scan(self.tok, arr, begin, stop)
        assert status == 0 and n_lines > 0
        self.subjects.extend(self.tok.new_subjects())
        ctx.set_subjects(np.arange(len(self.subjects), dtype=np.int32))
        if extend and self.shown < len(self.subjects):
            self.table(self.subjects[self.shown:], self.shown)
            self.shown = len(self.subjects)
        status, n_reads, _ = ctx.dtok_stage_reads_plain()
        assert status == 0
        ctx.set_uniform_group(0)
        return n_reads

    def maps(self, unassigned=False):
        self.ctx.classify_staged_keep(self.jobs(unassigned))
        return self.ctx.dtok_readmap_reads(0)[0].tobytes()

    def close(self):
        self.tok.close()
        self.ctx.close()


@pytest.fixture(scope='module')
def dev():
    d = Device()
    yield d
    d.close()


@pytest.mark.parametrize('name', list(T.block_cases()))
def test_block_sizes_around_the_tiles_of_the_scan(dev, name):
    n = T.block_cases()[name]
    want = GOLD['blocks'][name]
    assert dev.stage(T.block_text(n)) == n
    got = dev.maps()
    have = T.digest(got)
    print(name, have['bytes'], have['lines'], have['sha256'])
    T.compare(got, want, name, model=lambda: T.block_map_text(n))
    assert got == T.block_map_text(n)
    if n == 65537:
        assert have['sha256'] == want['sha256']


@pytest.mark.parametrize('n', (1, 255, 256, 257, 65537))
def test_blocks_in_which_no_read_or_only_the_last_is_assigned(dev, n):
    assert dev.stage(T.block_text(n, 'nobody')) == n
    dev.ctx.classify_staged_keep(dev.jobs())
    text, inside = dev.ctx.dtok_readmap_reads(
        0, out=np.empty(16, dtype=np.uint8))
    assert text.size == 0 and inside         # n_bytes == 0: nothing to fetch
    assert dev.maps(unassigned=True) == \
        T.block_map_text(n, 'nobody', unassigned=True)
    assert dev.stage(T.block_text(n, 'last')) == n
    got = dev.maps()
    assert got == T.block_map_text(n, 'last') and got.count(b'\n') == 1
    assert dev.maps(unassigned=True) == \
        T.block_map_text(n, 'last', unassigned=True)


def test_the_table_grows_between_two_blocks(dev):
    """The first block's text, fetched before the table is extended by the
    second block's subjects, stays what it was; the second block shows the
    new subjects; setting the whole table anew gives the same text again."""
    tag = f'grow{len(dev.subjects)}'
    one = T.map_text([(f'q{i}', [f'{tag}a{i % 7}']) for i in range(300)])
    two = T.map_text([(f'p{i}', [f'{tag}b{i % 5}' if i % 2 else
                                 f'{tag}a{i % 7}']) for i in range(300)])
    assert dev.stage(one) == 300
    first = dev.maps()
    kept = bytes(first)
    before = dev.shown
    assert dev.stage(two) == 300
    second = dev.maps()
    assert dev.shown == before + 5           # (the five `b` subjects)
    assert first == kept == b''.join(
        f'q{i}\t{tag}a{i % 7}\n'.encode() for i in range(300))
    want = b''.join((f'p{i}\t{tag}b{i % 5}\n' if i % 2 else
                     f'p{i}\t{tag}a{i % 7}\n').encode() for i in range(300))
    assert second == want
    dev.table(dev.subjects, 0)
    assert dev.ctx.dtok_readmap_reads(0)[0].tobytes() == want


def test_a_code_outside_the_table_is_refused(dev):
    """A block whose subjects the table does not cover yet gives no text
    (WK_E_STATE); extended, it does."""
    tag = f'late{len(dev.subjects)}'
    text = T.map_text([(f'q{i}', [f'{tag}{i % 3}']) for i in range(10)])
    assert dev.stage(text, extend=False) == 10
    dev.ctx.classify_staged_keep(dev.jobs())
    with pytest.raises(RuntimeError, match='no single feature'):
        dev.ctx.dtok_readmap_reads(0)
    dev.table(dev.subjects[dev.shown:], dev.shown)
    dev.shown = len(dev.subjects)
    assert dev.ctx.dtok_readmap_reads(0)[0].tobytes() == b''.join(
        f'q{i}\t{tag}{i % 3}\n'.encode() for i in range(10))


def test_classify_staged_with_a_host_pointer_gives_the_same_codes(dev):
    """The old contract on a chunk of this route: `classify_staged(...,
    want_assign=True)` returns the codes the formatter used, and forgets
    nothing it should keep -- but the codes it leaves are no longer the
    kept ones, so the formatter asks for `classify_staged_keep` again."""
    nat = dev.nat
    n = 1000
    reads = T.block_reads(n, 'all')
    reads = [(q, s if i % 3 else s + [T.BLOCK_SUBJECTS[(i + 5) % 30]])
             for i, (q, s) in enumerate(reads)]
    assert dev.stage(T.map_text(reads)) == n
    text = dev.maps()
    codes = dev.ctx.classify_staged(dev.jobs(), want_assign=True)
    assert codes.shape == (1, n)
    where = {s: i for i, s in enumerate(dev.subjects)}
    want = np.asarray([where[s[0]] if len(s) == 1 else nat.ASSIGN_NONE
                       for _, s in reads], dtype=np.int32)
    assert np.array_equal(codes[0], want)
    lines = [f'{q}\t{dev.subjects[v]}\n' for (q, _), v in
             zip(reads, codes[0].tolist()) if v >= 0]
    assert text == ''.join(lines).encode()
    with pytest.raises(RuntimeError, match='codes are not on the device'):
        dev.ctx.dtok_readmap_reads(0)
    assert dev.maps() == text


def test_readmap_reads_refuses_a_chunk_of_another_kind(dev):
    ctx = dev.ctx
    assert dev.stage(T.block_text(2)) == 2      # (two subjects are registered)
    subj = np.asarray([0, 1], dtype=np.int32)
    ctx.chunk_stage(subj, np.asarray([0, 1, 2], dtype=np.int32), group=0,
                    subj_is_set=True, indexed=True)
    ctx.classify_staged_keep(dev.jobs())
    with pytest.raises(RuntimeError, match='wk_dtok_stage_reads_plain'):
        ctx.dtok_readmap_reads(0)
    ctx.counts_clear()
