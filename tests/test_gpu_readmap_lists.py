"""The read maps with taxon lists the device writes
(csrc/wk_readmap_lists.hpp: readmap_lists_build_kernel, the u64_tile_* scan,
readmap_lists_write_kernel; `_run_dreads_lists`, `_sync_shown` and
`_device_maps` of routes/device_text.py) against the reference's own text:
tests/golden/vectors/readmap_lists_device.json holds what
`workflow.workflow(..., outmap_dir=...)` of the reference wrote for the cases
of tests/readmap_lists_cases.py (tests/golden/make_readmap_lists_reference.py).
tests/test_readmap_lists_host.py holds the gate and the host formatter to the
same texts.

a. whole commands with the route on -- plain ranks under `--trim-sub` (with
   `--name-as-id`: the Method II recipe) and `--exclude`, sets that mix list
   jobs with whole-read jobs, `--unassigned`, `--zipmap none`, all four
   formats, gzip, many blocks with shown and id tables that grow until the
   last one, a read of 4096 subjects handed to the host, a map ring no text
   fits, reads of 2 .. 4095 subjects and counts of 1 .. 4 digits -- with the
   route asserted from the case's construction (`ROUTES['dreads_lists']`);
b. the same with ``WOLTKA_NO_DLISTMAPS=1``;
c. the neighbouring sets keep `dtok_maps` and `dreads_maps`;
d. single blocks through `dtok_stage_reads_plain`, `classify_staged_keep`,
   `readmap_reads_tables`, `readmap_lists_ids` and `dtok_readmap_lists` on one
   context against the plain model the fixture's digests pin."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_lists_cases as T         # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('readmap_lists_device.json')
T.check_gold(GOLD)
CLI = {c['name']: c for c in T.cli_cases()}
NEAR = {c['name']: c for c in T.neighbour_cases()}
assert set(GOLD['cli']) == {c['gold'] for c in CLI.values()} | set(NEAR) and \
    set(GOLD['blocks']) == set(T.block_cases())


# ---- a. b. c. commands --------------------------------------------------------------
def _spy(monkeypatch):
    """What every `dtok_readmap_lists` said about its text lying inside the
    map ring's buffer."""
    from woltka_amd import _native as nat
    inside = []
    readmap = nat.Context.dtok_readmap_lists

    def spy(self, job, out=None):
        text, ok = readmap(self, job, out=out)
        inside.append(bool(ok))
        return text, ok
    monkeypatch.setattr(nat.Context, 'dtok_readmap_lists', spy)
    return inside


def _run(case, tmp_path, monkeypatch):
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    for var in ('WOLTKA_NO_DTOK', 'WOLTKA_NO_DREADMAPS', 'WOLTKA_NO_DMAPS',
                'WOLTKA_NO_WORDS'):
        monkeypatch.delenv(var, raising=False)
    if case['block']:
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', case['block'])
    if case['slot']:
        monkeypatch.setattr(C.Engine, 'MAP_TEXT_SLOT', case['slot'])
    ROUTES.clear()
    got = T.run_cli(workflow, case, str(tmp_path))
    return got, dict(ROUTES)


def _check(case, got):
    want = GOLD['cli'][case['gold']]
    assert sorted(got['maps']) == sorted(want['maps'])
    for k, text in sorted(got['maps'].items()):
        T.compare(text, want['maps'][k], f'{case["name"]} {k}')
    assert got['tables'] == want['tables']


@pytest.mark.parametrize('name', list(CLI))
def test_commands_write_the_reference_maps(tmp_path, monkeypatch, name):
    case = CLI[name]
    monkeypatch.delenv('WOLTKA_NO_DLISTMAPS', raising=False)
    inside = _spy(monkeypatch)
    got, routes = _run(case, tmp_path, monkeypatch)
    _check(case, got)
    n_files = sum(k.startswith('aln/') for k in case['files'])
    blocks = T.n_blocks(case)
    print(name, 'blocks', blocks, 'dreads_lists',
          routes.get('dreads_lists', 0), 'host_block',
          routes.get('host_block', 0), 'texts', len(inside))
    assert routes.get('host_block', 0) == case['host_blocks'], routes
    assert routes.get('dtok_maps', 0) == 0 and \
        routes.get('dreads_maps', 0) == 0, routes
    if blocks is None:
        assert routes.get('dreads_lists', 0) >= n_files, routes
    else:
        assert routes.get('dreads_lists', 0) == \
            blocks - case['host_blocks'] > 0, routes
    # one text per device block and rank; inside the ring's buffer unless the
    # slot is smaller than any block's text
    assert len(inside) == routes['dreads_lists'] * len(T.map_ranks(case))
    if case['slot']:
        assert not any(inside)
    else:
        assert all(inside)


@pytest.mark.parametrize('name', list(CLI))
def test_commands_write_the_same_maps_with_the_route_off(tmp_path,
                                                         monkeypatch, name):
    monkeypatch.setenv('WOLTKA_NO_DLISTMAPS', '1')
    got, routes = _run(CLI[name], tmp_path, monkeypatch)
    _check(CLI[name], got)
    assert routes.get('dreads_lists', 0) == 0, routes


@pytest.mark.parametrize('name, key', [('plain-only', 'dtok_maps'),
                                       ('none-genus-uniq', 'dreads_maps')])
def test_neighbouring_sets_keep_their_routes(tmp_path, monkeypatch, name, key):
    """Plain jobs whose ids are the tokenizer's are R1's, a set without a list
    job is R1m's: the new key is not counted, theirs is."""
    monkeypatch.delenv('WOLTKA_NO_DLISTMAPS', raising=False)
    got, routes = _run(NEAR[name], tmp_path, monkeypatch)
    _check(NEAR[name], got)
    assert routes.get('dreads_lists', 0) == 0 and routes.get(key, 0) > 0, \
        routes


# ---- d. the direct door -------------------------------------------------------------
def shown_name(x):
    """A name whose order among the names is not the id's among the ids."""
    return 'n' + x[::-1]


class Device:
    """One context and one tokenizer: the tokenizer's dictionary grows from
    block to block, a subject's feature is its index, and the tables are
    extended by the names a block brings, as `_sync_shown` does.  ``named``:
    the shown text is `shown_name` of the id and the ids are sent next to
    it."""

    def __init__(self, named):
        from woltka_amd import _native as nat
        self.nat = nat
        self.named = named
        self.ctx = nat.Context(0)
        self.tok = nat.Tokenizer(2)
        self.ctx.counts_reserve(1 << 18)
        self.ctx.dtok_format('map')
        self.subjects = []
        self.shown = 0

    def jobs(self, uniq=False):
        nat = self.nat
        return [nat.Job(nat.MODE_NONE, 0, nat.F_UNIQ if uniq else 0, 0, 0.0)]

    @staticmethod
    def _table(names):
        enc = [x.encode() for x in names]
        off = np.zeros(len(enc) + 1, dtype=np.uint32)
        np.cumsum([len(x) for x in enc], out=off[1:])
        return np.frombuffer(b''.join(enc), dtype=np.uint8), off

    def tables(self, names, first, ids=True):
        self.ctx.readmap_reads_tables(first, *self._table(
            [shown_name(x) for x in names] if self.named else names))
        if self.named and ids:
            self.ctx.readmap_lists_ids(first, *self._table(names))

    def namedic(self):
        return {x: shown_name(x) for x in self.subjects} if self.named \
            else None

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
            self.tables(self.subjects[self.shown:], self.shown)
            self.shown = len(self.subjects)
        status, n_reads, _ = ctx.dtok_stage_reads_plain()
        assert status == 0
        ctx.set_uniform_group(0)
        return n_reads

    def maps(self):
        self.ctx.classify_staged_keep(self.jobs())
        return self.ctx.dtok_readmap_lists(0)[0].tobytes()

    def close(self):
        self.tok.close()
        self.ctx.close()


@pytest.fixture(scope='module')
def dev():
    d = Device(False)
    yield d
    d.close()


@pytest.fixture(scope='module')
def named():
    d = Device(True)
    yield d
    d.close()


def _model(reads, namedic=None):
    return b''.join(T.model_line(q, T.model_value(s, 'none', None), namedic)
                    for q, s in reads)


@pytest.mark.parametrize('name', list(T.block_cases()))
def test_blocks_of_lists_around_the_tiles_of_the_scan(dev, name):
    n = T.block_cases()[name]
    want = GOLD['blocks'][name]
    assert dev.stage(T.block_text(n)) == n
    got = dev.maps()
    have = T.digest(got)
    print(name, have['bytes'], have['lines'], have['sha256'])
    T.compare(got, want, name, model=lambda: T.block_map_text(n))
    assert got == T.block_map_text(n)


@pytest.mark.parametrize('n', (1, 256, 257))
def test_blocks_with_no_list_or_only_the_last_read_a_list(dev, n):
    assert dev.stage(T.block_text(n, 'nobody')) == n
    got = dev.maps()
    assert got == T.block_map_text(n, 'nobody') and b':' not in got
    # (without a list the two entry points agree)
    assert dev.ctx.dtok_readmap_reads(0)[0].tobytes() == got
    assert dev.stage(T.block_text(n, 'last')) == n
    got = dev.maps()
    assert got == T.block_map_text(n, 'last')
    assert got.count(b':1\n') == 1 and got.endswith(b':1\n')


def test_lists_are_ordered_by_the_ids_and_show_the_names(named):
    n = 600
    assert named.stage(T.block_text(n)) == n
    got = named.maps()
    want = T.block_map_text(n, shown=named.namedic())
    assert got == want, T.R.first_difference(got, want)
    by_name = b''.join(
        (q + '\t' + '\t'.join(f'{x}:1' for x in sorted(
            shown_name(s) for s in subs)) + '\n').encode()
        for q, subs in T.block_reads(n))
    assert got != by_name            # (the case can tell the two orders apart)


def test_the_tables_grow_between_two_blocks(named):
    """The first block's text, fetched before the tables are extended by the
    second block's subjects, stays what it was; the second block lists the new
    subjects among the old; set anew, the tables give the same text again."""
    tag = f'grow{len(named.subjects)}'
    one = [(f'q{i}', [f'{tag}a{i % 7}', f'{tag}a{(i + 3) % 7}'])
           for i in range(300)]
    two = [(f'p{i}', [f'{tag}b{i % 5}', f'{tag}a{i % 7}', f'{tag}B{i % 2}'])
           for i in range(300)]
    assert named.stage(T.map_text(one)) == 300
    first = named.maps()
    kept = bytes(first)
    before = named.shown
    assert named.stage(T.map_text(two)) == 300
    second = named.maps()
    assert named.shown == before + 7
    assert first == kept == _model(one, named.namedic())
    assert second == _model(two, named.namedic())
    named.tables(named.subjects, 0)
    assert named.ctx.dtok_readmap_lists(0)[0].tobytes() == second


def test_an_id_table_of_another_size_is_refused(named):
    tag = f'size{len(named.subjects)}'
    reads = [(f'q{i}', [f'{tag}{i % 3}', f'{tag}{(i + 1) % 3}'])
             for i in range(10)]
    assert named.stage(T.map_text(reads), extend=False) == 10
    named.tables(named.subjects[named.shown:], named.shown, ids=False)
    named.ctx.classify_staged_keep(named.jobs())
    with pytest.raises(RuntimeError, match='id table holds'):
        named.ctx.dtok_readmap_lists(0)
    named.ctx.readmap_lists_ids(named.shown, *named._table(
        named.subjects[named.shown:]))
    named.shown = len(named.subjects)
    assert named.ctx.dtok_readmap_lists(0)[0].tobytes() == \
        _model(reads, named.namedic())


def test_a_list_with_a_feature_outside_the_table_is_refused(dev):
    """A block whose subjects the table does not cover yet gives no text
    (WK_E_STATE); extended, it does."""
    tag = f'late{len(dev.subjects)}'
    reads = [(f'q{i}', [f'{tag}{i % 3}', 'S00']) for i in range(10)]
    assert dev.stage(T.map_text(reads), extend=False) == 10
    dev.ctx.classify_staged_keep(dev.jobs())
    with pytest.raises(RuntimeError, match='cannot print'):
        dev.ctx.dtok_readmap_lists(0)
    dev.tables(dev.subjects[dev.shown:], dev.shown)
    dev.shown = len(dev.subjects)
    assert dev.ctx.dtok_readmap_lists(0)[0].tobytes() == _model(reads)


def test_readmap_reads_still_refuses_a_list_code(dev):
    reads = T.block_reads(300)
    assert dev.stage(T.block_text(300)) == 300
    assert dev.maps() == _model(reads)
    with pytest.raises(RuntimeError, match='no single feature'):
        dev.ctx.dtok_readmap_reads(0)
    # ... and takes the same chunk once no job of the set returns a list
    dev.ctx.classify_staged_keep(dev.jobs(uniq=True))
    assert dev.ctx.dtok_readmap_reads(0)[0].tobytes() == b'' == \
        dev.ctx.dtok_readmap_lists(0)[0].tobytes()
