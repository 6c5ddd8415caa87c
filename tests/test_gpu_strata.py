"""The strata join on the device (csrc/wk_strata.hpp: strata_parse_kernel,
strata_verify_kernel, strata_lookup in dtok_place_kernel<true>) through its
own door -- `Context.strata_load`, `strata_groups`, `strata_clear` -- and
through whole `--coords --stratify` commands, against
tests/golden/vectors/strata_device.json: what the reference makes of the
hand-written maps and the commands of tests/strata_cases.py
(tests/golden/make_strata_reference.py).  tests/test_strata_host.py pins the
host's join to the same fixture.

No door returns a read's group, so a read's stratum is read off the count
table: every probe read hits a genome of its own whose one gene has the
probe's index as its feature; after the coord-match a cell (group, feature)
says that probe `feature` was joined to label `group`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import strata_cases as T                # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('strata_device.json')
MAPS = T.map_cases()
KEPT = [n for n in T.kept_maps()]
HANDOFF = list(T.handoff_maps())
CLI_CASES = {c['name']: c for c in T.cli_cases()}
N_GENOMES = 6000            # more than the probes of any case


class Device:
    """One context and one tokenizer for the whole module: the strata buffers
    live in the context, and every case loads its map over the one before."""

    def __init__(self):
        from woltka_amd import _native as nat
        self.nat = nat
        self.ctx = nat.Context(0)
        self.tok = nat.Tokenizer(2)
        n = N_GENOMES
        # genome P%05d: one gene [1, 1000], feature = the genome's number
        self.ctx.set_genes(np.arange(n + 1), np.zeros(n, np.int32),
                           np.full(n, 1000, np.int32), np.arange(n))
        self.ctx.counts_reserve(1 << 16)
        self.ctx.dtok_format('sam')
        self.genome = []        # genome of the tokenizer's subjects
        self.jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)]

    def load(self, name):
        return self.ctx.strata_load(np.frombuffer(MAPS[name], dtype=np.uint8))

    def cells(self, plist):
        """{probe index: group} after one block of the probes' SAM lines."""
        ctx = self.ctx
        assert len(plist) <= N_GENOMES
        text = np.frombuffer(T.probe_sam(plist), dtype=np.uint8)
        ctx.counts_clear()
        status, n_lines = ctx.dtok_scan(self.tok, text, 0, text.size,
                                        extra=True)
        assert status == 0 and n_lines == len(plist)
        self.genome.extend(int(x[1:]) for x in self.tok.new_subjects())
        st, reads, hits = ctx.dtok_stage_hits(
            np.asarray(self.genome, dtype=np.int32), 0.8)
        assert st == 0 and hits == len(plist) and 0 < reads <= hits
        ctx.ordinal_count(self.jobs)
        keys, vals = ctx.counts_fetch()
        # (job, group, feature) -> Fraction: a whole read is 1, whether the
        # table holds it as k = 1 or in units of 1 / WEIGHT_L
        cells = self.nat.counts_to_fractions(keys, vals)
        assert all(v == 1 and j == 0 for (j, _, _), v in cells.items())
        got = {f: g for _, g, f in cells}
        assert len(got) == len(cells)       # one cell per probe
        return got

    def join(self, plist, labels, slots):
        """[label or None] per probe through the map that is loaded."""
        self.ctx.strata_groups(slots, np.arange(len(labels), dtype=np.int32))
        got = self.cells(plist)
        assert all(0 <= g < len(labels) for g in got.values())
        return [labels[got[i]] if i in got else None
                for i in range(len(plist))]

    def close(self):
        self.tok.close()
        self.ctx.close()


@pytest.fixture(scope='module')
def dev():
    d = Device()
    yield d
    d.close()


def _want(name, plist):
    want, _ = T.gold_map(GOLD, name)
    return [want.get(T.probe_key(p)) for p in plist]


def _check_join(dev, name, labels, slots):
    plist = T.case_probes(name, MAPS[name])
    want = _want(name, plist)
    got = dev.join(plist, [x.decode() for x in labels], slots)
    assert got == want
    assert sum(x is not None for x in got) == \
        sum(x is not None for x in want)


# ---- a. load -------------------------------------------------------------------
@pytest.mark.parametrize('name', KEPT)
def test_load_gives_the_labels_in_the_reference_order(dev, name):
    got = dev.load(name)
    assert got is not None
    labels, slots = got
    assert [x.decode() for x in labels] == T.gold_map(GOLD, name)[1]
    assert len(set(slots.tolist())) == len(labels) == slots.size
    assert all(0 <= s < 1 << 17 for s in slots.tolist())
    if name in T.NO_LABELS:
        assert labels == []


def test_crlf_labels_are_those_of_the_same_map_with_lf(dev):
    a, b = dev.load('crlf'), dev.load('crlf-as-lf')
    assert a is not None and b is not None and a[0] == b[0]


@pytest.mark.parametrize('name', HANDOFF)
def test_maps_the_device_leaves_to_the_host(dev, name):
    assert dev.load('clean') is not None
    assert dev.load(name) is None
    with pytest.raises(RuntimeError, match='no strata map on the device'):
        dev.ctx.strata_groups(np.zeros(1, np.int32), np.zeros(1, np.int32))


# ---- b. join, per read ---------------------------------------------------------
@pytest.mark.parametrize('name', KEPT)
def test_join_gives_every_read_the_reference_label(dev, name):
    labels, slots = dev.load(name)
    _check_join(dev, name, labels, slots)
    # the same block without a map: every probe has its cell (so that "no
    # cell" above is the join's doing)
    dev.ctx.strata_clear()
    dev.ctx.set_uniform_group(0)
    plist = T.case_probes(name, MAPS[name])
    assert dev.cells(plist) == {i: 0 for i in range(len(plist))}


# ---- c. reload -----------------------------------------------------------------
def test_a_smaller_map_over_a_larger_one(dev):
    labels, slots = dev.load('labels-65536')
    big = T.case_probes('labels-65536', MAPS['labels-65536'])[:200]
    want = _want('labels-65536', big)
    assert 40 < sum(x is not None for x in want) < 160
    assert dev.join(big, [x.decode() for x in labels], slots) == want
    labels, slots = dev.load('clean')
    # keys of the first map are gone, its label slots carry no group (`join`
    # asserts that every group is one of the five)
    assert dev.join(big, [x.decode() for x in labels], slots) == \
        [None] * len(big)
    _check_join(dev, 'clean', labels, slots)
    dev.ctx.strata_clear()
    assert dev.load('tail-1c') is None
    labels2, slots2 = dev.load('clean')
    assert labels2 == labels and slots2.tolist() == slots.tolist()
    _check_join(dev, 'clean', labels2, slots2)


# ---- d. the command --------------------------------------------------------------
@pytest.mark.parametrize('name', list(CLI_CASES))
def test_commands_match_the_reference(tmp_path, monkeypatch, name):
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    case = CLI_CASES[name]
    monkeypatch.delenv('WOLTKA_NO_DTOK', raising=False)
    if case['route'] == 'mixed':
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 13)
    ROUTES.clear()
    got = T.run_cli(workflow, case, str(tmp_path))
    routes = dict(ROUTES)
    assert got == GOLD['cli'][name]
    if case['route'] == 'device':
        assert routes.get('dstrata', 0) == 2 and \
            routes.get('dhits_strata', 0) > 0 and \
            not routes.get('host_block'), routes
    elif case['route'] == 'host':
        assert not routes.get('dstrata'), routes
    elif case['route'] == 'mixed':
        assert routes.get('dstrata', 0) > 0 and \
            routes.get('dhits_strata', 0) > 0 and \
            routes.get('host_block', 0) > 0, routes
    else:
        assert 'error' in got
