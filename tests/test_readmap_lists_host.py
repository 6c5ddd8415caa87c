"""The read maps with taxon lists without a GPU: which calls the device route
takes (`Engine.read_map_lists_on_device`, routes/words.py) next to the gates
that were there before it, and the host formatter -- what every case writes
when the route is off (``WOLTKA_NO_DLISTMAPS=1``: `_multi_lists` and
`_format_maps_native` of routes/readmaps.py, fed by the host tokenizer's
query descriptors) -- on the cases of tests/readmap_lists_cases.py, compared
with tests/golden/vectors/readmap_lists_device.json: what the reference's
`workflow.workflow(..., outmap_dir=...)` wrote for them
(tests/golden/make_readmap_lists_reference.py).  The assignment codes come
from the plain model in the case module; tests/test_gpu_readmap_lists.py pins
the device formatter (csrc/wk_readmap_lists.hpp) to the same fixture."""
import gzip
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_lists_cases as T         # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('readmap_lists_device.json')
CASES = {c['name']: c for c in T.cli_cases()}
NEAR = {c['name']: c for c in T.neighbour_cases()}
SWITCHES = ('WOLTKA_NO_DLISTMAPS', 'WOLTKA_NO_DREADMAPS', 'WOLTKA_NO_DTOK',
            'WOLTKA_NO_WORDS', 'WOLTKA_NO_DMAPS')


def test_the_cases_hold_the_shapes_they_promise():
    T.check_inputs()
    T.check_gold(GOLD)
    assert set(GOLD['cli']) == {c['gold'] for c in CASES.values()} | set(NEAR)
    assert set(GOLD['blocks']) == set(T.block_cases())


def test_the_plain_model_has_the_digests_of_the_blocks():
    for name, n in T.block_cases().items():
        T.compare(T.block_map_text(n), GOLD['blocks'][name], name)


# ---- the gates ----------------------------------------------------------------------
def _engine(ranks, uniq=False, above=False, major=0, subok=False,
            sizes=None, replay=None, n_extra=0, identity=True):
    """A stand-in for the engine that holds what the gates look at."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.words import WordsRoute
    flags = (nat.F_UNIQ if uniq else 0) | (nat.F_ABOVE if above else 0) | \
        (nat.F_SUBOK if subok else 0) | (nat.F_SIZED if sizes else 0)
    jobs = []
    for rank in ranks.split(',') + ['free'] * n_extra:
        mode = {'none': nat.MODE_NONE, 'free': nat.MODE_FREE}.get(
            rank, nat.MODE_RANK)
        jobs.append(nat.Job(mode, 0, flags, 0,
                            major / 100 if mode == nat.MODE_RANK else 0.0))

    class Stub(WordsRoute):
        pass
    e = Stub()
    e.jobs, e.sizes, e._replay = jobs, sizes, replay
    e._tok_identity, e.use_tree = identity, True
    return e


# a job that can return a list, alone or next to jobs of any kind
TAKEN = [dict(ranks='none'), dict(ranks='genus'), dict(ranks='none,genus'),
         dict(ranks='phylum,genus'), dict(ranks='none,free'),
         dict(ranks='free,genus'), dict(ranks='none,free,genus'),
         dict(ranks='none,free,genus', subok=True),
         # (above / major touch the ranks alone: none still returns lists)
         dict(ranks='none,genus', above=True),
         dict(ranks='none,genus', major=80),
         dict(ranks='genus', n_extra=7)]
# no job of the set returns a list
LEFT = [dict(ranks='none', uniq=True), dict(ranks='free'),
        dict(ranks='genus', uniq=True), dict(ranks='genus', above=True),
        dict(ranks='genus', major=80), dict(ranks='genus', major=30),
        dict(ranks='none,free,genus', uniq=True),
        dict(ranks='free,phylum,genus', above=True)]


@pytest.mark.parametrize('kw', TAKEN)
def test_gate_takes_the_sets_of_the_scope(kw, monkeypatch):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    e = _engine(**kw)
    for fmt in ('sam', 'b6o', 'paf', 'map'):
        assert e.read_map_lists_on_device(fmt)
    assert not e.read_maps_on_device('sam')
    # every option that turns it off
    for out in (dict(demux=True), dict(strata=True), dict(coords=True),
                dict(outcov=True), dict(part=(0, 2)), dict(own_text=False)):
        assert not e.read_map_lists_on_device('sam', **out), out
    assert not e.read_map_lists_on_device('bam')
    assert not e.read_map_lists_on_device(None)
    assert not _engine(sizes={'a': 1}, **kw).read_map_lists_on_device('sam')
    assert not _engine(replay={}, **kw).read_map_lists_on_device('sam')
    more = dict(kw, n_extra=kw.get('n_extra', 0) + 8)
    assert not _engine(**more).read_map_lists_on_device('sam')
    # (whether the tokenizer's ids are the subjects' is R1's question)
    assert _engine(identity=False, **kw).read_map_lists_on_device('sam')
    monkeypatch.setenv('WOLTKA_NO_DLISTMAPS', '1')
    assert not e.read_map_lists_on_device('sam')
    monkeypatch.delenv('WOLTKA_NO_DLISTMAPS')
    monkeypatch.setenv('WOLTKA_NO_DTOK', '1')
    assert not e.read_map_lists_on_device('sam')
    monkeypatch.delenv('WOLTKA_NO_DTOK')
    monkeypatch.setenv('WOLTKA_NO_DREADMAPS', '1')      # (R1m's switch is not this route's)
    assert e.read_map_lists_on_device('sam')


@pytest.mark.parametrize('kw', LEFT)
def test_gate_leaves_sets_without_a_list_job(kw, monkeypatch):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    e = _engine(**kw)
    assert not e.read_map_lists_on_device('sam')
    assert e.read_maps_on_device('sam')


def _old_gates(case):
    """(dmaps, dreadmaps) as `workflow.classify` has them for the case's
    first file before the new gate is asked: `device_maps_eligible` under the
    options that let it be asked -- and a route only without `--exclude`
    (`native_chunks`) --, `read_maps_on_device` where `dmaps` is off."""
    kw = case['kwargs']
    e = _engine(kw['ranks'], uniq=kw.get('uniq', False))
    fmt = kw['input_fmt'] or 'b6o'
    asked = not kw.get('trimsub')
    dmaps = asked and e.device_maps_eligible()
    dreadmaps = not dmaps and e.read_maps_on_device(fmt)
    return e, fmt, bool(dmaps and not kw.get('exclude')), dreadmaps, \
        e.device_maps_eligible()


@pytest.mark.parametrize('name', list(CASES))
def test_old_gates_leave_every_case_to_the_new_one(name, monkeypatch):
    """What the gates of before say on the fixture's commands is what they
    said before: plain-only sets are `device_maps_eligible` (and kept from
    R1 by `--trim-sub` or `--exclude`), no set is `read_maps_on_device`'s."""
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    case = CASES[name]
    e, fmt, dmaps, dreadmaps, eligible = _old_gates(case)
    plain_only = 'free' not in case['kwargs']['ranks']
    assert eligible == plain_only
    assert not e.read_maps_on_device(fmt)
    assert not dmaps and not dreadmaps
    assert e.read_map_lists_on_device(fmt)
    monkeypatch.setenv('WOLTKA_NO_DLISTMAPS', '1')
    assert not e.read_map_lists_on_device(fmt)
    assert _old_gates(case)[2:] == (dmaps, dreadmaps, eligible)


def test_old_gates_keep_the_neighbours(monkeypatch):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    _, _, dmaps, dreadmaps, _ = _old_gates(NEAR['plain-only'])
    assert dmaps and not dreadmaps
    e, fmt, dmaps, dreadmaps, _ = _old_gates(NEAR['none-genus-uniq'])
    assert not dmaps and dreadmaps and not e.read_map_lists_on_device(fmt)


# ---- the host formatter -------------------------------------------------------------
def _host_maps(case):
    """{relative path: bytes} of the case's map files: the host tokenizer's
    reads, the model's codes (a list: ASSIGN_MULTI), `_multi_lists` and
    `_format_maps_native` over a feature index of the tree's nodes followed by
    the subjects outside it."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.readmaps import ReadMaps
    kw = case['kwargs']
    hier = T.hierarchy_of(case)
    tree, rankdic = hier
    ranks = T.map_ranks(case)
    opts = dict(uniq=kw.get('uniq', False), above=kw.get('above', False),
                major=kw.get('major'), subok=kw.get('subok', False))
    namedic = T._pairs(case['files']['names.txt']) \
        if kw.get('name_as_id') else None
    exclude = kw['exclude'].split(',') if kw.get('exclude') else None
    names = list(dict.fromkeys(list(tree) + list(tree.values())))
    n_nodes = len(names)
    ids = {x: i for i, x in enumerate(names)}

    def feature(x):
        if x not in ids:
            ids[x] = len(names)
            names.append(x)
        return ids[x]

    def rank_table(rank):
        def find_rank(x):
            while x is not None and rankdic.get(x) != rank:
                x = tree.get(x)
            return x
        return np.asarray([ids.get(find_rank(x), -1) for x in names[:n_nodes]],
                          dtype=np.int32)
    tables = {j: rank_table(rank) for j, rank in enumerate(ranks)
              if rank not in ('none', 'free')}
    out = {}
    for rel, data in sorted(case['files'].items()):
        if not rel.startswith('aln/'):
            continue
        fn = rel[4:]
        if fn.endswith('.gz'):
            data, fn = gzip.decompress(data), fn[:-3]
        sample, ext = fn.rsplit('.', 1)
        fmt = kw['input_fmt'] or ext
        tok = nat.Tokenizer(2, exclude)
        try:
            res = tok.parse(data, first=True, final=True, want_names=True,
                            fmt=fmt)
            subjects = tok.new_subjects()
        finally:
            tok.close()
        if kw.get('trimsub'):
            subjects = [x.rsplit(kw['trimsub'], 1)[0] for x in subjects]
        subj, qoff = res['subj'], res['off']
        feats = np.asarray([feature(x) for x in subjects], dtype=np.int32)
        assign = np.empty((len(ranks), qoff.size - 1), dtype=np.int32)
        for r in range(qoff.size - 1):
            subs = [subjects[i] for i in subj[qoff[r]:qoff[r + 1]].tolist()]
            for j, rank in enumerate(ranks):
                v = T.model_value(subs, rank, hier, **opts)
                assign[j, r] = nat.ASSIGN_MULTI if isinstance(v, list) else \
                    nat.ASSIGN_NONE if v is None else feature(v)

        class Stub(ReadMaps):
            index = SimpleNamespace(
                names=names, names_of=lambda ids_: [names[i] for i in ids_])
            hier = SimpleNamespace(n_nodes=n_nodes)
            modes = [nat.MODE_NONE if rank == 'none' else nat.MODE_FREE
                     if rank == 'free' else nat.MODE_RANK for rank in ranks]
            slots = list(range(len(ranks)))
            jobs = [nat.Job(nat.MODE_NONE, 0, nat.F_UNASSIGNED
                            if kw.get('unassigned') else 0, 0, 0.0)]

            def _rank_table(self, slot):
                return tables[slot]
        stub = Stub()
        stub.ranks = ranks
        texts = stub._format_maps_native(
            assign, feats[subj], qoff, (data, res['qname']), sample,
            {rank: (rank if len(ranks) > 1 else '') for rank in ranks}, None,
            namedic)
        for path, text, _ in texts:
            out[path.lstrip('/')] = bytes(text)
    return out


@pytest.mark.parametrize('name', list(CASES) + list(NEAR))
def test_host_formatter_writes_the_reference_maps(name):
    case = CASES.get(name) or NEAR[name]
    want = GOLD['cli'][case['gold']]['maps']
    got = _host_maps(case)
    assert sorted(got) == sorted(want)
    for k, text in sorted(got.items()):
        T.compare(text, want[k], f'{name} {k}')
