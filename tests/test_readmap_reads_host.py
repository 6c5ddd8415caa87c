"""The read maps of whole-read assignments without a GPU: which calls the
device route takes (`Engine.read_maps_on_device`, routes/words.py), and the
host formatter -- what every case writes when the route is off
(``WOLTKA_NO_DREADMAPS=1``: the native route of routes/readmaps.py,
`_format_maps_native` = `wk_format_readmap`, fed by the host tokenizer's query
descriptors) -- on the cases of tests/readmap_reads_cases.py, compared with
tests/golden/vectors/readmap_reads_device.json: what the reference's
`workflow.workflow(..., outmap_dir=...)` wrote for them
(tests/golden/make_readmap_reads_reference.py).  The assignment codes come
from the plain model of the assigners in the case module, so the fixture is
reachable before any kernel runs; tests/test_gpu_readmap_reads.py pins the
device writer (csrc/wk_readmap_reads.hpp) to the same fixture."""
import gzip
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_reads_cases as T         # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('readmap_reads_device.json')
CASES = {c['name']: c for c in T.cli_cases()}


def test_the_cases_hold_the_shapes_they_promise():
    T.check_inputs()
    T.check_gold(GOLD)
    assert set(GOLD['cli']) == {c['gold'] for c in CASES.values()}
    assert set(GOLD['blocks']) == set(T.block_cases())


def test_the_plain_model_has_the_digests_of_the_blocks():
    for name, n in T.block_cases().items():
        T.compare(T.block_map_text(n), GOLD['blocks'][name], name)


# ---- the gate -----------------------------------------------------------------------
def _engine(ranks, uniq=False, above=False, major=0, subok=False,
            sizes=None, replay=None, n_extra=0):
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
    e._tok_identity, e.use_tree = True, True
    return e


TAKEN = [dict(ranks='none', uniq=True), dict(ranks='free'),
         dict(ranks='free', subok=True), dict(ranks='genus', uniq=True),
         dict(ranks='genus', above=True), dict(ranks='genus', major=80),
         dict(ranks='free,phylum,genus', uniq=True),
         dict(ranks='none,free,genus', uniq=True),
         dict(ranks='free', n_extra=7)]
# a job that can return a list, alone or next to whole-read jobs
LISTS = [dict(ranks='none'), dict(ranks='genus'), dict(ranks='none,genus'),
         dict(ranks='none,free'), dict(ranks='free,genus'),
         dict(ranks='none,genus', above=True),
         dict(ranks='none,genus', major=80)]


@pytest.mark.parametrize('kw', TAKEN)
def test_gate_takes_the_sets_of_the_scope(kw, monkeypatch):
    for var in ('WOLTKA_NO_DREADMAPS', 'WOLTKA_NO_DTOK'):
        monkeypatch.delenv(var, raising=False)
    e = _engine(**kw)
    for fmt in ('sam', 'b6o', 'paf', 'map'):
        assert e.read_maps_on_device(fmt)
    assert not e.device_maps_eligible()
    # everything the scope leaves out
    for out in (dict(demux=True), dict(strata=True), dict(coords=True),
                dict(outcov=True), dict(part=(0, 2)), dict(own_text=False)):
        assert not e.read_maps_on_device('sam', **out), out
    assert not e.read_maps_on_device('bam')
    assert not e.read_maps_on_device(None)
    assert not _engine(sizes={'a': 1}, **kw).read_maps_on_device('sam')
    assert not _engine(replay={}, **kw).read_maps_on_device('sam')
    more = dict(kw, n_extra=kw.get('n_extra', 0) + 8)
    assert not _engine(**more).read_maps_on_device('sam')
    monkeypatch.setenv('WOLTKA_NO_DREADMAPS', '1')
    assert not e.read_maps_on_device('sam')
    monkeypatch.delenv('WOLTKA_NO_DREADMAPS')
    monkeypatch.setenv('WOLTKA_NO_DTOK', '1')
    assert not e.read_maps_on_device('sam')


@pytest.mark.parametrize('kw', LISTS)
def test_gate_leaves_sets_that_can_return_a_list(kw, monkeypatch):
    for var in ('WOLTKA_NO_DREADMAPS', 'WOLTKA_NO_DTOK', 'WOLTKA_NO_WORDS',
                'WOLTKA_NO_DMAPS'):
        monkeypatch.delenv(var, raising=False)
    e = _engine(**kw)
    assert not e.read_maps_on_device('sam')
    # sets of plain jobs only still choose `dtok_maps`
    plain_only = not (kw.get('above') or kw.get('major') or
                      'free' in kw['ranks'])
    assert e.device_maps_eligible() == plain_only


def test_every_case_of_the_fixture_is_in_scope(monkeypatch):
    for var in ('WOLTKA_NO_DREADMAPS', 'WOLTKA_NO_DTOK'):
        monkeypatch.delenv(var, raising=False)
    for case in CASES.values():
        kw = case['kwargs']
        e = _engine(kw['ranks'], uniq=kw.get('uniq', False),
                    above=kw.get('above', False), major=kw.get('major', 0),
                    subok=kw.get('subok', False))
        assert e.read_maps_on_device(kw['input_fmt'] or 'b6o'), case['name']


# ---- the host formatter -------------------------------------------------------------
def _host_maps(case):
    """{relative path: bytes} of the case's map files: the host tokenizer's
    reads, the model's codes, `_format_maps_native`."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.readmaps import ReadMaps
    kw = case['kwargs']
    hier = T.hierarchy_of(case)
    ranks = T.map_ranks(case)
    opts = dict(uniq=kw.get('uniq', False), above=kw.get('above', False),
                major=kw.get('major'), subok=kw.get('subok', False))
    namedic = T._pairs(case['files']['names.txt']) \
        if kw.get('name_as_id') else None
    exclude = kw['exclude'].split(',') if kw.get('exclude') else None
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
        names, ids = [], {}

        def feature(x):
            if x not in ids:
                ids[x] = len(names)
                names.append(x)
            return ids[x]
        assign = np.empty((len(ranks), qoff.size - 1), dtype=np.int32)
        for r in range(qoff.size - 1):
            subs = [subjects[i] for i in subj[qoff[r]:qoff[r + 1]].tolist()]
            for j, rank in enumerate(ranks):
                v = T.assign(subs, rank, hier, **opts)
                assign[j, r] = nat.ASSIGN_NONE if v is None else feature(v)

        class Stub(ReadMaps):
            index = SimpleNamespace(
                names=names, names_of=lambda ids_: [names[i] for i in ids_])
            hier = SimpleNamespace(n_nodes=len(names))
            modes = [nat.MODE_NONE] * len(ranks)    # (no list: no rank table is asked for)
            slots = [0] * len(ranks)
            jobs = [nat.Job(nat.MODE_NONE, 0, nat.F_UNASSIGNED
                            if kw.get('unassigned') else 0, 0, 0.0)]
        stub = Stub()
        stub.ranks = ranks
        texts = stub._format_maps_native(
            assign, np.zeros(subj.size, dtype=np.int32), qoff,
            (data, res['qname']), sample,
            {rank: (rank if len(ranks) > 1 else '') for rank in ranks}, None,
            namedic)
        for path, text, _ in texts:
            out[path.lstrip('/')] = bytes(text)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_host_formatter_writes_the_reference_maps(name):
    want = GOLD['cli'][CASES[name]['gold']]['maps']
    got = _host_maps(CASES[name])
    assert sorted(got) == sorted(want)
    for k, text in sorted(got.items()):
        T.compare(text, want[k], f'{name} {k}')
