"""The read maps under demultiplexing without a GPU: which calls the device
route takes (`Engine.demux_read_maps_on_device`, routes/words.py) next to the
gates that were there before it, and the host route -- what the cases write
when the route is off (``WOLTKA_NO_DDEMUXMAPS=1``: the host tokenizer's reads
as strings, `workflow.demux_labels`, the Python writer `_write_maps` of
routes/readmaps.py) -- on the cases of tests/readmap_demux_cases.py, compared
with tests/golden/vectors/readmap_demux_device.json: what the reference's
`workflow.workflow(..., outmap_dir=...)` wrote for them
(tests/golden/make_readmap_demux_reference.py).  The assignment codes come
from the plain model of the assigners in tests/readmap_reads_cases.py (the
sets in which no job returns a list), so the fixture is reachable before any
kernel runs; tests/test_gpu_readmap_demux.py pins the device route
(csrc/wk_readmap_demux.hpp) to the same fixture, every case of it."""
import gzip
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_demux_cases as T         # noqa: E402
import readmap_reads_cases as RR        # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('readmap_demux_device.json')
CASES = {c['name']: c for c in T.cli_cases()}
SWITCHES = ('WOLTKA_NO_DDEMUXMAPS', 'WOLTKA_NO_DDEMUX', 'WOLTKA_NO_DTOK',
            'WOLTKA_NO_DREADMAPS', 'WOLTKA_NO_DLISTMAPS')


def test_the_cases_hold_the_shapes_they_promise():
    T.check_inputs()
    T.check_gold(GOLD)
    assert set(GOLD['cli']) == {c['gold'] for c in CASES.values()}


def test_the_partition_model_is_a_stable_partition():
    """The model the device's partition is held to, on a case small enough
    to say by hand."""
    samp = np.asarray([2, 0, -1, 2, 0, 7], dtype=np.int32)
    length = np.asarray([5, 3, 9, 0, 4, 1], dtype=np.uint64)
    off, seg, total = T.partition_model(samp, length)
    assert off.tolist() == [7, 0, 0, 12, 3, 12] and total == 13
    assert seg.tolist() == [[0, 0, 7], [2, 7, 5], [7, 12, 1]]


# ---- the gates ----------------------------------------------------------------------
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


# 1 to 8 jobs of any kind
SETS = [dict(ranks='none', uniq=True), dict(ranks='genus', uniq=True),
        dict(ranks='free'), dict(ranks='genus', major=80), dict(ranks='none'),
        dict(ranks='genus'), dict(ranks='none,free,genus'),
        dict(ranks='genus', above=True), dict(ranks='free', subok=True),
        dict(ranks='free', n_extra=7)]


@pytest.mark.parametrize('kw', SETS)
def test_gate_takes_demultiplexed_files_with_read_maps(kw, monkeypatch):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    e = _engine(**kw)
    for fmt in ('sam', 'b6o', 'paf', 'map'):
        assert e.demux_read_maps_on_device(fmt)
    # the gates that were there say what they said: no read maps under demux
    assert not e.read_maps_on_device('sam', demux=True)
    assert not e.read_map_lists_on_device('sam', demux=True)
    # a file that is not demultiplexed is not this route's
    assert not e.demux_read_maps_on_device('sam', demux=False)
    for out in (dict(strata=True), dict(coords=True), dict(outcov=True),
                dict(part=(0, 2)), dict(own_text=False)):
        assert not e.demux_read_maps_on_device('sam', **out), out
    assert not e.demux_read_maps_on_device('bam')
    assert not e.demux_read_maps_on_device(None)
    assert not _engine(sizes={'a': 1}, **kw).demux_read_maps_on_device('sam')
    assert not _engine(replay={}, **kw).demux_read_maps_on_device('sam')
    more = dict(kw, n_extra=kw.get('n_extra', 0) + 8)
    assert not _engine(**more).demux_read_maps_on_device('sam')
    for var in ('WOLTKA_NO_DDEMUXMAPS', 'WOLTKA_NO_DDEMUX', 'WOLTKA_NO_DTOK'):
        monkeypatch.setenv(var, '1')
        assert not e.demux_read_maps_on_device('sam'), var
        monkeypatch.delenv(var)
    # (the switches of R1m and R1l are not this route's)
    monkeypatch.setenv('WOLTKA_NO_DREADMAPS', '1')
    monkeypatch.setenv('WOLTKA_NO_DLISTMAPS', '1')
    assert e.demux_read_maps_on_device('sam')


def test_the_old_demux_gates_still_say_no_outmap(monkeypatch):
    """`native_demux` -- what `workflow.classify` hands the gates of R1d and
    R2d -- is False with read maps, as before: the new route does not go
    through them."""
    from woltka_amd import classify as C
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    assert C.demux_on_device(True, 'sam') and \
        not C.demux_on_device(False, 'sam')
    assert C.demux_hits_on_device(True, 'sam') and \
        not C.demux_hits_on_device(False, 'sam')
    assert not C.cover_on_device('sam', demux=True)
    assert 'dreads_demux' in C.Engine.ROUTE_OF and \
        C.Engine.ROUTE_OF['ddemux'] == '_run_ddemux'


def test_every_case_of_the_fixture_is_in_scope(monkeypatch):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for case in CASES.values():
        kw = case['kwargs']
        e = _engine(kw['ranks'], uniq=kw.get('uniq', False),
                    major=kw.get('major', 0))
        assert e.demux_read_maps_on_device(kw['input_fmt']), case['name']


# ---- the host route -----------------------------------------------------------------
# the cases whose job sets return no list (the plain model gives their codes)
NO_LIST = ['none-uniq', 'genus-uniq', 'free', 'major', 'unassigned',
           'plain-text-uniq', 'one-sample', 'mates', 'b6o', 'gz', 'dir',
           'exclude', 'samples-middle', 'samples-none', 'late', 'handoff']


def _host_maps(case, root):
    """{relative path: bytes} of the case's map files: the host tokenizer's
    reads as strings, `demux_labels`, the model's codes, `_write_maps`."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.readmaps import ReadMaps
    from woltka_amd.workflow import demux_labels
    kw = case['kwargs']
    hier = RR.hierarchy_of(case)
    ranks = T.map_ranks(case)
    opts = dict(uniq=kw.get('uniq', False), major=kw.get('major'))
    exclude = kw['exclude'].split(',') if kw.get('exclude') else None
    allow = set(kw['samples'].split(',')) if kw.get('samples') else None
    rank2dir = {rank: os.path.join(root, rank if len(ranks) > 1 else '')
                for rank in ranks}
    for d in rank2dir.values():
        os.makedirs(d, exist_ok=True)
    for rel, data in sorted(case['files'].items()):
        if not rel.startswith('aln/'):
            continue
        fn = rel[4:]
        if fn.endswith('.gz'):
            data, fn = gzip.decompress(data), fn[:-3]
        fmt = kw['input_fmt'] or fn.rsplit('.', 1)[1]
        tok = nat.Tokenizer(2, exclude)
        try:
            res = tok.parse(data, first=True, final=True, want_names=True,
                            fmt=fmt)
            subjects = tok.new_subjects()
        finally:
            tok.close()
        subj, qoff = res['subj'], res['off']
        reads = nat.Tokenizer.query_names(data, res['qname'])
        sample_of, reads = demux_labels(reads, allow)
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
                v = RR.assign(subs, rank, hier, **opts)
                assign[j, r] = nat.ASSIGN_NONE if v is None else feature(v)

        class Stub(ReadMaps):
            index = SimpleNamespace(names=names)
            hier = SimpleNamespace(n_nodes=len(names))
            modes = [nat.MODE_NONE] * len(ranks)    # (no list: no rank table is asked for)
            slots = [0] * len(ranks)
            jobs = [nat.Job(nat.MODE_NONE, 0, nat.F_UNASSIGNED
                            if kw.get('unassigned') else 0, 0, 0.0)]
        stub = Stub()
        stub.ranks = ranks
        stub._write_maps(assign, subj, qoff, reads, sample_of, rank2dir,
                         None, None)
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            fp = os.path.join(dirpath, f)
            with open(fp, 'rb') as fh:
                out[os.path.relpath(fp, root)] = fh.read()
    return out


@pytest.mark.parametrize('name', NO_LIST)
def test_host_route_writes_the_reference_maps(name, tmp_path):
    want = GOLD['cli'][CASES[name]['gold']]['maps']
    got = _host_maps(CASES[name], str(tmp_path))
    assert sorted(got) == sorted(want)
    for k, text in sorted(got.items()):
        T.compare(text, want[k], f'{name} {k}')
