"""The host's two read-map formatters against the reference's own text, no GPU:
`file.write_readmap` and the native route of routes/readmaps.py
(`_multi_lists` + `_native.format_readmap` = `wk_format_readmap`, fed by the
host tokenizer's query descriptors) on the `ties`, `digits`, `names` and
`mates` cases of tests/readmap_cases.py, compared with
tests/golden/vectors/readmap_device.json -- what the reference's
`workflow.workflow(..., outmap_dir=...)` wrote for them
(tests/golden/make_readmap_reference.py).  tests/test_gpu_readmap.py pins the
device writer (csrc/wk_readmap.hpp) to the same fixture: the three formatters
are held to the reference, not only to each other."""
import io
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import readmap_cases as T               # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('readmap_device.json')
CASES = {c['name']: c for c in T.cli_cases()}
GENUS = T.genus_of()


def _case(name):
    """(alignment text, format, name dictionary or None, {rank: gold text})."""
    case = CASES[name]
    (rel,) = [k for k in case['files'] if k.startswith('aln/')]
    gold = GOLD['cli'][name]['maps']
    return (case['files'][rel], case['kwargs']['input_fmt'],
            T.names_of() if case['kwargs'].get('name_as_id') else None,
            {'none': gold['none/S.txt'], 'genus': gold['genus/S.txt']})


def test_the_cases_hold_the_shapes_they_promise():
    T.check_inputs()
    T.check_gold(GOLD)
    assert set(GOLD['cli']) == set(CASES)
    assert set(GOLD['blocks']) == set(T.block_cases())
    for name in T.DOOR_CASES:
        assert all(isinstance(v, str) for v in GOLD['cli'][name]['maps'].values())


@pytest.mark.parametrize('name', T.DOOR_CASES)
def test_the_plain_model_writes_the_reference_text(name):
    """`reads_of` / `map_line` (what the GPU tests build the device's tables
    from) say what the reference says."""
    text, fmt, namedic, gold = _case(name)
    reads = T.reads_of(text, fmt)
    for rank, tax in (('none', None), ('genus', GENUS)):
        got = ''.join(T.map_line(q, s, tax, namedic) + '\n' for q, s in reads)
        T.compare(got.encode(), gold[rank], f'{name} {rank}')


def test_the_plain_model_has_the_digests_of_the_large_texts():
    """Where the fixture holds a digest only -- `blocks`, the single blocks --
    the plain model rebuilds the reference's text: that is what a mismatch on
    the device is told against, line by line."""
    for name in ('blocks', 'blocks-small-slot'):
        want = GOLD['cli'][name]['maps']
        got = T.model_maps(CASES[name])
        assert sorted(got) == sorted(want) and len(got) == 3
        for k, text in got.items():
            assert isinstance(want[k], dict)
            T.compare(text, want[k], f'{name} {k}')
    for name, n in T.block_cases().items():
        T.compare(T.block_map_text(n), GOLD['blocks'][name], name)


@pytest.mark.parametrize('name', T.DOOR_CASES)
def test_python_writer_matches_the_reference(name):
    from woltka_amd.file import write_readmap
    text, fmt, namedic, gold = _case(name)
    reads = T.reads_of(text, fmt)
    rng = random.Random(5)
    for rank, tax in (('none', None), ('genus', GENUS)):
        taxque = []
        for _, subs in reads:
            taxa = [tax[s] if tax else s for s in subs]
            rng.shuffle(taxa)       # (a list(set): any order)
            taxque.append(taxa[0] if len(set(taxa)) == 1 else taxa)
        fh = io.StringIO()
        write_readmap(fh, [q for q, _ in reads], taxque, namedic)
        T.compare(fh.getvalue().encode(), gold[rank], f'{name} {rank}')


@pytest.mark.parametrize('name', T.DOOR_CASES)
def test_native_formatter_matches_the_reference(name):
    """The host tokenizer's reads through `ReadMaps._format_maps_native`, on a
    stand-in for the engine that holds the case's hierarchy: features are the
    subjects in the tokenizer's order, then the genus taxa."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.readmaps import ReadMaps
    text, fmt, namedic, gold = _case(name)
    tok = nat.Tokenizer(2)
    try:
        res = tok.parse(text, first=True, final=True, want_names=True, fmt=fmt)
        subjects = tok.new_subjects()
        queries = nat.Tokenizer.query_names(text, res['qname'])
    finally:
        tok.close()
    reads = T.reads_of(text, fmt)
    assert queries == [q for q, _ in reads]
    subj, qoff = res['subj'], res['off']
    taxa = sorted(set(GENUS[s] for s in subjects), reverse=True)
    names = list(subjects) + taxa
    anc = np.full(len(names), -1, dtype=np.int32)
    for i, s in enumerate(subjects):
        anc[i] = names.index(GENUS[s])

    class Stub(ReadMaps):
        index = SimpleNamespace(names=names,
                                names_of=lambda ids: [names[i] for i in ids])
        hier = SimpleNamespace(n_nodes=len(names))
        modes = [nat.MODE_NONE, nat.MODE_RANK]
        slots = [0, 0]
        ranks = ['none', 'genus']
        jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0),
                nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)]

        def _rank_table(self, slot):
            return anc

    assign = np.empty((2, len(reads)), dtype=np.int32)
    for r in range(len(reads)):
        ids = sorted(set(subj[qoff[r]:qoff[r + 1]].tolist()))
        assert [subjects[i] for i in ids] == \
            sorted(reads[r][1], key=subjects.index)
        assign[0, r] = ids[0] if len(ids) == 1 else nat.ASSIGN_MULTI
        tx = {int(anc[i]) for i in ids}
        assign[1, r] = tx.pop() if len(tx) == 1 else nat.ASSIGN_MULTI
    out = Stub()._format_maps_native(
        assign, subj, qoff, (text, res['qname']), 'S',
        {'none': 'none', 'genus': 'genus'}, None, namedic)
    assert [p for p, _, _ in out] == ['none/S.txt', 'genus/S.txt']
    for (_, got, _), rank in zip(out, ('none', 'genus')):
        T.compare(bytes(got), gold[rank], f'{name} {rank}')
