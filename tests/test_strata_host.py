"""The strata join of `--stratify` on hand-written maps, the parts that need no
GPU: the host tokenizer's join (`Tokenizer.load_strata` + `parse(...,
want_groups=True)`, csrc/wk_tokenize.cpp -- what takes every map the device
leaves alone) and the package's Python reader against
tests/golden/vectors/strata_device.json, which holds what the reference's
`workflow.read_strata` makes of the maps of tests/strata_cases.py
(tests/golden/make_strata_reference.py).  tests/test_gpu_strata.py pins the
device's join (csrc/wk_strata.hpp) to the same fixture."""
import io
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import strata_cases as T                # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('strata_device.json')
MAPS = T.map_cases()


def gold_map(name):
    return T.gold_map(GOLD, name)


def test_the_cases_hold_the_shapes_they_promise():
    T.check_inputs()
    assert set(GOLD['maps']) == set(MAPS)
    assert set(GOLD['cli']) == {c['name'] for c in T.cli_cases()}
    # the reference agrees about what the cases are made for
    assert GOLD['maps']['crlf'] == GOLD['maps']['crlf-as-lf']
    assert 'GONE' in GOLD['maps']['last-wins-near']['labels'] and \
        'GONE' not in GOLD['maps']['last-wins-near']['strata'].values()
    assert len(GOLD['maps']['hot-keys']['strata']) == 3 and \
        len(GOLD['maps']['hot-keys']['labels']) == 4
    assert GOLD['maps']['strip']['labels'].count('') == 1
    assert GOLD['maps']['open-end-pair']['strata']['last'] == 'END'
    assert 'last' not in GOLD['maps']['open-end-nonpair']['strata']
    for name in T.NO_LABELS:
        assert GOLD['maps'][name]['strata'][0] == 'ValueError'
        assert GOLD['maps'][name]['labels'] == []
    for name in ('columns', 'crlf'):
        assert not any('BAD' in x for x in GOLD['maps'][name]['labels'])
        assert not any('bad' in k for k in GOLD['maps'][name]['strata'])


@pytest.mark.parametrize('name', list(MAPS))
def test_python_reader_reads_the_maps_like_the_reference(name):
    want, labels = gold_map(name)
    from woltka_amd.file import read_map_uniq
    fh = io.TextIOWrapper(io.BytesIO(MAPS[name]), encoding='utf-8')
    pairs = list(read_map_uniq(fh))
    assert dict(pairs) == want
    assert list(dict.fromkeys(v for _, v in pairs)) == labels


@pytest.mark.parametrize('name', list(MAPS))
def test_host_join_matches_the_reference(name):
    """One thread on the whole text, four threads on small blocks (of the map
    and of the reads)."""
    from woltka_amd import align
    from woltka_amd._native import Tokenizer
    want, labels = gold_map(name)
    plist = T.case_probes(name, MAPS[name])
    sam = T.probe_sam(plist)
    for threads, map_block, block in ((1, 1 << 27, 1 << 26), (4, 1000, 1500)):
        tok = Tokenizer(threads)
        try:
            got_labels = tok.load_strata(io.BytesIO(MAPS[name]), map_block)
            got = []
            for _, res in align.native_sam_blocks(io.BytesIO(sam), tok, block,
                                                  want_groups=True):
                got.extend(res['group'].tolist())
        finally:
            tok.close()
        assert got_labels == labels
        assert len(got) == len(plist)
        assert [got_labels[g] if g >= 0 else None for g in got] == \
            [want.get(T.probe_key(p)) for p in plist]
