"""Coord-match under demultiplexing on the device text route, the parts that
need no GPU: when the route is chosen (`classify.demux_hits_on_device`), what
the fixture tests/golden/vectors/demux_coords_device.json (made by
tests/golden/make_demux_coords_reference.py from the reference) promises, and
the commands of tests/demux_coords_cases.py through oracle/woltka_oracle.py --
its parsers, its matcher, its demultiplexer and its counters -- so that the
fixture stands on two legs before any device run."""
import contextlib
import io
import itertools
import lzma
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import demux_coords_cases as T          # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('demux_coords_device.json')
CLI_CASES = {c['name']: c for c in T.cli_cases()}


def test_the_route_is_chosen_for_coord_match_demultiplexing(monkeypatch):
    from woltka_amd import _native as nat
    from woltka_amd.classify import demux_hits_on_device as on_device
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    monkeypatch.delenv('WOLTKA_NO_DTOK', raising=False)
    for fmt in ('sam', 'b6o', 'paf'):
        for n_jobs in range(1, nat.MAX_JOBS + 1):
            assert on_device(True, fmt, n_jobs=n_jobs)
            assert on_device(True, fmt, sizes=True, n_jobs=n_jobs)
    # every flag that keeps today's route, alone and together; `--sizes`
    # does not
    for native, sizes, exclude, replay in itertools.product((True, False),
                                                            repeat=4):
        want = native and not exclude and not replay
        assert on_device(native, 'sam', sizes=sizes, exclude=exclude,
                         n_jobs=3, replay=replay) is want
    assert not on_device(True, 'sam', n_jobs=nat.MAX_JOBS + 1)
    assert not on_device(True, 'sam', n_jobs=0)
    for fmt in ('map', 'b6', 'cent', 'unknown', None):  # (a simple map has no "ex" flavour)
        assert not on_device(True, fmt)
    for switch in ('WOLTKA_NO_DDEMUX', 'WOLTKA_NO_DTOK'):
        monkeypatch.setenv(switch, '1')
        assert not on_device(True, 'sam')
        monkeypatch.delenv(switch)
    assert on_device(True, 'sam')


def test_the_plain_route_s_predicate_stays_as_it_is():
    from woltka_amd.classify import demux_on_device
    assert demux_on_device(True, 'sam') is True
    assert demux_on_device(True, 'sam', coords=True) is False


def test_the_cases_hold_the_shapes_they_promise():
    reads = {c['name']: GOLD['reads'][c['name']] for c in T.read_cases()}
    cases = {c['name']: c for c in T.read_cases()}
    for case in cases.values():
        assert 50 <= case['text'].count('\n') <= 700
    flat, pair = reads['sam-unpaired'], reads['sam-paired']
    for name, got in (('sam-unpaired', flat), ('sam-paired', pair)):
        samples = {x[0] for x in got}
        assert {'', 'S1', 'S10', 'S1x', 'ninebytes', T.LONG} <= samples
        # met only in hits of length 0, on the genome without genes, below
        # the threshold, in unmapped lines: none of the reference's samples
        assert not samples & set(T.GENELESS)
        ids = {x.split('\t', 1)[0].split('_')[0]
               for x in cases[name]['text'].splitlines()[1:]}
        assert set(T.GENELESS) <= ids       # ... though the text holds them
        assert all(x[1] for x in got)
    # an id that ends in its first '_': '' unpaired, its left part as a mate
    assert not any(x[0].startswith(('Q', 'T')) for x in flat)
    assert any(x[0].startswith('Q') for x in pair)
    assert 'S3' in {x[0] for x in pair}     # both mates and an unpaired line in one run
    assert ['S1', ['GA_1']] in flat         # two hits on one gene
    assert {x[0] for x in reads['sam-whitelist']} == {None, 'S1', 'ninebytes'}
    assert reads['b6o'] == reads['paf']
    assert len({x[0] for x in reads['nine-samples']}) == 9
    cli = GOLD['cli']
    with open(os.path.join(ROOT, 'tests', 'golden', 'data', 'output',
                           'bowtie2.orf.tsv')) as f:
        assert cli['orf']['tables']['out'] == T.digest({'out': f.read()})['out']
    assert cli['orf']['classified'] == [8001]
    assert cli['nine']['tables'] == cli['cigar']['tables']


# ---- the commands through the oracle ------------------------------------------
def _coords(fp):
    """{genome: [(gene id, start0, end)]} of a coordinates file."""
    import woltka_oracle as O
    opener = lzma.open if fp.endswith('.xz') else open
    out, cur = {}, None
    with opener(fp, 'rt') as f:
        for line in f:
            line = line.rstrip()
            if line.startswith('>'):
                cur = out.setdefault(line[1:], [])
            elif line:
                gid, beg, end = line.split('\t')
                cur.append((gid,) + O.normalize_gene(int(beg), int(end)))
    return {g: sorted(rows, key=lambda r: (r[1], r[2]))
            for g, rows in out.items()}


def _records(text, fmt):
    """[(query, [(subject, length, start0, end)])] as the "ex" parsers yield
    them."""
    import woltka_oracle as O
    if fmt == 'sam':
        return [(q, [(s, n, b, e) for s, _, n, b, e in hits])
                for q, hits in O.parse_sam_lines(text.splitlines(),
                                                 extra=True)]
    out = []
    for line in text.splitlines():      # (align.parse_b6o_file_ex, align.py:941-975)
        x = line.split('\t')
        beg, end = sorted((int(x[8]), int(x[9])))
        if not out or out[-1][0] != x[0]:
            out.append((x[0], []))
        out[-1][1].append((x[1], int(x[3]), beg - 1, end))
    return out


def _first_column_map(fp):
    opener = lzma.open if fp.endswith('.xz') else open
    out = {}
    with opener(fp, 'rt') as f:
        for line in f:
            x = line.rstrip().split('\t')
            if len(x) > 1:
                out.setdefault(x[0], x[1])
    return out


def _reproduce(case, root):
    import woltka_oracle as O
    from woltka_amd.workflow import (round_profiles, scale_profiles,
                                     write_profiles)
    args = T.write_cli(case, root)
    kw = case['kwargs']
    coords = _coords(args['coords_fp'])
    records = _records(T.text_of(case['text']), case['fmt'])
    queries, genes = O.ordinal_chunk(records, coords,
                                     kw.get('overlap', 80) / 100, prefix=True)
    allow = None
    if 'samples' in args:
        with open(args['samples']) as f:
            allow = f.read().split()
    ranks = kw.get('ranks', 'none').split(',')
    tree, rankdic, namedic = None, None, None
    if 'map_fps' in args:       # (`--map-as-rank`: a file's targets are of its rank)
        tree, rankdic = {}, {}
        for fp in args['map_fps']:
            rank = os.path.basename(fp).split('.')[0]
            for k, v in _first_column_map(fp).items():
                tree[k] = v
                rankdic[v] = rank
        # (tree.fill_root, tree.py:302-388: the nodes without a parent hang
        # under a root of their own)
        for top in {v for v in tree.values() if v not in tree}:
            tree[top] = '1'
        tree['1'] = '1'
        namedic = {}
        for fp in args['names_fps']:
            namedic.update(_first_column_map(fp))
    sizes = None
    if kw.get('sizes') == '.':
        sizes = {f'{g}_{gid}': 1 / (e - s) for g, rows in coords.items()
                 for gid, s, e in rows}
    data = {r: {} for r in ranks}
    for sample, (qs, subque) in O.demultiplex(queries, genes, allow).items():
        subque = [tuple(s) for s in subque]
        for rank in ranks:
            taxque, counts = O.classify_chunk(qs, subque, rank, tree, rankdic,
                                              '1' if tree else None)
            if sizes is not None:
                counts = O.count_sized(subque, taxque, sizes)
            data[rank][sample] = {
                k: (v.numerator / v.denominator) if getattr(
                    v, 'denominator', 1) != 1 else
                (v.numerator if hasattr(v, 'numerator') else v)
                for k, v in counts.items()}
    out = os.path.join(root, 'out')
    with contextlib.redirect_stdout(io.StringIO()):
        scale_profiles(data, kw.get('scale'))
        round_profiles(data, kw.get('digits'))
        write_profiles(data, out, False, allow, tree, rankdic, namedic)
    return {'tables': T.digest(T.tables_of(out)), 'classified': [len(queries)]}


@pytest.mark.parametrize('name', list(CLI_CASES))
def test_the_fixture_is_what_the_oracle_makes(tmp_path, name):
    assert _reproduce(CLI_CASES[name], str(tmp_path)) == GOLD['cli'][name]
