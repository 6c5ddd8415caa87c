"""Plain classification with `--stratify` on the device text route
(csrc/wk_strata_reads.hpp), the parts that need no GPU: when the route is
chosen (`classify.strata_reads_on_device`), and the commands of
tests/strata_plain_cases.py reproduced without a device -- the host
tokenizer's join (what takes every block and every map the device leaves
alone), the assigners and exact counters of oracle/woltka_oracle.py, the
package's own rounding and table writer -- against
tests/golden/vectors/strata_plain_device.json
(tests/golden/make_strata_plain_reference.py), so that the fixture is pinned
before any device run.  tests/test_gpu_strata_plain.py runs the same commands
through the device."""
import contextlib
import gzip
import io
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import strata_plain_cases as P          # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('strata_plain_device.json')
CASES = {c['name']: c for c in P.cases()}


def test_the_route_is_chosen_for_plain_stratification_only(monkeypatch):
    from woltka_amd import _native as nat
    from woltka_amd.classify import strata_reads_on_device as on_device
    for switch in ('WOLTKA_NO_DSTRATA', 'WOLTKA_NO_DTOK'):
        monkeypatch.delenv(switch, raising=False)
    for fmt in ('sam', 'b6o', 'paf', 'map'):
        for n_jobs in range(1, nat.MAX_JOBS + 1):
            assert on_device(fmt, n_jobs=n_jobs) is True
    # every flag that keeps today's route, alone and together
    flags = ('demux', 'coords', 'sizes', 'outmap', 'outcov', 'replay')
    for values in itertools.product((False, True), repeat=len(flags)):
        for strata, own_text, part in itertools.product(
                (True, False), (True, False), (None, (0, 2))):
            want = strata and own_text and part is None and not any(values)
            assert on_device('sam', strata=strata, own_text=own_text,
                             part=part, n_jobs=3,
                             **dict(zip(flags, values))) is want
    assert not on_device('sam', n_jobs=nat.MAX_JOBS + 1)
    assert not on_device('sam', n_jobs=0)
    for fmt in ('b6', 'cent', 'unknown', None):
        assert not on_device(fmt)
    for switch in ('WOLTKA_NO_DSTRATA', 'WOLTKA_NO_DTOK'):
        monkeypatch.setenv(switch, '1')
        assert not on_device('sam')
        monkeypatch.delenv(switch)
    assert on_device('sam')


def test_the_cases_hold_the_shapes_they_promise():
    P.check_inputs()
    assert sorted(GOLD) == sorted(CASES)
    want = {'fmt-sam', 'fmt-b6o', 'fmt-paf', 'fmt-map', 'sam-none',
            'sam-genus', 'sam-free', 'sam-mixed', 'sam-uniq', 'sam-major',
            'trimsub', 'exclude', 'mates', 'strangers', 'two-maps', 'gz',
            'blocks', 'mixed-routes', 'no-pairs'}
    assert want <= set(CASES)
    assert set(CASES) - want == {f'handoff-{n}' for n in P.T.handoff_maps()}
    for name, case in CASES.items():
        got = GOLD[name]
        assert set(got) == ({'error'} if case['route'] == 'error'
                            else {'tables'})
        if 'tables' in got:
            ranks = case['kwargs']['ranks'].split(',')
            assert sorted(got['tables']) == (
                ['out'] if len(ranks) == 1
                else sorted(f'{r}.tsv' for r in ranks))
    # the reference agrees about what the cases are made for: the same reads
    # in three formats; a sample whose reads the map does not hold keeps its
    # column; the stratum is in front of the feature
    assert GOLD['fmt-b6o'] == GOLD['fmt-paf'] == GOLD['fmt-map'] != \
        GOLD['fmt-sam']
    head, *rows = GOLD['strangers']['tables']['genus.tsv'].splitlines()
    assert head.split('\t')[1:] == ['S1', 'S2']
    assert rows and all(r.split('\t')[2] in ('0', '0.0') for r in rows)
    assert all(r.split('|')[0] in P.T.LABELS5 for r in rows)
    assert GOLD['sam-mixed']['tables']['genus.tsv'] == \
        GOLD['sam-genus']['tables']['out']
    assert GOLD['sam-mixed']['tables']['none.tsv'] == \
        GOLD['sam-none']['tables']['out']
    assert GOLD['sam-mixed']['tables']['free.tsv'] == \
        GOLD['sam-free']['tables']['out']


def _hierarchy(args):
    """(tree, rankdic) as dicts: nodes.dmp, then the subjects of the map."""
    tree, rankdic = {}, {}
    for fp in args['nodes_fps']:
        with open(fp) as f:
            for line in f:
                x = [y.strip() for y in line.split('|')]
                tree[x[0]], rankdic[x[0]] = x[1], x[2]
    for fp in args['map_fps']:
        with open(fp) as f:
            for line in f:
                if line.strip():
                    sub, taxon = line.split()
                    tree[sub] = taxon
    return tree, rankdic


def _sample_reads(path, fmt, strata_fp, exclude, trimsub):
    """[(stratum or None, subjects)] of one alignment file through the host
    tokenizer and its join."""
    from woltka_amd import _native as nat
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        text = f.read()
    tok = nat.Tokenizer(2, exclude)
    try:
        with open(strata_fp, 'rb') as f:
            labels = tok.load_strata(f)
        if not labels:
            raise ValueError('No stratification information is found in '
                             f'file: {os.path.basename(strata_fp)}.')
        res = tok.parse(text, first=True, final=True, fmt=fmt,
                        want_groups=True)
        assert res['consumed'] == len(text)
        names = tok.new_subjects()
    finally:
        tok.close()
    if trimsub:
        names = [x.rsplit(trimsub, 1)[0] for x in names]
    off, subj = res['off'].tolist(), res['subj'].tolist()
    return [(labels[g] if g >= 0 else None,
             list(dict.fromkeys(names[s] for s in subj[off[i]:off[i + 1]])))
            for i, g in enumerate(res['group'].tolist())]


def _reproduce(case, root):
    import woltka_oracle as O
    from woltka_amd.workflow import round_profiles, write_profiles
    args = P.write_case(case, root)
    tree, rankdic = _hierarchy(args)
    root_node = next(k for k, v in tree.items() if k == v)
    exclude = set(args['exclude'].split(',')) if args.get('exclude') else None
    ranks = args['ranks'].split(',')
    data = {r: {} for r in ranks}
    try:
        for sample in ('S1', 'S2'):
            fn = next(f for f in sorted(os.listdir(args['input_fp']))
                      if f.startswith(sample + '.'))
            reads = _sample_reads(
                os.path.join(args['input_fp'], fn), args['input_fmt'],
                os.path.join(args['strata_dir'], f'{sample}.txt'), exclude,
                args.get('trimsub'))
            strata = {i: s for i, (s, _) in enumerate(reads) if s is not None}
            for rank in ranks:
                _, counts = O.classify_chunk(
                    list(range(len(reads))), [subs for _, subs in reads],
                    rank, tree, rankdic, root_node,
                    uniq=bool(args.get('uniq')),
                    major=args['major'] / 100 if args.get('major') else None,
                    strata=strata)
                data[rank][sample] = {
                    k: (v.numerator / v.denominator) if v.denominator != 1
                    else v.numerator for k, v in counts.items()}
    except ValueError as e:
        return {'error': [type(e).__name__, str(e)]}
    out = os.path.join(root, 'out')
    with contextlib.redirect_stdout(io.StringIO()):
        round_profiles(data, None)
        write_profiles(data, out, False, ['S1', 'S2'])
    return {'tables': P.tables_of(out)}


@pytest.mark.parametrize('name', list(CASES))
def test_the_fixture_is_what_the_host_join_and_the_oracle_make(tmp_path,
                                                               name):
    assert _reproduce(CASES[name], str(tmp_path)) == GOLD[name]
