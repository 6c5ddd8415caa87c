"""`woltka classify` on random small inputs with random option sets: 56 cases
made by tests/golden/make_golden.gen_cli_random — input files, keyword
arguments of workflow.workflow (= the CLI options) and what the reference
wrote (table text per rank, decompressed read maps) or raised.  The GPU path
must write the same bytes / raise the same error.  18 more cases
(gen_cli_coords) go through `--coords`: reads placed over / next to genes of
the bundled coordinates, three formats, overlap 50 / 80 / 100, gene-length
normalisation (`--sizes .`) and gene -> function maps; 16 with `--outmap` and
small chunks, 20 more of those with hits of aligned length 0 (which count
towards the reference's chunk boundaries and nothing else, ordinal.py:222,231)."""
import contextlib
import gzip
import io
import os
from os.path import join

import pytest

from helpers import DATA, load_vectors

pytestmark = pytest.mark.gpu

_BIG = 'big_' if os.environ.get('WOLTKA_BIG_SWEEP') else ''    # one-off sweeps
CASES = load_vectors(_BIG + 'cli_random.json') + \
    load_vectors(_BIG + 'cli_coords.json') + \
    ([] if _BIG else load_vectors('cli_coords_excl.json')) + \
    ([] if _BIG else load_vectors('cli_coords_maps.json')) + \
    ([] if _BIG else load_vectors('cli_coords_zero.json'))
TAX = join(DATA, 'taxonomy')
FUN = join(DATA, 'function')


def write_case_file(path, text):
    """A fixture's input file; the extension picks the compression."""
    import bz2
    import lzma
    path.parent.mkdir(parents=True, exist_ok=True)
    opener = {'.gz': gzip.open, '.bz2': bz2.open, '.xz': lzma.open}.get(
        path.suffix, open)
    with opener(path, 'wt') as f:
        f.write(text)


def _label(i):
    kw = CASES[i]['kwargs']
    bits = [os.path.splitext(kw['input_fp'])[1].lstrip('.') or 'dir',
            kw.get('ranks', 'map' if kw.get('map_rank') else 'ogu')]
    bits += [k for k in ('coords_fp', 'overlap', 'demux', 'uniq', 'major', 'above', 'subok',
                         'unassigned', 'exclude', 'trimsub', 'sizes', 'frac',
                         'scale', 'digits', 'chunk') if k in kw]
    return f'{i}-' + '-'.join(map(str, bits))


def route_factors(case):
    """The case's options as factor levels of tests/cli_routes_cases.py (what
    its `expected_route` reads): a single-file input is demultiplexed, bzip2
    and xz are both text the package does not read block by block, and a job
    set is known by its kinds of jobs -- plain ones (`none`, a rank),
    whole-read ones (`free`, a rank under --uniq / --above / --major above 50), `none`
    under --uniq."""
    kw = case['kwargs']
    files = [f for f in case['files']
             if f.startswith('aln/') or f.startswith('mux.')]
    root, zext = os.path.splitext(files[0])
    if zext not in ('.gz', '.bz2', '.xz'):
        root, zext = files[0], ''
    fmt = {'b6': 'b6o'}.get(root.rsplit('.', 1)[1], root.rsplit('.', 1)[1])
    if kw['input_fp'] == 'aln' and not kw.get('demux'):
        layout = 'dir-samples' if kw.get('samples') else 'dir'
    else:
        layout = 'mux-list' if kw.get('samples') else 'mux'
    ranks = (kw.get('ranks') or ('rank' if kw.get('map_rank') else 'none')
             ).split(',')
    tree = any(kw.get(k) for k in ('nodes_fps', 'lineage_fps', 'columns_fps',
                                   'newick_fps', 'map_fps'))
    kinds = set()
    for r in ranks:
        if r == 'none' or not tree:
            kinds.add('none-uniq' if kw.get('uniq') else 'plain')
        elif r == 'free' or kw.get('uniq') or kw.get('above') or \
                (kw.get('major') or 0) > 50:
            kinds.add('whole')
        else:
            assert not kw.get('major')      # (<= 50: no level stands for it)
            kinds.add('plain')
    jobs = 'none-uniq' if 'none-uniq' in kinds else \
        'mixed' if kinds == {'plain', 'whole'} else \
        'whole' if kinds == {'whole'} else \
        'three' if len(ranks) > 1 else 'one' if ranks != ['none'] else 'none'
    return dict(
        fmt=fmt, input=layout, zip=zext if zext in ('', '.gz') else '.bz2',
        system='coords' if kw.get('coords_fp') else 'plain', jobs=jobs,
        outmap=bool(case['want_maps']), outcov=bool(case.get('want_cov')),
        stratify=bool(kw.get('strata_dir')), sizes=bool(kw.get('sizes')),
        trimsub=bool(kw.get('trimsub')), exclude=bool(kw.get('exclude')),
        unassigned=bool(kw.get('unassigned')),
        name_as_id=bool(kw.get('name_as_id')), blocks='one')


def expects_device_text(case, args):
    """Must this reference case be tokenised on the device?  The table of
    DESIGN.md section 3 as tests/cli_routes_cases.py holds it
    (`expected_route`, `expected_also`): the ROUTES keys of which one must
    have counted and those that must have counted next to it, or None."""
    import cli_routes_cases
    if not any(f.startswith('aln/') or f.startswith('mux.')
               for f in case['files']) or 'error' in case['expect']:
        return None
    factors = route_factors(case)
    want = cli_routes_cases.expected_route(factors)
    if want is None:
        return None
    return tuple(sorted(want)), tuple(sorted(
        cli_routes_cases.expected_also(factors)))


@pytest.mark.parametrize('i', range(len(CASES)), ids=_label)
def test_random_cli_case(tmp_path, i):
    from woltka_amd.workflow import workflow
    from woltka_amd.classify import ROUTES
    case = CASES[i]
    routes_before = dict(ROUTES)
    for rel, text in case['files'].items():
        write_case_file(tmp_path / rel, text)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return join(TAX, v[5:])
        if isinstance(v, str) and v.startswith('$FUN/'):
            return join(FUN, v[5:])
        if isinstance(v, str) and (v in case['files'] or v == 'aln'):
            return str(tmp_path / v)
        return v
    args = {k: real(v) for k, v in case['kwargs'].items()}
    args['output_fp'] = str(tmp_path / 'out')
    if case['want_maps']:
        args['outmap_dir'] = str(tmp_path / 'maps')
    if case.get('want_cov'):
        args['outcov_dir'] = str(tmp_path / 'cov')
    args['no_exe'] = i % 2 == 0     # built-in codecs / external decompressors
    expect = case['expect']
    if 'error' in expect:
        with pytest.raises(Exception) as err, \
                contextlib.redirect_stdout(io.StringIO()):
            workflow(**args)
        assert type(err.value).__name__ == expect['error'][0]
        assert str(err.value) == expect['error'][1]
        return
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**args)
    if len(expect['tables']) == 1 and 'out' in expect['tables']:
        got = {'out': (tmp_path / 'out').read_text()}
    else:
        got = {fn: (tmp_path / 'out' / fn).read_text()
               for fn in sorted(os.listdir(tmp_path / 'out'))}
    assert got == expect['tables']
    # the route: an uncompressed SAM / BLAST / PAF / map case
    # within the stated limits went through the tokenizer on the device
    want = expects_device_text(case, args)
    took = {k: ROUTES[k] - routes_before.get(k, 0) for k in ROUTES
            if ROUTES[k] != routes_before.get(k, 0)}
    if want is not None and any(x.strip() for f, x in case['files'].items()
                                if f.startswith('aln/') or
                                f.startswith('mux.')):
        assert any(took.get(k) for k in want[0]), (want, took)
        for k in want[1]:
            assert took.get(k), (want, took)
    if case['want_maps']:
        maps = {}
        for root, _, fns in os.walk(args['outmap_dir']):
            for fn in fns:
                rel = os.path.relpath(join(root, fn), args['outmap_dir'])
                with gzip.open(join(root, fn), 'rt') as f:
                    maps[rel] = f.read()
        # (also under --coords --trim-sub, where genes share a trimmed id: the
        # gene lists then carry the genes themselves, wk_ordinal_pair_genes)
        assert maps == expect['maps']
    if case.get('want_cov'):
        got_cov = {fn: open(join(args['outcov_dir'], fn)).read()
                   for fn in sorted(os.listdir(args['outcov_dir']))}
        assert got_cov == expect['cov']


STRATA = load_vectors(_BIG + 'cli_strata.json')


@pytest.mark.parametrize('i', range(len(STRATA)))
def test_random_two_pass_stratified(tmp_path, i):
    """Pass 1 writes read maps at a rank (gz / bz2 / plain), pass 2 is
    stratified by them: both tables as the reference wrote them."""
    from woltka_amd.workflow import workflow
    case = STRATA[i]
    for rel, text in case['files'].items():
        write_case_file(tmp_path / rel, text)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return join(TAX, v[5:])
        if isinstance(v, str) and (v in case['files'] or v == 'aln'):
            return str(tmp_path / v)
        return v
    a1 = {k: real(v) for k, v in case['pass1'].items()}
    a1.update(output_fp=str(tmp_path / 'out1'),
              outmap_dir=str(tmp_path / 'maps'), no_exe=True)
    a2 = {k: real(v) for k, v in case['pass2'].items()}
    a2.update(output_fp=str(tmp_path / 'out2'),
              strata_dir=str(tmp_path / 'maps'), no_exe=True)
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**a1)
        workflow(**a2)
    assert (tmp_path / 'out1').read_text() == case['expect']['table1']
    assert (tmp_path / 'out2').read_text() == case['expect']['table2']


def _medium():
    import sys
    sys.path.insert(0, join(os.path.dirname(__file__), 'golden'))
    import make_golden
    return make_golden


@pytest.mark.parametrize('case', range(4))
def test_medium_size_runs(tmp_path, case):
    """Runs of 1-1.5 M records (multi-block tokenising on all threads, cache
    overflow and miss-log paths on the device) against the reference's tables;
    the input text is regenerated from the case's seed by the same generator
    that fed the reference (tests/golden/make_golden.medium_input)."""
    from woltka_amd.workflow import workflow
    mg = _medium()
    name, seed, fmt, nq, kw = mg.MEDIUM[case]
    gold = load_vectors('cli_medium.json')[name]
    with open(join(TAX, 'taxid.map')) as f:
        genomes = [x.split('\t')[0] for x in f]
    text = mg.medium_input(seed, fmt, nq, genomes)
    assert text.count('\n') == gold['records']
    fp = tmp_path / f'S1.{fmt}'
    fp.write_text(text)
    args = {k: ([join(TAX, x[5:]) for x in v] if isinstance(v, list) else v)
            for k, v in kw.items()}
    args.update(input_fp=str(fp), input_fmt=fmt, output_fmt=False,
                output_fp=str(tmp_path / 'out'))
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**args)
    if len(gold['tables']) == 1 and 'out' in gold['tables']:
        got = {'out': (tmp_path / 'out').read_text()}
    else:
        got = {fn: (tmp_path / 'out' / fn).read_text()
               for fn in sorted(os.listdir(tmp_path / 'out'))}
    assert got == gold['tables']
