"""`woltka classify --sizes` on the calls that end in the general evaluator's
contribution log, which the device reduces (csrc/wk_logred.hpp): byte for
byte what the reference wrote -- the cases of tests/logred_cases.py
(tests/golden/vectors/logred_device.json, made by
tests/golden/make_logred_reference.py), the `--sizes` cases of
cli_random.json outside the words route, those of cli_coords.json and the
bundled RPK table -- each through the reduction (ROUTES['log_reduce'])."""
import contextlib
import io
import os
from os.path import join

import pytest

import logred_cases as LC
from helpers import DATA, load_vectors

pytestmark = pytest.mark.gpu

GOLD = load_vectors('logred_device.json')
CASES = {c['name']: c for c in LC.cases()}


def _classify(case, tmp_path, monkeypatch, no_dlog=False, digits=None):
    """Run the case; returns (result as `logred_cases.run_case` gives it, the
    routes taken)."""
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    if no_dlog:
        monkeypatch.setenv('WOLTKA_NO_DLOG', '1')
    else:
        monkeypatch.delenv('WOLTKA_NO_DLOG', raising=False)
    case = dict(case, kwargs=dict(case['kwargs']))
    if digits is not None:
        case['kwargs']['digits'] = digits
    ROUTES.clear()
    os.makedirs(tmp_path, exist_ok=True)
    res = LC.run_case(workflow, case, str(tmp_path))
    return res, dict(ROUTES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture_case(tmp_path, monkeypatch, name):
    assert set(GOLD) == set(CASES)
    res, routes = _classify(CASES[name], tmp_path, monkeypatch)
    assert res == GOLD[name]
    assert routes.get('log_reduce', 0) > 0, routes
    if name == 'nine-ranks':    # two batches of jobs for every chunk
        assert routes['log_reduce'] >= 2
    if name == 'unsized':
        assert 'error' in res


@pytest.mark.parametrize('name', ['free', 'uniq', 'nine-ranks'])
def test_both_routes_write_the_same_bytes(tmp_path, monkeypatch, name):
    """`--digits 10`: the floats of the two routes, not their roundings."""
    a, ra = _classify(CASES[name], tmp_path / 'a', monkeypatch, digits=10)
    b, rb = _classify(CASES[name], tmp_path / 'b', monkeypatch, digits=10,
                      no_dlog=True)
    assert 'tables' in a and a == b
    assert ra.get('log_reduce', 0) > 0 and rb.get('log_reduce', 0) == 0


def _random_cases():
    """The `--sizes` cases of cli_random.json that `test_gpu_sizes` leaves out:
    those outside the words route."""
    from test_gpu_sizes import _random_cases as within
    taken = set(within())
    return [i for i, c in enumerate(load_vectors('cli_random.json'))
            if c['kwargs'].get('sizes') and i not in taken]


def _coords_cases():
    return [i for i, c in enumerate(load_vectors('cli_coords.json'))
            if c['kwargs'].get('sizes')]


def test_the_selections_are_not_empty():
    picked = [load_vectors('cli_random.json')[i]['kwargs'] for i in _random_cases()]
    assert picked
    assert any('free' in (kw.get('ranks') or '') for kw in picked)
    for option in ('major', 'above', 'uniq', 'demux'):
        assert any(kw.get(option) for kw in picked), option
    assert any(load_vectors('cli_random.json')[i]['want_maps'] for i in _random_cases())
    assert len(_coords_cases()) == 3


def _run_vector(tmp_path, monkeypatch, case):
    """As test_gpu_cli_random.test_random_cli_case runs a case; returns the
    routes taken."""
    from test_gpu_cli_random import write_case_file
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    monkeypatch.delenv('WOLTKA_NO_DLOG', raising=False)
    for rel, text in case['files'].items():
        write_case_file(tmp_path / rel, text)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return join(DATA, 'taxonomy', v[5:])
        if isinstance(v, str) and v.startswith('$FUN/'):
            return join(DATA, 'function', v[5:])
        if isinstance(v, str) and (v in case['files'] or v == 'aln'):
            return str(tmp_path / v)
        return v
    args = {k: real(v) for k, v in case['kwargs'].items()}
    args['output_fp'] = str(tmp_path / 'out')
    if case['want_maps']:
        args['outmap_dir'] = str(tmp_path / 'maps')
    if case.get('want_cov'):
        args['outcov_dir'] = str(tmp_path / 'cov')
    args['no_exe'] = True
    expect = case['expect']
    ROUTES.clear()
    if 'error' in expect:
        with pytest.raises(Exception) as err, \
                contextlib.redirect_stdout(io.StringIO()):
            workflow(**args)
        assert type(err.value).__name__ == expect['error'][0]
        assert str(err.value) == expect['error'][1]
        return None
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**args)
    if len(expect['tables']) == 1 and 'out' in expect['tables']:
        got = {'out': (tmp_path / 'out').read_text()}
    else:
        got = {fn: (tmp_path / 'out' / fn).read_text()
               for fn in sorted(os.listdir(tmp_path / 'out'))}
    assert got == expect['tables']
    return dict(ROUTES)


@pytest.mark.parametrize('i', _random_cases())
def test_reference_written_random_case(tmp_path, monkeypatch, i):
    """(The one error case is refused before a file is read -- its sample list
    names a file that is not there --, so it has no route to assert.)"""
    case = load_vectors('cli_random.json')[i]
    routes = _run_vector(tmp_path, monkeypatch, case)
    if routes is None:
        assert case['expect']['error'][1] == \
            'Provided sample IDs and actual files are inconsistent.'
    else:
        assert routes.get('log_reduce', 0) > 0, routes


@pytest.mark.parametrize('i', _coords_cases())
def test_reference_written_coords_case(tmp_path, monkeypatch, i):
    routes = _run_vector(tmp_path, monkeypatch, load_vectors('cli_coords.json')[i])
    assert routes.get('log_reduce', 0) > 0, routes


def test_bt2sho_component_rpk_gene_lengths(tmp_path, monkeypatch):
    """The reference's own RPK recipe (golden bt2sho.component.rpk.tsv)."""
    import filecmp
    from click.testing import CliRunner
    from woltka_amd.cli import classify_cmd
    from woltka_amd.hostio import ROUTES
    monkeypatch.delenv('WOLTKA_NO_DLOG', raising=False)
    fun = join(DATA, 'function')
    out = str(tmp_path / 'output.tsv')
    ROUTES.clear()
    res = CliRunner().invoke(classify_cmd, [
        '--input', join(DATA, 'align', 'bt2sho'), '--rank', 'component',
        '--coords', join(fun, 'coords.txt.xz'),
        '--map', join(fun, 'uniref', 'uniref.map.xz'),
        '--map', join(fun, 'go', 'component.tsv.xz'),
        '--sizes', '.', '--scale', '1k', '--digits', '3',
        '--output', out, '--no-exe'])
    assert res.exit_code == 0, res.output + repr(res.exception)
    assert filecmp.cmp(out, join(DATA, 'output', 'bt2sho.component.rpk.tsv'),
                       shallow=False)
    assert ROUTES['log_reduce'] > 0, dict(ROUTES)
