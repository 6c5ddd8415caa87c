"""`woltka classify` with its options met two at a time over every device
route (tests/cli_routes_cases.py): per case the files are rebuilt from the
seed, `workflow.workflow` runs with the case's options -- many-blocks cases
with 8192-byte tokenizer blocks --, and tables, read maps and coverage are the
reference's byte for byte (tests/golden/vectors/cli_routes.json, made by
tests/golden/make_cli_routes_reference.py).  The route is asserted from the
ROUTES deltas: a key of `expected_route(case)` counted, no block went through
the host tokenizer, with 8192-byte blocks at least three blocks per file;
where the table of DESIGN.md section 3 names no device route, none counted."""
import pytest

import cli_routes_cases as T
from helpers import load_vectors

pytestmark = pytest.mark.gpu

CASES = T.cases()
GOLD = load_vectors('cli_routes.json')


@pytest.mark.parametrize('case', CASES, ids=T.label)
def test_cli_route_case(tmp_path, monkeypatch, case):
    from woltka_amd import classify
    from woltka_amd.workflow import workflow
    ROUTES = classify.ROUTES
    what = T.label(case)
    gold = GOLD[case['name']]
    if case['blocks'] == 'many':
        monkeypatch.setattr(classify.Engine, 'DTOK_BLOCK', T.BLOCK)
    before = dict(ROUTES)
    got = T.run_case(workflow, case, str(tmp_path))
    took = {k: ROUTES[k] - before.get(k, 0) for k in ROUTES
            if ROUTES[k] != before.get(k, 0)}
    assert got['inputs'] == gold['inputs'], what
    if 'error' in gold:
        assert got.get('error') == gold['error'], what
        return
    assert 'error' not in got, (what, got.get('error'))
    for part in ('tables', 'maps', 'cov'):
        assert sorted(got.get(part, {})) == sorted(gold.get(part, {})), \
            (what, part)
        for name, text in gold.get(part, {}).items():
            assert got[part][name] == text, (what, part, name, took)
    want = T.expected_route(case)
    if want is None:
        assert not any(took.get(k) for k in T.BLOCK_KEYS), (what, took)
        return
    assert any(took.get(k) for k in want), (what, want, took)
    for k in T.expected_also(case):
        assert took.get(k), (what, k, took)
    assert not took.get('host_block'), (what, took)
    if case['blocks'] == 'many':
        assert sum(took.get(k, 0) for k in want) >= 3 * T.n_files(case), \
            (what, want, took)
