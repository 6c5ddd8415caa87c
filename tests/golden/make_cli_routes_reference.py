#!/usr/bin/env python3
"""tests/golden/vectors/cli_routes.json: what the REAL reference makes of the
cases of tests/cli_routes_cases.py (build container only; the inputs are
regenerated from their seeds).

    python tests/golden/make_cli_routes_reference.py

Per case (by name): 'inputs' -- the sha256 of every generated input file, so
that a drift of the generator shows as a fixture mismatch --, and 'tables',
'maps', 'cov' -- the text of every file `workflow.workflow` wrote (read maps
decompressed; maps and coverage above `cli_routes_cases.VERBATIM` bytes as
`digest`: sha256, bytes, lines) -- or 'error': the exception's type and
message where the reference raised.

As in make_readmap_reference.py everything is made under two values of
PYTHONHASHSEED and nothing is written when the two differ."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cli_routes_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'cli_routes.json')
HASH_SEEDS = ('11', '4242')
MAX_BYTES = 2_500_000


def emit(only=None):
    from woltka.workflow import workflow
    doc = {}
    for case in T.cases():
        if only and case['name'] not in only:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            doc[case['name']] = T.run_case(workflow, case, tmp)
    return doc


def main():
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    if sys.argv[1:2] == ['emit']:
        json.dump(emit(sys.argv[2:]), sys.stdout)
        return
    docs = []
    for seed in HASH_SEEDS:
        env = dict(os.environ, PYTHONHASHSEED=seed)
        docs.append(json.loads(subprocess.check_output(
            [sys.executable, os.path.abspath(__file__), 'emit'], env=env)))
    if docs[0] != docs[1]:
        differ = [k for k in docs[0] if docs[0][k] != docs[1][k]]
        sys.exit(f'results that depend on the hash seed: {differ}')
    for case in T.cases():
        got = docs[0][case['name']]
        print(T.label(case), got.get('error') or
              {k: len(got[k]) for k in ('tables', 'maps', 'cov') if k in got})
    text = json.dumps(docs[0], separators=(',', ':'), sort_keys=True) + '\n'
    if len(text) > MAX_BYTES:
        sys.exit(f'the fixture would be {len(text)} bytes')
    with open(OUT, 'w') as fh:
        fh.write(text)
    errors = sum('error' in v for v in docs[0].values())
    print(f'{len(docs[0])} cases, {errors} errors, {len(text)} bytes')


if __name__ == '__main__':
    main()
