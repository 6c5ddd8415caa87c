#!/usr/bin/env python3
"""tests/golden/vectors/strata_plain_device.json: what the REAL reference makes
of the plain `--stratify` commands of tests/strata_plain_cases.py (build
container only; the inputs are regenerated from their seeds).

    python tests/golden/make_strata_plain_reference.py

Per case of `cases`: the tables `workflow.workflow` writes, or its error.  What
a read's label is under every map of the cases is not recorded again: it
stands in tests/golden/vectors/strata_device.json
(tests/golden/make_strata_reference.py).

As in make_strata_reference.py everything is made under two values of
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

import strata_plain_cases as P  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'strata_plain_device.json')
HASH_SEEDS = ('11', '4242')


def emit():
    from woltka.workflow import workflow
    doc = {}
    for case in P.cases():
        with tempfile.TemporaryDirectory() as tmp:
            doc[case['name']] = P.run_case(workflow, case, tmp)
    return doc


def main():
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    if sys.argv[1:] == ['emit']:
        json.dump(emit(), sys.stdout)
        return
    P.check_inputs()
    docs = []
    for seed in HASH_SEEDS:
        env = dict(os.environ, PYTHONHASHSEED=seed)
        docs.append(json.loads(subprocess.check_output(
            [sys.executable, os.path.abspath(__file__), 'emit'], env=env)))
    if docs[0] != docs[1]:
        sys.exit('results that depend on the hash seed: %s' % [
            k for k in docs[0] if docs[0][k] != docs[1][k]])
    for k, v in docs[0].items():
        print(k, v.get('error') or {fn: len(t)
                                    for fn, t in v['tables'].items()})
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
