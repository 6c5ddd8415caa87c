#!/usr/bin/env python3
"""tests/golden/vectors/logred_device.json: what the REAL reference makes of
the `--sizes` cases of tests/logred_cases.py (build container only; the inputs
are regenerated from their seeds, only the expected table text / error of
every case is committed).

    python tests/golden/make_logred_reference.py

As in make_sizes_reference.py, a sum of the reference may depend on the
interpreter's hash seed: every case is run under two values of PYTHONHASHSEED,
and nothing is written when any table differs between them -- that case's
seed is changed (no case is dropped).

The fetch route of this package must reproduce every entry before the file is
committed: `python tests/golden/make_logred_reference.py check` runs it with
WOLTKA_NO_DLOG=1 (on a machine with a device, like every classify call; it
needs no reference tree)."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import logred_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'logred_device.json')
HASH_SEEDS = ('11', '4242')


def run_all(workflow):
    runs = {}
    for case in T.cases():
        with tempfile.TemporaryDirectory() as tmp:
            runs[case['name']] = T.run_case(workflow, case, tmp)
    return runs


def check_inputs():
    """What the cases promise about their inputs."""
    cases = T.cases()
    assert len({c['name'] for c in cases}) == len(cases)
    for case in cases:
        queries, widest = set(), {}
        for rel, text in case['files'].items():
            if not rel.startswith('aln/'):
                continue
            for x in text.splitlines():
                if x and not x.startswith('@'):
                    f = x.split('\t')
                    queries.add((rel, f[0]))
                    widest.setdefault((rel, f[0]), set()).add(f[2])
        assert 0 < len(queries) <= 400, (case['name'], len(queries))
        if case['name'] == 'wide-free':
            assert max(map(len, widest.values())) > 16
        if case['name'] == 'nine-ranks':
            assert len(case['kwargs']['ranks'].split(',')) == 9


def main():
    if sys.argv[1:] == ['check']:
        os.environ['WOLTKA_NO_DLOG'] = '1'
        from woltka_amd.workflow import workflow
        with open(OUT) as fh:
            gold = json.load(fh)
        got = run_all(workflow)
        bad = [k for k in gold if got.get(k) != gold[k]]
        print('fetch route:', 'every entry reproduced' if not bad else bad)
        sys.exit(1 if bad else 0)
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    if sys.argv[1:] == ['emit']:        # (one hash seed: the tables as JSON)
        from woltka.workflow import workflow
        json.dump(run_all(workflow), sys.stdout)
        return
    check_inputs()
    docs = []
    for seed in HASH_SEEDS:
        env = dict(os.environ, PYTHONHASHSEED=seed)
        docs.append(json.loads(subprocess.check_output(
            [sys.executable, os.path.abspath(__file__), 'emit'], env=env)))
    differ = [k for k in docs[0] if docs[0][k] != docs[1][k]]
    if differ:
        sys.exit(f'tables that depend on the hash seed (change the seed of '
                 f'these cases): {differ}')
    for k, v in docs[0].items():
        print(k, v['error'] if 'error' in v else
              {fn: t.count('\n') for fn, t in v['tables'].items()})
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
