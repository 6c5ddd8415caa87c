#!/usr/bin/env python3
"""tests/golden/vectors/mixed_device.json: what the REAL reference makes of
the mixed-rank-set cases of tests/mixed_cases.py (build container only; the
inputs are regenerated from their seeds, only the expected table text / error
of every call is committed).

    python tests/golden/make_mixed_reference.py

{case name: [per call {'tables': {file name: text}} or {'error': [type,
message]}]}.  As in make_demux_reference.py every command is run under two
values of PYTHONHASHSEED and nothing is written when a table differs between
them."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import mixed_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'mixed_device.json')
HASH_SEEDS = ('11', '4242')
COLUMN = {'sam': 2, 'b6o': 1, 'paf': 5, 'map': 1}


def run_all(workflow):
    runs = {}
    for case in T.cases():
        runs[case['name']] = []
        for call in case['calls']:
            with tempfile.TemporaryDirectory() as tmp:
                runs[case['name']].append(T.run_case(workflow, call, tmp))
    return runs


def check_inputs():
    """What the cases promise about their inputs."""
    ranks = T.genome_ranks()
    assert len(ranks) == 107 and len(T.full()) == 103
    assert len(T.lacking('class')) == 3 and len(T.lacking('order')) == 1
    cases = T.cases()
    assert len({c['name'] for c in cases}) == len(cases)
    for case in cases:
        for call in case['calls']:
            assert call['kwargs']['output_fmt'] is False
            assert call['route'] in ('device', 'both', 'host', 'as-plain')
            col = COLUMN[call['kwargs']['input_fmt']]
            n_reads, widest = 0, 0
            for rel, text in call['files'].items():
                per_read = {}
                for x in text.splitlines():
                    if x and not x.startswith('@'):
                        f = x.split('\t')
                        per_read.setdefault(f[0], set()).add(f[col])
                n_reads += len(per_read)
                widest = max([widest] + [len(v) for v in per_read.values()])
            assert 0 < n_reads <= 400, (case['name'], n_reads)
            assert widest == 19 if case['name'] == 'wide-read' \
                else widest <= 16, (case['name'], widest)
    one = {c['name']: c for c in cases}
    files = one['sop8']['calls'][0]['files']
    assert [len({x.split('\t')[0] for x in text.splitlines()[1:]})
            for text in files.values()] == [260, 140]
    assert one['blocks']['calls'][0]['files'] == files
    assert min(len(t) for t in files.values()) > 8192   # several blocks each
    full = set(T.full())
    for text in files.values():
        assert {x.split('\t')[2] for x in text.splitlines()[1:]} <= full
    named = {x.split('\t')[2] for x in
             one['no-class']['calls'][0]['files']['aln/S2.sam'].splitlines()[1:]}
    assert set(T.lacking('class')) <= named


def main():
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
        print(k, ['error' if 'error' in r else
                  {fn: t.count('\n') for fn, t in r['tables'].items()}
                  for r in v])
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
