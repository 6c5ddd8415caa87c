#!/usr/bin/env python3
"""tests/golden/vectors/demux_device.json: what the REAL reference makes of
the demultiplexing cases of tests/demux_cases.py (build container only; the
inputs are regenerated from their seeds and from the bundled alignments).

    python tests/golden/make_demux_reference.py

'reads': per case of `read_cases`, [sample or null, sorted subjects] of every
read in the order `align.plain_mapper` yields them, the sample from
`workflow.demultiplex` (null: dropped by the whitelist).  'cli': per case of
`cli_cases`, the tables `workflow.workflow` writes -- their text where small,
their sha256 otherwise.

As in make_logred_reference.py every command is run under two values of
PYTHONHASHSEED and nothing is written when a table differs between them."""
import io
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import demux_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'demux_device.json')
HASH_SEEDS = ('11', '4242')


def reads_of(case):
    from woltka.align import plain_mapper
    from woltka.workflow import demultiplex
    out = []
    excl = set(case['exclude']) if case['exclude'] else None
    for qryque, subque in plain_mapper(io.StringIO(case['text']),
                                       fmt=case['fmt'], excl=excl, n=64):
        for q, subs in zip(qryque, subque):
            got = demultiplex([q], [subs], case['samples'])
            assert len(got) <= 1
            out.append([next(iter(got), None), sorted(subs)])
    return out


def emit():
    from woltka.workflow import workflow
    doc = {'reads': {c['name']: reads_of(c) for c in T.read_cases()},
           'cli': {}}
    texts = {}
    for case in T.cli_cases():
        if case['text'] not in texts:
            texts[case['text']] = T.mux5_text() if case['text'] == 'mux5' \
                else T.trimsub_text()
        with tempfile.TemporaryDirectory() as tmp:
            doc['cli'][case['name']] = T.run_cli(workflow, case, tmp,
                                                 texts[case['text']])
    return doc


def check_inputs():
    """What the cases promise about their inputs."""
    for case in T.read_cases():
        assert 50 < case['text'].count('\n') < 700, case['name']
    text = T.mux5_text()
    widest, ids = {}, set()
    for line in text.splitlines():
        f = line.split('\t')
        ids.add(f[0])
        if f[2] != '*':
            widest.setdefault(f[0], set()).add(f[2])
    assert max(map(len, ids)) <= 60
    assert max(map(len, widest.values())) <= 16


def main():
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    if sys.argv[1:] == ['emit']:
        json.dump(emit(), sys.stdout)
        return
    check_inputs()
    docs = []
    for seed in HASH_SEEDS:
        env = dict(os.environ, PYTHONHASHSEED=seed)
        docs.append(json.loads(subprocess.check_output(
            [sys.executable, os.path.abspath(__file__), 'emit'], env=env)))
    if docs[0] != docs[1]:
        differ = [k for k in docs[0]['cli']
                  if docs[0]['cli'][k] != docs[1]['cli'][k]]
        sys.exit(f'results that depend on the hash seed: {differ or "reads"}')
    for k, v in docs[0]['reads'].items():
        print(k, len(v), 'reads,', sorted({x[0] for x in v if x[0] is not None}))
    for k, v in docs[0]['cli'].items():
        print(k, {fn: (t if isinstance(t, dict) else len(t))
                  for fn, t in v.items()})
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
