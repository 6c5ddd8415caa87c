#!/usr/bin/env python3
"""tests/golden/vectors/readmap_demux_device.json: what the REAL reference
makes of the demultiplexed read-map cases of tests/readmap_demux_cases.py
(build container only; the inputs are regenerated from their seeds).

    python tests/golden/make_readmap_demux_reference.py

'cli': per case of `cli_cases`, 'maps' -- the text of every file
`workflow.workflow(..., outmap_dir=...)` wrote (decompressed), verbatim or,
above 64 KB, as `readmap_cases.digest` (sha256, bytes, lines) -- and 'tables'.

The edges the cases are made for are asserted on the reference's text
(`readmap_demux_cases.check_gold`) before anything is written.  As in
make_readmap_reads_reference.py everything is made under two values of
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

import readmap_demux_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'readmap_demux_device.json')
HASH_SEEDS = ('11', '4242')


def emit():
    from woltka.workflow import workflow
    doc = {'cli': {}}
    for case in T.cli_cases():
        if case['gold'] != case['name']:    # (the same command on the same files)
            continue
        with tempfile.TemporaryDirectory() as tmp:
            got = T.run_cli(workflow, case, tmp)
        doc['cli'][case['name']] = {
            'maps': {k: T.kept(v) for k, v in sorted(got['maps'].items())},
            'tables': got['tables']}
    return doc


def main():
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    if sys.argv[1:] == ['emit']:
        json.dump(emit(), sys.stdout)
        return
    T.check_inputs()
    docs = []
    for seed in HASH_SEEDS:
        env = dict(os.environ, PYTHONHASHSEED=seed)
        docs.append(json.loads(subprocess.check_output(
            [sys.executable, os.path.abspath(__file__), 'emit'], env=env)))
    if docs[0] != docs[1]:
        differ = [k for k in docs[0]['cli']
                  if docs[0]['cli'][k] != docs[1]['cli'][k]]
        sys.exit(f'results that depend on the hash seed: {differ}')
    T.check_gold(docs[0])
    for k, v in docs[0]['cli'].items():
        print(k, len(v['maps']), 'maps,',
              sum(len(t) if isinstance(t, str) else t['bytes']
                  for t in v['maps'].values()), 'bytes;',
              {fn: len(t) for fn, t in v['tables'].items()})
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
