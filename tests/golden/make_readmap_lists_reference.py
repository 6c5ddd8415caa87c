#!/usr/bin/env python3
"""tests/golden/vectors/readmap_lists_device.json: what the REAL reference
makes of the read-map cases of tests/readmap_lists_cases.py (build container
only; the inputs are regenerated from their seeds).

    python tests/golden/make_readmap_lists_reference.py

'cli': per case of `cli_cases` and `neighbour_cases`, 'maps' -- the text of
every file `workflow.workflow(..., outmap_dir=...)` wrote (decompressed),
verbatim or, above 64 KB, as `readmap_cases.digest` (sha256, bytes, lines) --,
'summary' -- per map its lines, how many of them are lists, and the ends of
the lines of `PROBES` (`readmap_lists_cases.summary`) -- and 'tables'.
'blocks': per case of `block_cases`, the digest of the one map file of the
block under `--rank none`.

The edges the cases are made for, and the share of lists in every command, are
asserted on the reference's text (`readmap_lists_cases.check_gold`) before
anything is written.  As in make_readmap_reads_reference.py everything is made
under two values of PYTHONHASHSEED and nothing is written when the two
differ."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import readmap_lists_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'readmap_lists_device.json')
HASH_SEEDS = ('11', '4242')


def block_of(workflow, n, tmp):
    import contextlib
    import io
    os.makedirs(os.path.join(tmp, 'aln'))
    with open(os.path.join(tmp, 'aln', 'S.map'), 'wb') as f:
        f.write(T.block_text(n))
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=os.path.join(tmp, 'aln'), input_fmt='map',
                 output_fp=os.path.join(tmp, 'out'), output_fmt=False,
                 ranks='none', outmap_dir=os.path.join(tmp, 'maps'),
                 outmap_zip=None)
    with open(os.path.join(tmp, 'maps', 'S.txt'), 'rb') as f:
        return T.digest(f.read())


def emit():
    from woltka.workflow import workflow
    doc = {'cli': {}, 'blocks': {}}
    for case in T.cli_cases() + T.neighbour_cases():
        if case['gold'] != case['name']:    # (the same command on the same files)
            continue
        with tempfile.TemporaryDirectory() as tmp:
            got = T.run_cli(workflow, case, tmp)
        doc['cli'][case['name']] = {
            'maps': {k: T.kept(v) for k, v in sorted(got['maps'].items())},
            'summary': {k: T.summary(v)
                        for k, v in sorted(got['maps'].items())},
            'tables': got['tables']}
    for name, n in T.block_cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            doc['blocks'][name] = block_of(workflow, n, tmp)
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
        differ = [k for part in ('cli', 'blocks') for k in docs[0][part]
                  if docs[0][part][k] != docs[1][part][k]]
        sys.exit(f'results that depend on the hash seed: {differ}')
    T.check_gold(docs[0])
    for k, v in docs[0]['cli'].items():
        print(k, {fn: (s['lists'], s['lines'])
                  for fn, s in v['summary'].items()},
              {fn: len(t) for fn, t in v['tables'].items()})
    for k, v in docs[0]['blocks'].items():
        print(k, v['bytes'], v['lines'], v['sha256'][:16])
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
