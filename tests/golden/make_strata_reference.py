#!/usr/bin/env python3
"""tests/golden/vectors/strata_device.json: what the REAL reference makes of
the strata maps and commands of tests/strata_cases.py (build container only;
the inputs are regenerated from their seeds).

    python tests/golden/make_strata_reference.py

'maps': per case of `map_cases`, 'strata' -- the dict of
`workflow.read_strata` on the map written to a file, or ['ValueError',
message] -- and 'labels' -- the values `file.read_map_uniq` yields over the
file opened with `file.readzip`, each once, in order.  Of the two maps around
the device's label cap only the sha256 of the sorted `key<tab>label` lines
and the number of labels are kept.  'cli': per case of `cli_cases`, the
tables `workflow.workflow` writes, or its error.

As in make_demux_reference.py everything is made under two values of
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

import strata_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'strata_device.json')
HASH_SEEDS = ('11', '4242')


def map_of(name, text, tmp):
    from woltka.file import read_map_uniq, readzip
    from woltka.workflow import read_strata
    fp = os.path.join(tmp, 'map.txt')
    with open(fp, 'wb') as f:
        f.write(text)
    try:
        strata = read_strata(fp)
    except ValueError as e:
        strata = ['ValueError', str(e)]
    with readzip(fp) as fh:
        labels = list(dict.fromkeys(v for _, v in read_map_uniq(fh)))
    if name.startswith('labels-'):
        assert list(strata.values()) == labels
        return {'strata': {'sha256': T.dict_digest(strata),
                           'pairs': len(strata)},
                'labels': {'count': len(labels)}}
    return {'strata': strata, 'labels': labels}


def emit():
    from woltka.workflow import workflow
    doc = {'maps': {}, 'cli': {}}
    for name, text in T.map_cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            doc['maps'][name] = map_of(name, text, tmp)
    for case in T.cli_cases():
        with tempfile.TemporaryDirectory() as tmp:
            doc['cli'][case['name']] = T.run_cli(workflow, case, tmp)
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
        differ = [k for part in ('maps', 'cli') for k in docs[0][part]
                  if docs[0][part][k] != docs[1][part][k]]
        sys.exit(f'results that depend on the hash seed: {differ}')
    for k, v in docs[0]['maps'].items():
        print(k, v['strata'] if isinstance(v['strata'], list)
              else len(v['strata']), 'labels:',
              v['labels'] if len(v['labels']) < 12 else len(v['labels']))
    for k, v in docs[0]['cli'].items():
        print(k, v.get('error') or {fn: len(t)
                                    for fn, t in v['tables'].items()})
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
