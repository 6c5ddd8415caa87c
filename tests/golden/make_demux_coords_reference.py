#!/usr/bin/env python3
"""tests/golden/vectors/demux_coords_device.json: what the REAL reference makes
of the coord-match demultiplexing cases of tests/demux_coords_cases.py (build
container only; the inputs are regenerated from their seeds and from the
bundled alignments).

    python tests/golden/make_demux_coords_reference.py

'reads': per case of `read_cases`, [sample or null, sorted genes] of every
read in the order `ordinal.ordinal_mapper` yields them (its matcher's, not
the text's) -- the reads that matched a gene --, the sample from
`workflow.demultiplex` (null: dropped by the whitelist).  'cli': per case of
`cli_cases`, the tables
`workflow.workflow` writes -- their text where small, their sha256 otherwise
-- and the number of sequences it reports as classified.

As in make_demux_reference.py every command is run under two values of
PYTHONHASHSEED and nothing is written when a result differs between them."""
import contextlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import demux_coords_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'demux_coords_device.json')
HASH_SEEDS = ('11', '4242')


def reads_of(case):
    from woltka.ordinal import load_gene_coords, ordinal_mapper
    from woltka.workflow import demultiplex
    coords, idmap, prefix = load_gene_coords(io.StringIO(T.coords_text()),
                                             sort=True)
    out = []
    for qryque, subque in ordinal_mapper(io.StringIO(case['text']), coords,
                                         idmap, fmt=case['fmt'], n=64, th=0.8,
                                         prefix=prefix):
        for q, genes in zip(list(qryque), list(subque)):
            got = demultiplex([q], [genes], case['samples'])
            assert len(got) <= 1
            out.append([next(iter(got), None), sorted(genes)])
    return out


def emit():
    from woltka.workflow import workflow
    doc = {'reads': {c['name']: reads_of(c) for c in T.read_cases()},
           'cli': {}}
    for case in T.cli_cases():
        with tempfile.TemporaryDirectory() as tmp:
            args = T.write_cli(case, tmp)
            args['output_fp'] = os.path.join(tmp, 'out')
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                workflow(**args)
            n = re.findall(r'Number of sequences classified: (\d+)\.',
                           said.getvalue())
            doc['cli'][case['name']] = {
                'tables': T.digest(T.tables_of(args['output_fp'])),
                'classified': [int(x) for x in n]}
    return doc


def check_inputs():
    """What the cases promise about their inputs."""
    cases = {c['name']: c for c in T.read_cases()}
    for case in cases.values():
        assert 50 <= case['text'].count('\n') <= 700, case['name']
    for name in ('sam-unpaired', 'sam-paired'):
        rows = [x.split('\t') for x in cases[name]['text'].splitlines()[1:]]
        hits = {}
        for f in rows:
            if f[2] != '*':
                hits[f[0], int(f[1]) >> 6 & 3] = \
                    hits.get((f[0], int(f[1]) >> 6 & 3), 0) + 1
        assert max(hits.values()) == 17, name
    for name in ('sam-unpaired', 'sam-paired', 'nine-samples'):
        ids = [x.split('\t', 1)[0]
               for x in cases[name]['text'].splitlines()[1:]]
        runs = [q for i, q in enumerate(ids) if i == 0 or ids[i - 1] != q]
        assert len(runs) == len(set(runs)), name    # an id leads one run
    pair = [x.split('\t') for x in cases['sam-paired']['text'].splitlines()[1:]]
    mates = {}
    for f in pair:
        if f[2] != '*':
            mates.setdefault(f[0], set()).add(int(f[1]) >> 6 & 3)
    assert any({1, 2} <= m for m in mates.values())     # both mates in one run
    assert {0, 1, 2} == mates['S3_']
    assert cases['sam-whitelist']['samples'] == T.WHITELIST
    text = T.text_of('mux5')
    assert text.count('\n') == 10000
    assert max(len(x.split('\t', 1)[0]) for x in text.splitlines()) <= 60


def check_results(doc):
    """What the cases promise about the reference's answers."""
    reads = doc['reads']
    flat, pair = reads['sam-unpaired'], reads['sam-paired']
    for got in (flat, pair):
        samples = {x[0] for x in got}
        assert {'', 'S1', 'S10', 'S1x', 'ninebytes', T.LONG} <= samples
        # (a condition on the inputs: the samples met only in hits of length
        # 0, on the genome without genes, below the threshold or in unmapped
        # lines are none of the reference's)
        assert not samples & set(T.GENELESS), samples & set(T.GENELESS)
        assert all(x[1] for x in got)           # every read matched a gene
    # an id that ends in its first '_': '' unpaired, its left part as a mate
    assert not any(x[0].startswith('Q') for x in flat)
    assert any(x[0].startswith('Q') for x in pair)
    assert 'S1' in {x[0] for x in pair}
    assert 'S3' in {x[0] for x in pair}
    # two hits of a read on one gene: one gene
    assert ['S1', ['GA_1']] in flat
    assert {x[0] for x in reads['sam-whitelist']} == {None, 'S1', 'ninebytes'}
    assert [x[1] for x in reads['sam-whitelist']] == [x[1] for x in pair]
    assert reads['b6o'] == reads['paf'] and len(reads['b6o']) > 40
    assert len({x[0] for x in reads['nine-samples']}) == 9
    cli = doc['cli']
    with open(os.path.join(HERE, 'data', 'output', 'bowtie2.orf.tsv')) as f:
        orf = f.read()
    assert cli['orf']['tables']['out'] == T.digest({'out': orf})['out']
    assert orf.splitlines()[0].split('\t')[1:] == [
        'S01', 'S02', 'S03', 'S04', 'S05'] and orf.count('\n') == 4186
    assert cli['orf']['classified'] == [8001]
    assert cli['orf-sizes']['tables'] != cli['orf']['tables']
    assert cli['nine']['tables'] == cli['cigar']['tables']


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
    check_results(docs[0])
    for k, v in docs[0]['reads'].items():
        print(k, len(v), 'reads,', sorted({x[0] for x in v if x[0] is not None}))
    for k, v in docs[0]['cli'].items():
        print(k, v['classified'], {fn: (t if isinstance(t, dict) else len(t))
                                   for fn, t in v['tables'].items()})
    with open(OUT, 'w') as fh:
        json.dump(docs[0], fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
