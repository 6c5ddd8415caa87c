#!/usr/bin/env python3
"""tests/golden/vectors/coords_rows.json: what the REAL reference makes of the
hand-written rows of tests/coords_rows_cases.py (build container only; data
only -- the rows themselves stay in the cases module).

    python tests/golden/make_coords_rows_reference.py

'cases': per case
  'records'  what `align.iter_align(fh, fmt, None, True)` yields over the
             case's text, as [query, [[subject, length, start, end], ...]], or
             the name of the exception's type
  'genes'    what `ordinal.ordinal_mapper` (threshold 1.0) makes of it over the
             probe genes of the case (coords_rows_cases.probe_genes, built from
             'records') and the good rows' gene, as [query, sorted genes] per
             read it yields, or the exception's name (null where the parser
             raised already)
  'ranges'   per subject, `range.merge_ranges` over the ranges of every record
'raises': per case, the name of the exception `workflow.workflow` ends with --
  null: none -- over a file of the row between good rows, once with
  `coords_fp` (threshold 100) and once, without it, with `outcov_dir`
'cli': per format, over one file (coords_rows_cases.cli_text) of every row
  that is not wide and on which the `coords_fp` command does not raise, between
  two pads of good rows: its table and the numbers of its
  "Number of sequences classified" lines; the same of the `outcov_dir` command,
  and its .cov files.

Every result is computed under two values of PYTHONHASHSEED; nothing is written
when they differ, when the cases module's claims about the reference ('ref',
'finding') do not hold, or when the file would pass the size limit."""
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

import coords_rows_cases as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'coords_rows.json')
HASH_SEEDS = ('11', '4242')
SIZE_LIMIT = 1 << 20


def _fh(text):
    """The text as the reference's commands read it: universal newlines."""
    return io.TextIOWrapper(io.BytesIO(text.encode()), newline=None)


def records_of(case):
    from woltka.align import iter_align
    try:
        return [[q, [[s, ln, b, e] for s, _, ln, b, e in recs]] for q, recs in
                iter_align(_fh(case['text'] + '\n'), case['fmt'], None, True)]
    except Exception as e:      # noqa: BLE001 - its type is the result
        return type(e).__name__


def genes_of(case, doc):
    from woltka.ordinal import load_gene_coords, ordinal_mapper
    if not isinstance(doc['cases'][case['name']]['records'], list):
        return None
    coords, idmap, _ = load_gene_coords(
        io.StringIO(T.coords_text([case], doc)), sort=True)
    try:
        out = []
        for qryque, subque in ordinal_mapper(
                _fh(case['text'] + '\n'), coords, idmap, fmt=case['fmt'],
                n=1024, th=1.0, prefix=True):
            out += [[q, sorted(g)] for q, g in zip(list(qryque), list(subque))]
        return out
    except Exception as e:      # noqa: BLE001
        return type(e).__name__


def ranges_of(records):
    from woltka.range import merge_ranges
    flat = {}
    for _, recs in records:
        for s, _, b, e in recs:
            flat.setdefault(s, []).extend((b, e))
    return {s: merge_ranges(r) for s, r in flat.items()}


def _command(text, fmt, tmp, coords=None):
    """workflow.workflow over one file S1.<fmt>: with `coords` the coord-match
    at threshold 100, else the plain classification with --outcov."""
    from woltka.workflow import workflow
    os.makedirs(os.path.join(tmp, 'in'))
    with open(os.path.join(tmp, 'in', f'S1.{fmt}'), 'w') as f:
        f.write(text)
    kw = dict(input_fp=os.path.join(tmp, 'in'), input_fmt=fmt,
              output_fp=os.path.join(tmp, 'out.tsv'))
    if coords is not None:
        with open(os.path.join(tmp, 'coords.txt'), 'w') as f:
            f.write(coords)
        kw.update(coords_fp=os.path.join(tmp, 'coords.txt'), overlap=100)
    else:
        kw.update(outcov_dir=os.path.join(tmp, 'cov'))
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        workflow(**kw)
    with open(kw['output_fp']) as f:
        res = {'table': f.read(), 'classified': [int(x) for x in re.findall(
            r'Number of sequences classified: (\d+)\.', said.getvalue())]}
    if coords is None:
        res['cov'] = {fn: open(os.path.join(tmp, 'cov', fn)).read()
                      for fn in sorted(os.listdir(os.path.join(tmp, 'cov')))}
    return res


def raises_of(case, doc):
    out = {}
    for key, coords in (('coords', T.coords_text([case], doc, command=True)),
                        ('outcov', None)):
        with tempfile.TemporaryDirectory() as tmp:
            try:
                _command(T.around(case), case['fmt'], tmp, coords)
                out[key] = None
            except Exception as e:      # noqa: BLE001
                out[key] = type(e).__name__
    return out


def emit():
    doc = {'cases': {}, 'raises': {}, 'cli': {}}
    for case in T.cases():
        rec = records_of(case)
        doc['cases'][case['name']] = {
            'records': rec,
            'ranges': ranges_of(rec) if isinstance(rec, list) else None}
    for case in T.cases():
        doc['cases'][case['name']]['genes'] = genes_of(case, doc)
        doc['raises'][case['name']] = raises_of(case, doc)
    for fmt in T.FORMATS:
        rows = [c for c in T.cases(fmt) if T.in_cli_file(c, doc)]
        text = T.cli_text(rows)
        res = {'rows': [c['name'] for c in rows]}
        with tempfile.TemporaryDirectory() as tmp:
            res['coords'] = _command(text, fmt, tmp,
                                     T.coords_text(rows, doc, command=True))
        with tempfile.TemporaryDirectory() as tmp:
            res['outcov'] = _command(text, fmt, tmp)
        doc['cli'][fmt] = res
    return doc


def check_results(doc):
    """What the cases module says about the reference."""
    for case in T.cases():
        got, name = doc['cases'][case['name']], case['name']
        rec = got['records']
        if case['ref'] == 'raises':
            assert rec == 'ValueError', (name, rec)
            assert doc['raises'][name] == {'coords': 'ValueError',
                                           'outcov': 'ValueError'}, name
            continue
        assert isinstance(rec, list), (name, rec)
        hits = [r for _, recs in rec for r in recs]
        if case['ref'] == 'skips':
            assert not hits, (name, rec)
        else:
            assert hits and all(r[0] == case['subject'] for r in hits), name
        if case['finding']:
            # the parser takes the negative length, the matcher refuses it,
            # the coverage never reads it
            assert [r[1] for r in hits] == [-5], (name, rec)
            assert got['genes'] == 'OverflowError', (name, got['genes'])
            assert doc['raises'][name] == {'coords': 'OverflowError',
                                           'outcov': None}, doc['raises'][name]
        elif case['cls'] != T.WIDE:
            assert isinstance(got['genes'], list), (name, got['genes'])
            assert doc['raises'][name] == {'coords': None, 'outcov': None}, \
                (name, doc['raises'][name])
        if case['cls'] == T.STAY:
            # a stay row's numbers are all within int32
            assert all(-2 ** 31 < v < 2 ** 31 for r in hits for v in r[1:]), \
                name
            # every positive hit that can match a gene matches `a` and `b`
            # of its own and nothing else
            want = {}
            for q, recs in rec:
                for r in [r for r in recs if r[1] > 0]:
                    if r[3] - r[2] >= r[1]:
                        genes = {g[0] for g in T.probe_genes(T.hits_of(rec))
                                 if g[1:] in ((r[2], r[2] + r[1]),
                                              (r[3] - r[1], r[3]))}
                        want.setdefault(q, set()).update(
                            f'{case["subject"]}_{g}' for g in genes)
                        assert genes, name
            assert got['genes'] == [[q, sorted(g)] for q, g in want.items()], \
                (name, got['genes'], want)
    for fmt in T.FORMATS:
        cli = doc['cli'][fmt]
        assert len(cli['rows']) >= 15, fmt
        assert cli['coords']['table'].count('\n') >= 8, fmt
        assert cli['outcov']['cov']['S1.cov'].count('\n') >= 10, fmt


def main():
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    if sys.argv[1:] == ['emit']:
        json.dump(emit(), sys.stdout)
        return
    T.check_cases()
    docs = []
    for seed in HASH_SEEDS:
        env = dict(os.environ, PYTHONHASHSEED=seed)
        docs.append(json.loads(subprocess.check_output(
            [sys.executable, os.path.abspath(__file__), 'emit'], env=env)))
    if docs[0] != docs[1]:
        differ = [k for k in docs[0] for n in docs[0][k]
                  if docs[0][k][n] != docs[1][k][n]]
        sys.exit(f'results that depend on the hash seed: {differ}')
    check_results(docs[0])
    blob = json.dumps(docs[0], separators=(',', ':'), sort_keys=True) + '\n'
    if len(blob) >= SIZE_LIMIT:
        sys.exit(f'{len(blob)} bytes: over the limit for a committed file')
    for fmt in T.FORMATS:
        cli = docs[0]['cli'][fmt]
        print(fmt, len(cli['rows']), 'rows in the file; classified',
              cli['coords']['classified'], cli['outcov']['classified'])
    odd = {n: r for n, r in docs[0]['raises'].items() if any(r.values())}
    for n, r in odd.items():
        print('raises', n, r)
    with open(OUT, 'w') as fh:
        fh.write(blob)
    print(len(blob), 'bytes')


if __name__ == '__main__':
    main()
