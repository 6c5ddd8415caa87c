"""Inputs of the `--sizes` cases of tests/golden/vectors/logred_device.json:
the calls that go through the general evaluator's contribution log, which the
device reduces (csrc/wk_logred.hpp).  Regenerated from seeds, both by
tests/golden/make_logred_reference.py (which runs the reference on them) and
by tests/test_gpu_logred_cli.py.  Only the expected table text / error of
every case is committed.

Every case has at most 400 reads, `--scale 1M --digits 3`; subjects are
genomes of `sizes_cases.ranked_genomes()` where ranks are needed."""
import os
import random

import sizes_cases as SC

TREE = SC.TREE
RANKS9 = ('none', 'free', 'superkingdom', 'phylum', 'class', 'order', 'family',
          'genus', 'species')


def _case(name, files, **kw):
    kwargs = dict(input_fp='aln', input_fmt='sam', output_fmt=False,
                  scale='1M', digits=3, sizes='$TAX/length.map')
    kwargs.update(kw)
    return dict(name=name, files=files, kwargs=kwargs)


def cases():
    """As `sizes_cases.cases`; 'strata' names the directory of the strata maps
    made from 'files'."""
    G = SC.ranked_genomes()
    out = []
    out.append(_case('free', {'aln/S1.sam': SC.as_sam(SC.reads(1100, 300, G, 6)),
                              'aln/S2.sam': SC.as_sam(SC.reads(1101, 90, G, 4))},
                     ranks='free', **TREE))
    out.append(_case('uniq', {'aln/S1.sam': SC.as_sam(SC.reads(1200, 380, G, 5))},
                     ranks='genus', uniq=True, **TREE))
    out.append(_case('major', {'aln/S1.sam': SC.as_sam(SC.reads(1300, 390, G[:60], 7))},
                     ranks='genus', major=80, **TREE))
    out.append(_case('above', {'aln/S1.sam': SC.as_sam(SC.reads(1400, 350, G, 5))},
                     ranks='phylum', above=True, **TREE))
    out.append(_case('mixed', {'aln/S1.sam': SC.as_sam(SC.reads(1500, 260, G, 6)),
                               'aln/S2.sam': SC.as_sam(SC.reads(1501, 140, G, 3))},
                     ranks='free,genus,none', **TREE))
    # a subject outside the hierarchy, alone in a read and next to a genome
    recs = SC.reads(1600, 300, G, 5)
    recs.insert(3, ('mixed', [G[0], 'NOGENUS1']))
    recs.insert(150, ('alone', ['NOGENUS1']))
    with open(os.path.join(SC.TAX, 'length.map')) as f:
        lengths = f.read()
    out.append(_case('unassigned', {'aln/S1.sam': SC.as_sam(recs),
                                    'sizes.map': lengths + 'NOGENUS1\t5000\n'},
                     ranks='genus', unassigned=True, sizes='sizes.map', **TREE))
    # --stratify: a small strata map per sample; some reads are in no stratum
    files = {}
    for k in range(2):
        recs = SC.reads(1700 + k, 180, G, 5)
        rng = random.Random(1710 + k)
        files[f'aln/T{k}.sam'] = SC.as_sam(recs)
        files[f'strata/T{k}.txt'] = ''.join(
            f'{q}\t{rng.choice(("soil", "gut", "reef"))}\n'
            for q, _ in recs if rng.random() < 0.85)
    out.append(_case('stratify', files, ranks='genus', strata_dir='strata', **TREE))
    # --demux on one multiplexed file: the sample is the query's prefix
    rng = random.Random(1800)
    recs = [(f'M{rng.randint(1, 3)}_{q}', subs) for q, subs in SC.reads(1801, 390, G, 5)]
    out.append(_case('demux', {'aln/mux.sam': SC.as_sam(recs)},
                     input_fp='aln/mux.sam', demux=True, ranks='genus', uniq=True, **TREE))
    # nine ranks: two batches of jobs (job bases 0 and 8)
    out.append(_case('nine-ranks', {'aln/S1.sam': SC.as_sam(SC.reads(1900, 250, G, 5)),
                                    'aln/S2.sam': SC.as_sam(SC.reads(1901, 120, G, 8))},
                     ranks=','.join(RANKS9), **TREE))
    # a read of more than 16 subjects
    recs = SC.reads(2000, 300, G, 5)
    recs.insert(120, ('wide', random.Random(20).sample(G, 19)))
    out.append(_case('wide-free', {'aln/S1.sam': SC.as_sam(recs)}, ranks='free', **TREE))
    # a contributing subject that is not in the size map
    recs = SC.reads(2100, 200, G[:20], 4)
    out.append(_case('unsized', {'aln/S1.sam': SC.as_sam(recs),
                                 'sizes.map': SC.size_map([g for g in G[:20] if g != G[2]], 21)},
                     ranks='free', sizes='sizes.map', **TREE))
    return out


def write_case(case, root):
    """`sizes_cases.write_case`, with the directory of strata maps."""
    args = SC.write_case(case, root)
    if args.get('strata_dir'):
        args['strata_dir'] = os.path.join(root, args['strata_dir'])
    return args


def run_case(workflow, case, root):
    """As `sizes_cases.run_case`."""
    import contextlib
    import io
    args = write_case(case, root)
    out = os.path.join(root, 'out')
    args['output_fp'] = out
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            workflow(**args)
    except Exception as e:                  # noqa: BLE001 (the reference's own)
        return {'error': [type(e).__name__, str(e)]}
    if os.path.isdir(out):
        return {'tables': {fn: open(os.path.join(out, fn)).read()
                           for fn in sorted(os.listdir(out))}}
    with open(out) as f:
        return {'tables': {'out': f.read()}}
