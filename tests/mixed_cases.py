"""Inputs of the mixed-rank-set cases of tests/golden/vectors/mixed_device.json
(`--rank none,free,phylum,...`: whole-read jobs next to plain ones on the
packed-record route): regenerated from seeds, both by
tests/golden/make_mixed_reference.py (which runs the reference on them) and by
tests/test_gpu_mixed.py.  Only the expected table text / error of every call is
committed.

Every case is plain classification of a directory of alignment files over the
bundled taxonomy, at most 400 reads, `output_fmt=False`.  A case is one or two
`workflow` calls; a call carries the route expected of it:

    device    every block appended under the mixed set on the device
    both      blocks on the device, then the hand-off to the host tokenizer
    host      the general route (the set is none the mixed entry takes)
    as-plain  whatever the set's plain ranks alone (`plain_ranks`) take

`block`: the device tokenizer's block size for the call (`Engine.DTOK_BLOCK`,
WOLTKA_DTOK_BLOCK): reads cut by block ends, several blocks per sample."""
import os
import random

from sizes_cases import (TAX, TREE, as_b6o, as_map, as_paf, as_sam,  # noqa: F401
                         genome_ranks, reads, run_case, write_case)

SOP6 = ('phylum', 'class', 'order', 'family', 'genus', 'species')
SOP8 = 'none,free,' + ','.join(SOP6)


def genomes():
    """Every genome of the bundled `taxid.map`, in file order."""
    return list(genome_ranks())


def full():
    """`FULL`: the genomes with an ancestor at all six ranks of SOP6."""
    return [g for g, have in genome_ranks().items() if set(SOP6) <= have]


def lacking(rank):
    return [g for g, have in genome_ranks().items() if rank not in have]


def _call(files, route, block=None, **kw):
    kwargs = dict(input_fp='aln', output_fmt=False)
    kwargs.update(kw)
    call = dict(files=files, kwargs=kwargs, route=route)
    if block:
        call['block'] = block
    return call


def cases():
    """[{'name', 'calls': [{'files': {relative path: text}, 'kwargs': of
    workflow.workflow, 'route', 'block'?, 'plain_ranks'?}]}]"""
    G, FULL = genomes(), full()
    out = []

    def case(name, *calls):
        out.append(dict(name=name, calls=list(calls)))

    sop = {'aln/S1.sam': as_sam(reads(1100, 260, FULL, 6)),
           'aln/S2.sam': as_sam(reads(1101, 140, FULL, 6))}
    case('sop8', _call(sop, 'device', input_fmt='sam', ranks=SOP8, **TREE))
    # the whole-read job first: the job ids in the keys
    case('free-first', _call({'aln/S1.sam': as_sam(reads(1200, 300, G, 5))},
                             'device', input_fmt='sam', ranks='free,none',
                             **TREE))
    case('two-whole', _call({'aln/S1.sam': as_sam(reads(1300, 320, FULL, 7))},
                            'device', input_fmt='sam', ranks='none,free,genus',
                            above=True, **TREE))
    case('major', _call({'aln/S1.sam': as_sam(reads(1400, 350, FULL, 6))},
                        'device', input_fmt='sam', ranks='none,genus',
                        major=80, **TREE))
    recs = reads(1500, 300, FULL, 6)
    case('unassigned-subok',
         _call({'aln/S1.sam': as_sam(recs)}, 'device', input_fmt='sam',
               ranks='none,free,genus', unassigned=True, **TREE),
         _call({'aln/S1.sam': as_sam(recs)}, 'device', input_fmt='sam',
               ranks='none,free', subok=True, **TREE))
    case('blocks', _call(sop, 'device', block=8192, input_fmt='sam',
                         ranks=SOP8, **TREE))
    recs = reads(1600, 380, FULL, 7)
    for fmt, ext, render in (('b6o', 'b6', as_b6o), ('paf', 'paf', as_paf),
                             ('map', 'map', as_map)):
        case(fmt, _call({f'aln/S1.{ext}': render(recs)}, 'device',
                        input_fmt=fmt, ranks='none,free,genus', **TREE))
    case('gz', _call({'aln/S1.sam.gz': as_sam(reads(1700, 250, FULL, 4)),
                      'aln/S2.sam.gz': as_sam(reads(1701, 120, FULL, 9))},
                     'device', input_fmt='sam', ranks='none,free,genus',
                     **TREE))
    # `--trim-sub` on subjects G..._1; `--exclude` (both: `words_dev`)
    rng = random.Random(1810)
    recs = [(q, list(dict.fromkeys(f'{s}_{rng.randint(1, 3)}' for s in subs)))
            for q, subs in reads(1800, 400, FULL[:40], 6)]
    case('trimsub',
         _call({'aln/S1.sam': as_sam(recs)}, 'device', input_fmt='sam',
               ranks='none,free,genus', trimsub='_', **TREE),
         _call({'aln/S1.sam': as_sam(reads(1801, 400, FULL[:30], 6))},
               'device', input_fmt='sam', ranks='none,free,genus',
               exclude=','.join(FULL[1:4]), **TREE))
    # the SOP's other branch: a hierarchy from lineage strings
    lin = _call({'aln/S1.sam': as_sam(reads(1900, 300, G, 5))}, 'as-plain',
                input_fmt='sam', ranks='none,free,phylum,genus',
                lineage_fps=['$TAX/lineages.txt'])
    lin['plain_ranks'] = 'phylum,genus'
    case('lineage', lin)
    # genomes without a class: the second file's reads name them
    no_class = lacking('class')
    case('no-class', _call(
        {'aln/S1.sam': as_sam(reads(2000, 300, FULL, 5)),
         'aln/S2.sam': as_sam(reads(2001, 100, no_class + FULL[:5], 3))},
        'both', block=8192, input_fmt='sam', ranks='none,free,class', **TREE))
    # a subject outside the tree, two thirds into the file
    recs = reads(2100, 390, FULL, 5)
    recs.insert(260, ('stranger', [FULL[0], 'NOT_IN_TREE']))
    recs.insert(300, ('again', ['NOT_IN_TREE']))
    case('stranger', _call({'aln/S1.sam': as_sam(recs)}, 'both', block=8192,
                           input_fmt='sam', ranks='none,free,genus', **TREE))
    # one read of 19 subjects in the middle of the file
    recs = reads(2200, 399, FULL, 5)
    recs.insert(200, ('wide', random.Random(22).sample(FULL, 19)))
    case('wide-read', _call({'aln/S1.sam': as_sam(recs)}, 'both', block=8192,
                            input_fmt='sam', ranks='none,free,genus', **TREE))
    # `none` under --uniq is no plain job
    case('uniq', _call({'aln/S1.sam': as_sam(reads(2300, 300, FULL, 5))},
                       'host', input_fmt='sam', ranks='none,free', uniq=True,
                       **TREE))
    return out
