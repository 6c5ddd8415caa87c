"""Inputs of the `--sizes` cases of tests/golden/vectors/sizes_device.json:
regenerated from seeds, both by tests/golden/make_sizes_reference.py (which
runs the reference on them) and by tests/test_gpu_sizes.py.  Only the expected
table text / error of every case is committed.

Every case is plain classification of a directory of alignment files with a
size map, `--scale 1M --digits 3` unless it says otherwise; at most 400 reads.
Subjects of the cases with a hierarchy are genomes of the bundled
`taxonomy/taxid.map` that have an ancestor at phylum, genus and species in
`taxonomy/nodes.dmp` (`ranked_genomes`; the generator asserts it)."""
import gzip
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
TAX = os.path.join(HERE, 'golden', 'data', 'taxonomy')
RANKS3 = ('phylum', 'genus', 'species')


def genome_ranks():
    """{genome: set of the ranks on its path to the root} of the bundled
    taxonomy."""
    parent, rank = {}, {}
    with open(os.path.join(TAX, 'nodes.dmp')) as f:
        for line in f:
            x = [y.strip() for y in line.split('|')]
            parent[x[0]], rank[x[0]] = x[1], x[2]
    out = {}
    with open(os.path.join(TAX, 'taxid.map')) as f:
        for line in f:
            g, t = line.split()
            have = set()
            while True:
                have.add(rank.get(t))
                if t not in parent or parent[t] == t:
                    break
                t = parent[t]
            out[g] = have
    return out


def ranked_genomes():
    """Genomes with an ancestor at each of RANKS3 and a length in the bundled
    `length.map`, in file order."""
    with open(os.path.join(TAX, 'length.map')) as f:
        sized = {line.split()[0] for line in f if line.strip()}
    return [g for g, have in genome_ranks().items()
            if set(RANKS3) <= have and g in sized]


def reads(seed, n, pool, kmax=6, name='r'):
    """``n`` reads as (query name, list of distinct subjects): most have one
    subject, the others 2..kmax; subjects are drawn unevenly from ``pool``."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        k = 1 if rng.random() < 0.55 else rng.randint(2, kmax)
        subs = []
        while len(subs) < k:
            s = pool[min(int(rng.expovariate(1 / (len(pool) / 4))),
                         len(pool) - 1)]
            if s not in subs:
                subs.append(s)
        out.append((f'{name}{i:04d}', subs))
    return out


# ---- the same records in the four formats ----------------------------------
def as_sam(recs, paired=False):
    lines = ['@HD\tVN:1.0\tSO:unsorted']
    for i, (q, subs) in enumerate(recs):
        for j, s in enumerate(subs):
            flag = 0
            if paired:      # both mates: the first subjects on /1, the rest on /2
                flag = 65 if j < (len(subs) + 1) // 2 else 129
            lines.append(f'{q}\t{flag}\t{s}\t{1 + 7 * i + j}\t42\t50M\t*\t0\t0'
                         '\t*\t*')
    return '\n'.join(lines) + '\n'


def as_b6o(recs):
    return ''.join(f'{q}\t{s}\t98.5\t50\t1\t0\t1\t50\t{1 + 7 * i + j}'
                   f'\t{50 + 7 * i + j}\t1e-20\t95.0\n'
                   for i, (q, subs) in enumerate(recs)
                   for j, s in enumerate(subs))


def as_paf(recs):
    return ''.join(f'{q}\t50\t0\t50\t+\t{s}\t100000\t{7 * i + j}'
                   f'\t{50 + 7 * i + j}\t50\t50\t60\n'
                   for i, (q, subs) in enumerate(recs)
                   for j, s in enumerate(subs))


def as_map(recs):
    return ''.join(f'{q}\t{s}\n' for q, subs in recs for s in subs)


def size_map(subjects, seed):
    rng = random.Random(seed)
    return ''.join(f'{s}\t{rng.randint(900, 9_000_000)}\n' for s in subjects)


TREE = dict(nodes_fps=['$TAX/nodes.dmp'], map_fps=['$TAX/taxid.map'])


def _case(name, files, **kw):
    kwargs = dict(input_fp='aln', output_fmt=False, scale='1M', digits=3)
    kwargs.update(kw)
    return dict(name=name, files=files, kwargs=kwargs)


def cases():
    """[{'name', 'files': {relative path: text}, 'kwargs': of
    workflow.workflow ('$TAX/...': a bundled file, 'aln' / 'sizes.map': made
    from 'files')}] -- a file whose name ends in .gz is written through
    gzip."""
    G = ranked_genomes()
    out = []
    # 1. every divisor: reads of 1, 2, ..., 16 distinct subjects, `--rank none`
    rng = random.Random(101)
    pool = [f'S{i:03d}' for i in range(40)]
    recs = []
    for i in range(336):
        recs.append((f'd{i:04d}', rng.sample(pool, 1 + i % 16)))
    rng.shuffle(recs)
    out.append(_case('1-divisors', {'aln/S1.sam': as_sam(recs),
                                    'sizes.map': size_map(pool, 1)},
                     input_fmt='sam', ranks='none', sizes='sizes.map'))
    # 2. three samples, both mates, three ranks, the bundled maps
    files = {f'aln/P{k}.sam': as_sam(reads(200 + k, 80 + 40 * k, G, 5),
                                     paired=True) for k in range(3)}
    out.append(_case('2-paired-ranks', files, input_fmt='sam',
                     ranks=','.join(RANKS3), sizes='$TAX/length.map', **TREE))
    # 3. the same records as BLAST tabular, PAF and a simple map
    recs = reads(300, 380, G, 7)
    for fmt, ext, render in (('b6o', 'b6', as_b6o), ('paf', 'paf', as_paf),
                             ('map', 'map', as_map)):
        out.append(_case(f'3-{fmt}', {f'aln/S1.{ext}': render(recs)},
                         input_fmt=fmt, ranks=','.join(RANKS3),
                         sizes='$TAX/length.map', **TREE))
    # 4. gzip
    out.append(_case('4-gz', {'aln/S1.sam.gz': as_sam(reads(400, 250, G, 4)),
                              'aln/S2.sam.gz': as_sam(reads(401, 120, G, 9))},
                     input_fmt='sam', ranks='genus,species',
                     sizes='$TAX/length.map', **TREE))
    # 5. --exclude; --trim-sub with a size map keyed by the trimmed ids
    recs = reads(500, 400, G[:30], 6)
    out.append(_case('5-exclude', {'aln/S1.sam': as_sam(recs)},
                     input_fmt='sam', ranks='phylum,genus',
                     exclude=','.join(G[1:4]), sizes='$TAX/length.map', **TREE))
    rng = random.Random(510)
    recs = [(q, list(dict.fromkeys(f'{s}_{rng.randint(1, 3)}' for s in subs)))
            for q, subs in reads(501, 400, G[:40], 6)]
    out.append(_case('5-trimsub', {'aln/S1.sam': as_sam(recs),
                                   'sizes.map': size_map(G[:40], 5)},
                     input_fmt='sam', ranks='genus,species', trimsub='_',
                     sizes='sizes.map', **TREE))
    # 6. --frac
    out.append(_case('6-frac', {'aln/S1.sam': as_sam(reads(600, 300, G, 5)),
                                'aln/S2.sam': as_sam(reads(601, 100, G, 3))},
                     input_fmt='sam', ranks='genus', frac=True, scale=None,
                     digits=6, sizes='$TAX/length.map', **TREE))
    # 7. one read of 17 subjects in the middle of a file
    recs = reads(700, 300, G, 5)
    recs.insert(150, ('wide', random.Random(7).sample(G, 17)))
    # (a second file: at the default block size the first one is a single
    # block, which the wide read sends to the host tokenizer whole)
    out.append(_case('7-wide-read', {'aln/S1.sam': as_sam(recs),
                                     'aln/S2.sam': as_sam(reads(701, 90, G, 5))},
                     input_fmt='sam', ranks=','.join(RANKS3),
                     sizes='$TAX/length.map', **TREE))
    # 8. a subject without a genus (it is not in the hierarchy at all) in the
    # file's first read, `--rank genus`
    recs = reads(800, 300, G, 5)
    recs.insert(0, ('first', [G[0], 'NOGENUS1']))
    recs.insert(200, ('later', ['NOGENUS1']))
    with open(os.path.join(TAX, 'length.map')) as f:
        lengths = f.read()
    out.append(_case('8-no-genus', {'aln/S1.sam': as_sam(recs),
                                    'sizes.map': lengths + 'NOGENUS1\t5000\n'},
                     input_fmt='sam', ranks='genus', sizes='sizes.map', **TREE))
    # 9. a contributing subject that is not in the size map
    recs = reads(900, 200, G[:20], 4)
    out.append(_case('9-unsized', {'aln/S1.sam': as_sam(recs),
                                   'sizes.map': size_map(
                                       [g for g in G[:20] if g != G[2]], 9)},
                     input_fmt='sam', ranks='genus', sizes='sizes.map', **TREE))
    return out


def write_case(case, root):
    """The case's files under ``root``; returns the keyword arguments of
    `workflow` with the paths made real (all but ``output_fp``)."""
    for rel, text in case['files'].items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        opener = gzip.open if rel.endswith('.gz') else open
        with opener(path, 'wt') as f:
            f.write(text)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return os.path.join(TAX, v[5:])
        if isinstance(v, str) and (v == 'aln' or v in case['files']):
            return os.path.join(root, v)
        return v
    return {k: real(v) for k, v in case['kwargs'].items()}


def run_case(workflow, case, root):
    """Run ``workflow`` on the case: {'tables': {file name: text}} or
    {'error': [type name, message]}."""
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
