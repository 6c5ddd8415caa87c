"""Inputs of the coord-match demultiplexing cases of
tests/golden/vectors/demux_coords_device.json: regenerated from seeds (and from
the bundled bowtie2 alignments), both by
tests/golden/make_demux_coords_reference.py (which runs the reference on them)
and by tests/test_demux_coords_host.py / tests/test_gpu_demux_coords.py.  Only
what the reference makes of them is committed: the sample and the genes of
every read `ordinal_mapper` yields (`read_cases`), the tables of every command
(`cli_cases`).

`workflow.classify` demultiplexes what `ordinal_mapper` yields: a sample is met
only when one of its reads matched a gene."""
import os
import random

import demux_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
FUN = os.path.join(HERE, 'golden', 'data', 'function')
COORDS_XZ = os.path.join(FUN, 'coords.txt.xz')
LONG = D.LONG

# ---- the hand-written coordinates table --------------------------------------
# genome -> [(gene, beg, end)]; 'GN' is a genome without genes (not in the table)
GENES = {
    'GA': [(1, 101, 400), (2, 501, 700), (3, 650, 900), (4, 2100, 2000)],
    'GB': [(1, 1, 300), (2, 1000, 1500), (3, 1200, 1300)],
    'GC': [(1, 50, 5000)],
    'GD': [(1, 10, 90), (2, 100, 190), (3, 200, 290), (4, 300, 390)],
}
NO_GENES = 'GN'
# samples the reference must never see: met only in hits of aligned length 0,
# only on the genome without genes, only below the overlap threshold, only in
# unmapped lines
GENELESS = ['ZERO', 'NOGENE', 'BELOW', 'UNM']


def coords_text():
    return ''.join(f'>{g}\n' + ''.join(f'{i}\t{b}\t{e}\n' for i, b, e in genes)
                   for g, genes in GENES.items())


def gene_tables():
    """(genomes, genome_off, start0, end, gene names) as wk_set_genes takes
    them: genes sorted by start within their genome."""
    genomes = sorted(GENES)
    off, start0, end, names = [0], [], [], []
    for g in genomes:
        rows = sorted((min(b, e) - 1, max(b, e), f'{g}_{i}')
                      for i, b, e in GENES[g])
        for s, e, name in rows:
            start0.append(s)
            end.append(e)
            names.append(name)
        off.append(len(start0))
    return genomes, off, start0, end, names


# ---- per-read cases ----------------------------------------------------------
def _pos(rng, genome):
    """A POS on ``genome`` that mostly lands a 50-base hit inside a gene."""
    if genome == NO_GENES:
        return rng.randint(1, 3000)
    _, b, e = rng.choice(GENES[genome])
    lo, hi = min(b, e), max(b, e)
    return max(1, rng.randint(lo - 30, max(lo, hi - 40)))


def shapes(seed, paired):
    """Records [(QNAME, [(mate, genome or '*', POS, CIGAR), ...])] with every
    shape of name and of read the route can meet, samples interleaved read by
    read.  ``paired``: lines carry mate bits (mate 0 lines stay in between).
    Every id leads one run only: `ordinal_mapper` keys a chunk's reads by their
    id, so an id that came twice would be one read to it."""
    rng = random.Random(seed)
    shapes_of = [
        lambda i: f'plain{i}',              # no '_': sample ''
        lambda i: f'_lead{i}',              # begins with '_': sample ''
        lambda i: f'T{i}_',                 # ends in its first '_'
        lambda i: f'Q{i}_',                 # ... several such ids
        lambda i: f'S1_r{i}_x',             # two '_'
        lambda i: f'S1_r{i}',
        lambda i: f'S10_r{i}',
        lambda i: f'S1x_r{i}',
        lambda i: f'ninebytes_r{i}',        # a 9-byte sample name
        lambda i: f'{LONG}_r{i}',           # a 40-byte one
        lambda i: f'S2_{i}',
    ]
    genomes = sorted(GENES) + [NO_GENES]
    recs = []
    for i in range(110):
        q = shapes_of[i % len(shapes_of)](i)
        k = 1 if rng.random() < 0.5 else rng.randint(2, 5)
        lines = []
        for _ in range(k):
            g = rng.choice(genomes)
            mate = rng.choice((0, 1, 2) if i % 3 else (1, 2)) if paired else 0
            cigar = rng.choice(['50M', '50M', '50M', '20S30M', '25M5D25M',
                                '10H40M', '50S'])
            lines.append((mate, g, _pos(rng, g), cigar))
            if rng.random() < 0.15:         # an unmapped line inside the run
                lines.append((mate, '*', 0, '*'))
        recs.append((q, lines))
    m = (lambda j: 1 + j % 2) if paired else (lambda j: 0)
    # a read of all-unmapped lines; a sample met in unmapped lines only
    recs.insert(7, ('S1_unm', [(m(0), '*', 0, '*'), (m(1), '*', 0, '*')]))
    recs.insert(20, ('UNM_only', [(m(0), '*', 0, '*')]))
    # a sample met only in hits of aligned length 0 (inside a gene)
    recs.insert(30, ('ZERO_r1', [(m(0), 'GA', 150, '50S'),
                                 (m(1), 'GC', 600, '30I20S')]))
    recs.insert(31, ('ZERO_r2', [(m(0), 'GB', 20, '50H')]))
    # ... whose reads hit only the genome without genes
    recs.insert(45, ('NOGENE_r1', [(m(0), NO_GENES, 120, '50M'),
                                   (m(1), NO_GENES, 900, '50M')]))
    # ... whose reads overlap genes below the threshold (21 and 30 of 50)
    recs.insert(50, ('BELOW_r1', [(m(0), 'GA', 380, '50M'),
                                  (m(1), 'GB', 271, '50M')]))
    recs.insert(55, ('S1_', [(m(0), 'GD', 15, '50M')]))
    # two hits of a read on one gene
    recs.insert(60, ('S1_twice', [(m(0), 'GA', 150, '50M'),
                                  (m(0), 'GA', 220, '50M')]))
    # a read of 17 hits
    recs.insert(70, ('S10_wide', [(m(0), 'GC', 100 + 200 * j, '50M')
                                  for j in range(17)]))
    # the same id as one run: unpaired line and both mates side by side
    if paired:
        recs.insert(90, ('S3_', [(0, 'GA', 520, '50M'), (1, 'GB', 1210, '50M'),
                                 (2, 'GD', 105, '50M'), (1, 'GD', 20, '50M')]))
    return recs


def nine(seed):
    """Reads of nine samples A..I, interleaved, every one inside a gene."""
    rng = random.Random(seed)
    return [(f'{"ABCDEFGHI"[i % 9]}_r{i}',
             [(0, g, _pos(rng, g), '50M')
              for g in rng.sample(sorted(GENES), rng.randint(1, 3))] +
             [(0, 'GC', 1000 + i, '50M')])
            for i in range(90)]


def as_sam(recs):
    flag = {0: 0, 1: 65, 2: 129}
    lines = ['@HD\tVN:1.0\tSO:unsorted']
    for q, rows in recs:
        for mate, g, pos, cigar in rows:
            f = flag[mate] | (4 if g == '*' else 0)
            lines.append(f'{q}\t{f}\t{g}\t{pos}\t42\t{cigar}\t*\t0\t0\t*\t*')
    return '\n'.join(lines) + '\n'


def _mapped(recs):
    """(query, genome, POS) of the rows the formats without mates, unmapped
    rows and CIGARs can say: the 50-base hits."""
    return [(q, g, pos) for q, rows in recs for _, g, pos, cigar in rows
            if g != '*' and cigar == '50M']


def as_b6o(rows):
    return ''.join(f'{q}\t{g}\t98.5\t50\t1\t0\t1\t50\t{pos}\t{pos + 49}'
                   '\t1e-20\t95.0\n' for q, g, pos in rows)


def as_paf(rows):
    return ''.join(f'{q}\t50\t0\t50\t+\t{g}\t100000\t{pos - 1}\t{pos + 49}'
                   '\t50\t50\t60\n' for q, g, pos in rows)


WHITELIST = ['S1', 'ninebytes', 'ABSENT', 'NOGENE']     # present, present, absent, gene-less


def read_cases():
    """[{'name', 'fmt', 'text', 'samples': whitelist or None}]: 50-700 lines
    each, against `coords_text`."""
    flat, pair = shapes(21, False), shapes(22, True)
    out = [
        dict(name='sam-unpaired', fmt='sam', text=as_sam(flat)),
        dict(name='sam-paired', fmt='sam', text=as_sam(pair)),
        dict(name='sam-whitelist', fmt='sam', text=as_sam(pair),
             samples=WHITELIST),
        dict(name='b6o', fmt='b6o', text=as_b6o(_mapped(flat))),
        dict(name='paf', fmt='paf', text=as_paf(_mapped(flat))),
        dict(name='nine-samples', fmt='sam', text=as_sam(nine(23))),
    ]
    for c in out:
        c.setdefault('samples', None)
    return out


def cigar_text():
    """The nine-sample text with one CIGAR the device hands back ('*': no
    length, no hit for the reference) in its middle."""
    lines = as_sam(nine(23)).splitlines()
    half = len(lines) // 2
    q = lines[half].split('\t')[0]
    lines.insert(half, f'{q}\t0\tGA\t150\t42\t*\t*\t0\t0\t*\t*')
    return '\n'.join(lines) + '\n'


# ---- command-line cases ------------------------------------------------------
def paired_text():
    """A paired multiplexed text of three samples on the bundled genomes'
    first genes."""
    rng = random.Random(2400)
    genomes = ['G000006745', 'G000006785', 'G000006845']
    lines = []
    for i in range(300):
        q = f'P{rng.randint(1, 3)}_r{i}'
        g = rng.choice(genomes)
        pos = rng.randint(1, 20000)
        for flag in ((65, 129) if rng.random() < 0.7 else (65,)):
            lines.append(f'{q}\t{flag}\t{g}\t{pos + (flag > 100) * 180}\t42\t'
                         '100M\t=\t1\t0\t*\t*')
    return '\n'.join(lines) + '\n'


def b6o_text():
    """mux5's mapped lines as BLAST tabular rows (100 bases from POS)."""
    rows = []
    for line in D.mux5_text().splitlines():
        f = line.split('\t')
        if f[2] != '*':
            pos = int(f[3])
            rows.append(f'{f[0]}\t{f[2]}\t98.5\t100\t1\t0\t1\t100\t{pos}'
                        f'\t{pos + 99}\t1e-20\t95.0\n')
    return ''.join(rows[:4000])


TEXTS = {'mux5': D.mux5_text, 'paired': paired_text, 'b6o': b6o_text,
         'nine': lambda: as_sam(nine(23)), 'cigar': cigar_text}
_memo = {}


def text_of(kind):
    if kind not in _memo:
        _memo[kind] = TEXTS[kind]()
    return _memo[kind]


def cli_cases():
    """[{'name', 'text', 'fmt', 'kwargs': of workflow.workflow beyond input_fp
    / output_fp}] -- single-file inputs, no `--demux` flag, `--coords` the
    bundled table ('$HAND': the hand-written one)."""
    def case(name, text='mux5', fmt='sam', **kw):
        kwargs = dict(input_fmt=fmt, output_fmt=False, coords_fp='$FUN/coords.txt.xz')
        kwargs.update(kw)
        return dict(name=name, text=text, fmt=fmt, kwargs=kwargs)
    return [
        case('orf'),
        case('orf-samples', samples=['S04', 'S02', 'S09']),
        case('orf-sizes', sizes='.', scale='1k', digits=3),
        case('function', ranks='none,uniref,process',
             map_fps=['$FUN/uniref/uniref.map.xz', '$FUN/go/process.tsv.xz'],
             names_fps=["$FUN/go/name.txt.xz"], map_rank=True),
        case('overlap50', overlap=50),
        case('paired', text='paired'),
        case('b6o', text='b6o', fmt='b6o'),
        case('nine', text='nine', coords_fp='$HAND'),
        case('cigar', text='cigar', coords_fp='$HAND'),
    ]


def write_cli(case, root, text=None):
    """The case's input under ``root``; returns workflow's keyword arguments
    (all but ``output_fp``)."""
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, 'mux.' + case['fmt'])
    with open(path, 'w') as f:
        f.write(text_of(case['text']) if text is None else text)
    args = {}
    for k, v in case['kwargs'].items():
        if k == 'samples':
            fp = os.path.join(root, 'samples.txt')
            with open(fp, 'w') as f:
                f.write(''.join(f'{x}\n' for x in v))
            v = fp
        elif v == '$HAND':
            v = os.path.join(root, 'coords.txt')
            with open(v, 'w') as f:
                f.write(coords_text())
        elif isinstance(v, list):
            v = [os.path.join(FUN, x[5:]) if x.startswith('$FUN/') else x
                 for x in v]
        elif isinstance(v, str) and v.startswith('$FUN/'):
            v = os.path.join(FUN, v[5:])
        args[k] = v
    args['input_fp'] = path
    return args


tables_of = D.tables_of
digest = D.digest


def run_cli(workflow, case, root, text=None, **more):
    """Run ``workflow`` on the case; returns `digest` of its tables."""
    import contextlib
    import io
    args = write_cli(case, root, text)
    args.update(more)
    args['output_fp'] = os.path.join(root, 'out')
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(**args)
    return digest(tables_of(args['output_fp']))
