"""Inputs of the demultiplexing cases of tests/golden/vectors/demux_device.json:
regenerated from seeds (and from the bundled bowtie2 alignments), both by
tests/golden/make_demux_reference.py (which runs the reference on them) and by
tests/test_demux_host.py / tests/test_gpu_demux.py.  Only what the reference
makes of them is committed: the sample and the subjects of every read
(`read_cases`), the tables of every command (`cli_cases`).

The sample of a read is its id -- QNAME + "/1" | "/2" for a mate -- up to the
first '_' when something follows it, '' otherwise (workflow.demultiplex)."""
import hashlib
import lzma
import os
import random

import sizes_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
ALN = os.path.join(HERE, 'golden', 'data', 'align')
TREE = SC.TREE
LONG = 'L' * 40                 # a 40-byte sample name
SUBJECTS = [f'G{i:03d}' for i in range(30)]
EXCLUDED = ['G003', 'G017', 'GX99']     # (`--exclude` of the 'sam-exclude' case)


# ---- per-read cases ---------------------------------------------------------
def shapes(seed, paired):
    """Records [(QNAME, [(mate, subject or '*'), ...])] with every shape of
    name and of read the demultiplexer can meet, samples interleaved read by
    read.  ``paired``: lines carry mate bits (mate 0 lines stay in between)."""
    rng = random.Random(seed)
    shapes_of = [
        lambda i: f'plain{i}',              # no '_': sample ''
        lambda i: f'_lead{i}',              # begins with '_': sample ''
        lambda i: 'S1_',                    # ends in its first '_'
        lambda i: f'Q{i % 4}_',             # ... several such ids
        lambda i: f'S1_r{i}_x',             # two '_'
        lambda i: f'S1_r{i}',
        lambda i: f'S10_r{i}',
        lambda i: f'S1x_r{i}',
        lambda i: f'ninebytes_r{i}',        # a 9-byte sample name
        lambda i: f'{LONG}_r{i}',           # a 40-byte one
        lambda i: f'S2_{i}',
    ]
    recs = []
    for i in range(120):
        q = shapes_of[i % len(shapes_of)](i)
        k = 1 if rng.random() < 0.5 else rng.randint(2, 5)
        lines = []
        for s in rng.sample(SUBJECTS, k):
            mate = rng.choice((0, 1, 2) if i % 3 else (1, 2)) if paired else 0
            lines.append((mate, s))
            if rng.random() < 0.25:         # the same subject again
                lines.append((mate, s))
            if rng.random() < 0.15:         # an unmapped line inside the run
                lines.append((mate, '*'))
        recs.append((q, lines))
    m = (lambda j: 1 + j % 2) if paired else (lambda j: 0)
    # a read of all-unmapped lines; a sample met in unmapped reads only
    recs.insert(7, ('S1_unm', [(m(0), '*'), (m(1), '*')]))
    recs.insert(40, ('UNM_only', [(m(0), '*')]))
    # a sample whose only read hits a subject of the exclusion set
    recs.insert(55, ('EXC_only', [(m(0), 'G001'), (m(0), EXCLUDED[2])]))
    # a read of 17 subjects
    recs.insert(70, ('S10_wide', [(m(0), s) for s in SUBJECTS[:17]]))
    # the same id as one run: unpaired line and mates side by side
    if paired:
        recs.insert(90, ('S3_', [(0, 'G002'), (1, 'G004'), (2, 'G005')]))
    return recs


def nine(seed):
    """Reads of nine samples A..I, interleaved."""
    rng = random.Random(seed)
    return [(f'{"ABCDEFGHI"[i % 9]}_r{i}',
             [(0, s) for s in rng.sample(SUBJECTS, rng.randint(1, 3))])
            for i in range(90)]


def as_sam(recs):
    flag = {0: 0, 1: 65, 2: 129}
    lines = ['@HD\tVN:1.0\tSO:unsorted']
    for i, (q, rows) in enumerate(recs):
        for j, (mate, s) in enumerate(rows):
            f = flag[mate] | (4 if s == '*' else 0)
            lines.append(f'{q}\t{f}\t{s}\t{1 + 7 * i + j}\t42\t50M\t*\t0\t0'
                         '\t*\t*')
    return '\n'.join(lines) + '\n'


def _mapped(recs):
    """(query, subjects) of the formats that have no mates and no unmapped
    rows."""
    out = [(q, [s for _, s in rows if s != '*']) for q, rows in recs]
    return [(q, subs) for q, subs in out if subs]


def read_cases():
    """[{'name', 'fmt', 'text', 'exclude': names or None, 'samples':
    whitelist or None}]: a few hundred lines each."""
    flat, pair = shapes(11, False), shapes(12, True)
    out = [
        dict(name='sam-unpaired', fmt='sam', text=as_sam(flat)),
        dict(name='sam-paired', fmt='sam', text=as_sam(pair)),
        dict(name='sam-exclude', fmt='sam', text=as_sam(pair),
             exclude=EXCLUDED),
        dict(name='sam-whitelist', fmt='sam', text=as_sam(pair),
             samples=['S1', 'ninebytes', 'S3']),
        dict(name='b6o', fmt='b6o', text=SC.as_b6o(_mapped(flat))),
        dict(name='paf', fmt='paf', text=SC.as_paf(_mapped(flat))),
        dict(name='map', fmt='map', text=SC.as_map(_mapped(flat))),
        dict(name='nine-samples', fmt='sam', text=as_sam(nine(13))),
    ]
    for c in out:
        c.setdefault('exclude', None)
        c.setdefault('samples', None)
    return out


def label_reads(reads, names, allow=None):
    """[[sample or None, sorted subjects]] of reads given as (sample id,
    subject names): what the fixture holds per read.  ``names``: sample id ->
    name; ``allow``: the whitelist."""
    out = []
    for sid, subs in reads:
        name = names[sid]
        out.append([None if (allow is not None and name not in allow)
                    else name, sorted(subs)])
    return out


# ---- command-line cases -----------------------------------------------------
def mux5_text():
    """The five bundled bowtie2 alignments multiplexed into one SAM text: the
    read ids prefixed with their sample, samples in runs of ~40 reads."""
    per = []
    for i in range(1, 6):
        with lzma.open(os.path.join(ALN, 'bowtie2', f'S0{i}.sam.xz'),
                       'rt') as f:
            runs, last = [], None
            for line in f:
                if line[0] == '@':
                    continue
                q = line.split('\t', 1)[0]
                if q != last:
                    runs.append([])
                    last = q
                runs[-1].append(f'S0{i}_{line}')
            per.append(runs)
    out, pos = [], [0] * 5
    while any(p < len(r) for p, r in zip(pos, per)):
        for k in range(5):
            for run in per[k][pos[k]:pos[k] + 40]:
                out.extend(run)
            pos[k] += 40
    return ''.join(out)


def trimsub_text():
    """Reads of three samples whose subjects carry a suffix to trim."""
    G = SC.ranked_genomes()[:40]
    rng = random.Random(1800)
    recs = [(f'M{rng.randint(1, 3)}_{q}',
             list(dict.fromkeys(f'{s}_{rng.randint(1, 3)}' for s in subs)))
            for q, subs in SC.reads(1801, 390, G, 5)]
    return SC.as_sam(recs)


def cli_cases():
    """[{'name', 'text': 'mux5' | 'trimsub', 'kwargs': of workflow.workflow
    beyond input_fp / output_fp ('$TAX/...': a bundled file; 'samples': a
    list, written to a file of ids)}] -- single-file inputs, no `--demux`
    flag."""
    def case(name, text='mux5', **kw):
        kwargs = dict(input_fmt='sam', output_fmt=False)
        kwargs.update(TREE)
        kwargs.update(kw)
        return dict(name=name, text=text, kwargs=kwargs)
    return [
        case('ranks3', ranks='none,phylum,genus'),
        case('ranks3-samples', ranks='none,phylum,genus',
             samples=['S02', 'S04']),
        case('free', ranks='free'),
        case('uniq', ranks='genus', uniq=True),
        case('major', ranks='genus', major=80),
        case('above', ranks='phylum', above=True),
        case('mixed', ranks='free,genus,none', uniq=True),
        case('exclude', ranks='none,genus',
             exclude=['G000091545', 'G000015005']),
        case('trimsub', text='trimsub', ranks='genus,species', trimsub='_'),
    ]


def write_cli(case, root, text=None):
    """The case's input under ``root``; returns workflow's keyword arguments
    (all but ``output_fp``)."""
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, 'mux.sam')
    if text is None:
        text = mux5_text() if case['text'] == 'mux5' else trimsub_text()
    with open(path, 'w') as f:
        f.write(text)
    args = {}
    for k, v in case['kwargs'].items():
        if k in ('samples', 'exclude'):
            fp = os.path.join(root, f'{k}.txt')
            with open(fp, 'w') as f:
                f.write(''.join(f'{x}\n' for x in v))
            v = fp
        elif isinstance(v, list):
            v = [os.path.join(SC.TAX, x[5:]) if x.startswith('$TAX/') else x
                 for x in v]
        args[k] = v
    args['input_fp'] = path
    return args


def tables_of(out):
    """{file name: text} of what a command wrote to ``out``."""
    if os.path.isdir(out):
        return {fn: open(os.path.join(out, fn)).read()
                for fn in sorted(os.listdir(out))}
    with open(out) as f:
        return {'out': f.read()}


def digest(tables):
    """What the fixture holds of a command's tables: their text where small,
    their sha256 and size otherwise."""
    return {fn: (t if len(t) <= 1024 else
                 {'sha256': hashlib.sha256(t.encode()).hexdigest(),
                  'bytes': len(t.encode())})
            for fn, t in tables.items()}


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
