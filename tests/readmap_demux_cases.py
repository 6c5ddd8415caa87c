"""Inputs of the cases of tests/golden/vectors/readmap_demux_device.json:
hand-written multiplexed alignments whose `--outmap` text probes the read maps
under demultiplexing (csrc/wk_readmap_demux.hpp, `_run_dreads_demux`) at their
edges -- read ids that `workflow.demultiplex` cuts in every way it knows,
1, 2 and 65 samples, samples that alternate, arrive late or are dropped by
`--samples`, blocks handed to the host in the middle of a file -- rebuilt
from fixed seeds both by tests/golden/make_readmap_demux_reference.py (which
runs the reference on them) and by tests/test_gpu_readmap_demux.py /
tests/test_readmap_demux_host.py.  Only what the reference makes of them is
committed: the text of every map file (verbatim below `VERBATIM` bytes, else
`digest`), and the tables.

The hierarchy, the subjects and the job sets are those of
tests/readmap_reads_cases.py.  This module imports neither the package nor
the reference; `partition_cases` / `partition_model` are the inputs and the
plain model (a stable sort and a running sum) of the partition alone."""
import gzip
import os
import random

import numpy as np

import readmap_cases as R
import readmap_reads_cases as RR
from readmap_cases import (b6o_text, compare, digest, kept,  # noqa: F401
                           map_text, paf_text)

BLOCK = 1 << 13             # Engine.DTOK_BLOCK of the many-block cases
VERBATIM = R.VERBATIM
TILE = 512                  # reads of a tile of the partition (WK_READMAP_DEMUX_TILE)
MAX_SAMPLES = 1 << 16       # kDemuxMaxSamples
S, X, Z = RR.S, RR.X, RR.Z


# ---- read ids ---------------------------------------------------------------------
def edge_reads():
    """[(QNAME, [subjects], sample, read)]: every way `left, _, right =
    id.partition('_')`, `sample = right and left`, `read = right or left`
    can go for an id without a mate."""
    return [
        ('nounder', [S[0]], '', 'nounder'),
        ('S1_', [S[1]], '', 'S1'),              # the '_' is gone
        ('_x', [S[2]], '', 'x'),                # empty left
        ('a__b', [S[3]], 'a', '_b'),
        ('a_r1', [S[4]], 'a', 'r1'),
        ('ab_r1', [S[5]], 'ab', 'r1'),          # ids that are prefixes of each other
        ('abc_r1', [S[6], S[7]], 'abc', 'r1'),
        ('ab_r', [S[8]], 'ab', 'r'),
        ('ab_r1x', [S[9]], 'ab', 'r1x'),
        ('a_', [S[10]], '', 'a'),
        ('a_b_c', [S[11], S[12]], 'a', 'b_c'),
        ('_', [S[13]], '', ''),                 # both sides empty: a line that starts with the tab
        ('__', [S[14]], '', '_'),
    ]


def edge_runs():
    """SAM runs `readmap_cases.sam_text` takes: `S1_` unpaired and as both
    mates in one run (sample '' / read 'S1', and sample 'S1' / reads '/1',
    '/2'), next to ordinary mates of two samples."""
    runs = [
        ('S1_', [(0, S[0]), (1, S[3]), (2, S[6]), (0, S[1])], 'trailing'),
        ('S1_q', [(1, S[3]), (2, S[4])], 'both'),
        ('nounder', [(1, S[9]), (2, S[12])], 'no sample'),
        ('_x', [(2, S[15])], 'empty left'),
        ('T2_', [(1, S[18])], 'trailing, mate only'),
        ('T3_', [(0, S[21])], 'trailing, unpaired only'),
    ]
    rng = random.Random(1101)
    for i in range(90):
        runs.append((f'{rng.choice(("S1", "T2", "U"))}_k{i}',
                     [(rng.randrange(3), rng.choice(S + X + Z[:1]))
                      for _ in range(rng.randint(1, 6))], 'random'))
    return runs


def mux_reads(tag, seed, samples, n=150, pick=None):
    """``n`` reads `<sample>_<tag><i>` with the subjects of
    `readmap_reads_cases.random_reads`; ``pick(i, rng)``: the read's sample
    (default: at random)."""
    rng = random.Random(seed)
    out = []
    for i, (_, subs) in enumerate(RR.random_reads(tag, seed, n)):
        s = pick(i, rng) if pick else rng.choice(samples)
        out.append((f'{s}_{tag}{i}', subs))
    return out


def branch_mux(samples):
    """The reads that decide a branch of the assigners, dealt out in turn."""
    return [(f'{samples[i % len(samples)]}_{q}', subs)
            for i, (q, subs, _) in enumerate(RR.branch_reads())]


NAMES65 = [f'n{i:02d}' for i in range(65)]


def late_reads(n_blocks=4):
    """Many blocks of BLOCK bytes: the samples alternate every read, new ones
    keep arriving (the device's table grows block by block), and one sample
    -- `zz` -- has its only reads at the file's end."""
    rng = random.Random(1202)
    reads, pos, i = [], 0, 0
    until = (n_blocks - 0.05) * BLOCK
    while pos < until:
        blk = int(pos // BLOCK)
        pool = NAMES65[:5 + 20 * blk]
        s = pool[i % len(pool)]
        subs = rng.sample(S, rng.choice((1, 1, 2, 3)))
        q = f'{s}_w{i:05d}'
        reads.append((q, subs))
        pos += sum(len(q) + len(x) + 2 for x in subs)
        i += 1
    reads += [('zz_last1', [S[0]]), ('zz_last2', [S[3], S[4]])]
    return reads


HANDOFF_BLOCK = 1 << 16


def handoff_reads():
    """A read of 4096 subjects (all of genus Gc) of sample `K` that starts
    near the end of the first block of HANDOFF_BLOCK bytes: the second block
    holds all of it, the third what is left of the file.  The other reads are
    `readmap_reads_cases.quiet_reads`, dealt out to two samples."""
    def deal(reads):
        return [(f'{"HK"[i % 2]}_{q}', subs) for i, (q, subs) in
                enumerate(reads)]
    a, size = [], 0
    for q, subs in deal(RR.quiet_reads('h', HANDOFF_BLOCK, 808)):
        size += sum(len(q) + len(x) + 2 for x in subs)
        if size > HANDOFF_BLOCK - 600:
            break
        a.append((q, subs))
    b = deal(RR.quiet_reads('i', 40000, 809))
    return a + [(f'K_{RR.BIG_Q}', RR.BIG_SUBJECTS)] + b


FULL_AT = 8         # `demux_max_samples` of the 'full' case: block 2 brings more


# ---- commands --------------------------------------------------------------------
def cli_cases():
    """[{'name', 'files', 'kwargs', 'input': the input path (a file: demux by
    default; 'aln': a directory, demux by `--demux`), 'block', 'host_blocks':
    blocks the host takes (None: some), 'max_samples', 'gold'}]"""
    H = {'genus.map': RR._map_file(RR.genus_of()),
         'phylum.map': RR._map_file(RR.phylum_of())}
    big = dict(RR.genus_of())
    big.update({s: 'Gc' for s in RR.BIG_SUBJECTS})
    HB = dict(H, **{'genus.map': RR._map_file(big)})
    HN = dict(H, **{'names.txt': RR._map_file(RR.names_of())})

    def case(name, aln, hier=H, fmt='map', block=None, host_blocks=0,
             gold=None, single=True, max_samples=0, **kw):
        files = {f'aln/{k}': v for k, v in aln.items()}
        files.update(hier)
        kwargs = dict(input_fmt=fmt, map_rank=True,
                      map_fps=[k for k in hier if k.endswith('.map')], **kw)
        if not single:
            kwargs['demux'] = True
        return dict(name=name, files=files, kwargs=kwargs, block=block,
                    host_blocks=host_blocks, gold=gold or name,
                    input=f'aln/{next(iter(aln))}' if single else 'aln',
                    max_samples=max_samples, slot=None)
    edges = [(q, s) for q, s, _, _ in edge_reads()]
    two = edges + branch_mux(['A', 'B']) + mux_reads('r', 11, ['A', 'B'])
    ids = {'M.map': map_text(two)}
    three = branch_mux(['A', 'B', 'C']) + \
        mux_reads('t', 12, ['A', 'B', 'C'], pick=lambda i, rng: 'ABC'[i % 3])
    sam = R.sam_text(edge_runs())
    one = {'M.map': map_text(branch_mux(['only']) +
                             mux_reads('o', 13, ['only']))}
    late = {'M.map': map_text(late_reads())}
    out = [
        case('none-uniq', ids, ranks='none', uniq=True),
        case('genus-uniq', ids, ranks='genus', uniq=True),
        case('free', ids, ranks='free'),
        case('major', ids, ranks='genus', major=80),
        case('none', ids, ranks='none'),
        case('mixed', ids, ranks='none,free,genus'),
        case('unassigned', ids, ranks='genus', uniq=True, unassigned=True),
        case('plain-text', ids, ranks='none,free,genus', outmap_zip='none'),
        case('plain-text-uniq', ids, ranks='genus', uniq=True,
             outmap_zip='none'),
        case('one-sample', one, ranks='free,genus', uniq=True),
        case('one-sample-lists', one, ranks='genus'),
        case('mates', {'M.sam': sam}, fmt='sam', ranks='none', uniq=True,
             unassigned=True),
        case('mates-lists', {'M.sam': sam}, fmt='sam',
             ranks='none,free,genus'),
        case('b6o', {'M.b6o': b6o_text(two + RR.slash_reads())}, fmt='b6o',
             ranks='free'),
        case('paf', {'M.paf': paf_text(two + RR.slash_reads())}, fmt='paf',
             ranks='genus'),
        case('gz', {'M.map.gz': gzip.compress(map_text(two), mtime=0)},
             ranks='genus', uniq=True),
        case('dir', {'M.map': map_text(two), 'N.map': map_text(three)},
             single=False, ranks='free,genus', uniq=True),
        case('trim-names', {'M.map': map_text(
            [(f'{"AB"[i % 2]}_{q}', subs)
             for i, (q, subs) in enumerate(RR.trim_reads())])}, HN,
            ranks='free,genus', trimsub='_', name_as_id=True,
            names_fps=['names.txt']),
        case('exclude', {'M.sam': R.sam_text(
            [(f'{"EF"[i % 2]}_{q}', r, w)
             for i, (q, r, w) in enumerate(RR.exclude_runs())])}, fmt='sam',
            ranks='free', exclude=RR.EXCLUDED),
        case('samples-middle', {'M.map': map_text(three)}, ranks='genus',
             uniq=True, samples='A,C'),
        case('samples-middle-lists', {'M.map': map_text(three)},
             ranks='none', samples='A,C'),
        case('samples-none', {'M.map': map_text(three)}, ranks='genus',
             uniq=True, samples='Q,R'),
        case('late', late, ranks='free', block=BLOCK),
        case('late-lists', late, ranks='none,genus', block=BLOCK),
        case('handoff', {'M.map': map_text(handoff_reads())}, HB,
             ranks='free,genus', uniq=True, block=HANDOFF_BLOCK,
             host_blocks=1),
        case('full', late, ranks='free', block=BLOCK, host_blocks=None,
             max_samples=FULL_AT, gold='late'),
    ]
    return out


map_ranks = RR.map_ranks


def n_blocks(case):
    return RR.n_blocks(case)


def write_cli(case, root):
    kw = R.write_cli(case, root)
    kw['input_fp'] = os.path.join(root, case['input'])
    return kw


def run_cli(workflow, case, root):
    """Run ``workflow`` on the case: {'maps': {relative path without .gz:
    bytes}, 'tables': {file name: text}}."""
    import contextlib
    import io
    kw = write_cli(case, root)
    out, maps = os.path.join(root, 'out'), os.path.join(root, 'maps')
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(output_fp=out, outmap_dir=maps, **kw)
    got = {}
    plain = kw.get('outmap_zip') == 'none'
    for dirpath, _, files in os.walk(maps):
        for fn in files:
            fp = os.path.join(dirpath, fn)
            rel = os.path.relpath(fp, maps)
            if plain:
                assert fn.endswith('.txt'), fn
                with open(fp, 'rb') as f:
                    got[rel] = f.read()
            else:
                assert fn.endswith('.txt.gz'), fn
                with gzip.open(fp, 'rb') as f:
                    got[rel[:-3]] = f.read()
    if os.path.isdir(out):
        tables = {fn: open(os.path.join(out, fn), newline='').read()
                  for fn in sorted(os.listdir(out))}
    elif os.path.exists(out):
        with open(out, newline='') as f:
            tables = {'out': f.read()}
    else:
        tables = {}
    return {'maps': got, 'tables': tables}


# ---- the partition alone ----------------------------------------------------------
def partition_cases():
    """{name: (samp int32[n], len uint64[n])}: sizes around the tile, 17 and
    34 tiles (strips of several tiles in the column scan), all lengths 0, lengths 0 interleaved, one sample, a sample per read, ids
    sparse in 0 .. 65 535, reads without a line (-1)."""
    rng = np.random.default_rng(1303)
    out = {}

    def lens(n):
        return rng.integers(1, 300, n).astype(np.uint64)
    for n in (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        out[f'n{n}'] = (rng.integers(0, 7, n).astype(np.int32), lens(n))
    # more tiles than the 16 strips the column scan cuts them into: strips of
    # two and three tiles, the last ones shorter or empty (17 tiles: eight
    # strips of two, one of one, seven of none; 34 tiles: eleven of three, one
    # of one)
    for n in (16 * TILE + 1, 33 * TILE + 1):
        samp = rng.integers(0, 7, n).astype(np.int32)
        samp[:TILE] = 6             # (a sample the first strip holds alone)
        samp[TILE:] %= 6
        out[f'strips{n}'] = (samp, lens(n))
    n = 2 * TILE + 37
    out['zeros'] = (rng.integers(0, 5, n).astype(np.int32),
                    np.zeros(n, dtype=np.uint64))
    ln = lens(n)
    ln[::2] = 0
    out['zeros-interleaved'] = (rng.integers(0, 5, n).astype(np.int32), ln)
    out['one-sample'] = (np.full(n, 3, dtype=np.int32), lens(n))
    out['sample-per-read'] = (rng.permutation(n).astype(np.int32), lens(n))
    sparse = np.asarray([0, 1, 63, 64, 65, 1023, 1024, 40000, 65534, 65535],
                        dtype=np.int32)
    out['sparse'] = (sparse[rng.integers(0, sparse.size, n)], lens(n))
    out['alternating'] = ((np.arange(n) % 2).astype(np.int32) * 65535,
                          lens(n))
    samp = rng.integers(0, 9, n).astype(np.int32)
    samp[rng.random(n) < 0.3] = -1
    out['dropped'] = (samp, lens(n))
    out['all-dropped'] = (np.full(TILE + 5, -1, dtype=np.int32),
                          lens(TILE + 5))
    out['wide'] = (rng.integers(0, 1 << 16, 5 * TILE).astype(np.int32),
                   rng.integers(1, 1 << 40, 5 * TILE).astype(np.uint64))
    return out


def partition_model(samp, length):
    """(off, segments [D, 3], total) by `numpy.argsort(kind='stable')` and
    `cumsum`: a read without a sample has no line, length 0 and place 0."""
    samp = np.asarray(samp, dtype=np.int64)
    length = np.where(samp < 0, 0, np.asarray(length, dtype=np.uint64)
                      ).astype(np.uint64)
    order = np.argsort(samp, kind='stable')
    ends = np.cumsum(length[order], dtype=np.uint64)
    off = np.zeros(samp.size, dtype=np.uint64)
    off[order] = ends - length[order]
    off[samp < 0] = 0
    ids = np.unique(samp[samp >= 0])
    seg = np.zeros((ids.size, 3), dtype=np.uint64)
    for k, s in enumerate(ids.tolist()):
        mine = samp == s
        seg[k] = (s, off[mine].min(), length[mine].sum(dtype=np.uint64))
    return off, seg, int(length.sum(dtype=np.uint64))


# ---- what the cases promise --------------------------------------------------------
def check_inputs():
    cases = {c['name']: c for c in cli_cases()}
    assert len(cases) == len(cli_cases())
    for q, _, sample, read in edge_reads():
        left, _, right = q.partition('_')
        assert (right and left, right or left) == (sample, read), q
    assert not any('/' in q.partition('_')[0] for q, _, _ in edge_runs())
    late = cases['late']
    assert n_blocks(late) == 4
    text = late['files']['aln/M.map']
    # new samples in every block; `zz` only in the last lines of the file
    for blk in range(4):
        first_new = NAMES65[5 + 20 * (blk - 1)] if blk else NAMES65[0]
        assert text.index(f'\n{first_new}_'.encode() if blk else
                          f'{first_new}_'.encode()) // BLOCK == blk, blk
    assert len({q.partition('_')[0] for q, _ in late_reads()}) == 66
    assert text.index(b'zz_') > 3 * BLOCK
    # the 'full' case: the first block holds fewer samples than the table
    # takes, the second brings more
    in_first = {x.split(b'_')[0] for x in text[:BLOCK].split(b'\n')[:-1]}
    in_second = {x.split(b'_')[0] for x in
                 text[BLOCK:2 * BLOCK].split(b'\n')[1:-1]}
    assert len(in_first) <= FULL_AT < len(in_first | in_second)
    h = cases['handoff']['files']['aln/M.map']
    at = h.index(f'\nK_{RR.BIG_Q}\t'.encode()) + 1
    run = (RR.MAX_K + 1) * 9
    assert 0 < HANDOFF_BLOCK - at < 2000 and run < HANDOFF_BLOCK - 2000
    assert len(h) > at + HANDOFF_BLOCK + 2000 and \
        n_blocks(cases['handoff']) == 3
    for name, (samp, length) in partition_cases().items():
        assert samp.size == length.size and samp.max() < MAX_SAMPLES, name


def check_gold(gold):
    """The edges are in the reference's text (a fixture that has lost them is
    no fixture)."""
    cli = gold['cli']

    def rows(case, fn):
        text = cli[case]['maps'][fn]
        assert isinstance(text, str), (case, fn)
        return [tuple(x.split('\t', 1)) for x in text.split('\n')[:-1]]
    nu = cli['none-uniq']['maps']
    # sample '' writes `.txt`, next to the named samples
    assert {'.txt', 'a.txt', 'ab.txt', 'A.txt', 'B.txt'} <= set(nu)
    anon = dict(rows('none-uniq', '.txt'))
    assert anon['nounder'] == S[0] and anon['S1'] == S[1] and \
        anon['x'] == S[2] and anon['a'] == S[10] and anon[''] == S[13] and \
        anon['_'] == S[14] and 'S1_' not in anon
    assert dict(rows('none-uniq', 'a.txt')) == {'_b': S[3], 'r1': S[4]}
    assert [q for q, _ in rows('none-uniq', 'ab.txt')] == ['r1', 'r', 'r1x']
    # a sample all of whose reads leave no line still has its (empty) file
    assert nu['abc.txt'] == '' and cli['none']['maps']['abc.txt'] != ''
    assert dict(rows('none', 'a.txt'))['b_c'].count(':') == 2
    mates = cli['mates']['maps']
    assert [q for q, _ in rows('mates', 'S1.txt')][:2] == ['/1', '/2']
    assert rows('mates', '.txt')[0][0] == 'S1' and \
        ('nounder/1' in dict(rows('mates', '.txt'))) and \
        ('x/2' in dict(rows('mates', '.txt')))
    assert dict(rows('mates', 'T2.txt')).get('/1') == S[18] and \
        dict(rows('mates', '.txt')).get('T3') == S[21]
    assert not any('/' in fn[:-4] for fn in mates)
    assert set(cli['plain-text']['maps']) >= {
        'none/A.txt', 'free/A.txt', 'genus/.txt'}
    assert set(cli['one-sample']['maps']) == {'free/only.txt',
                                              'genus/only.txt'}
    sm = cli['samples-middle']['maps']
    assert set(sm) == {'A.txt', 'C.txt'}
    assert cli['samples-none']['maps'] == {}
    late = cli['late']['maps']
    assert len(late) == 66 and late['zz.txt'].count('\n') >= 1
    hf = cli['handoff']['maps']
    assert any(f'{RR.BIG_Q}\tGc\n' in t for fn, t in hf.items()
               if fn.startswith('genus/'))
    assert set(cli['dir']['maps']) >= {'free/A.txt', 'free/C.txt', 'genus/.txt'}
