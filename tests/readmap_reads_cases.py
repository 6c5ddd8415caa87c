"""Inputs of the cases of tests/golden/vectors/readmap_reads_device.json:
hand-written alignments and hierarchies whose `--outmap` text under `--rank
free`, `--uniq`, `--above` and `--major` probes the device writer of
whole-read assignments (csrc/wk_readmap_reads.hpp) at its edges -- `cli_cases`
for whole commands, `block_cases` for single blocks through
`Context.dtok_readmap_reads` -- rebuilt from fixed seeds both by
tests/golden/make_readmap_reads_reference.py (which runs the reference on
them) and by tests/test_gpu_readmap_reads.py /
tests/test_readmap_reads_host.py.  Only what the reference makes of them is
committed: the text of every map file (verbatim below `VERBATIM` bytes, else
`digest`), and the tables.

The hierarchy is two map files: `genus.map` (subject -> genus) and
`phylum.map` (genus -> phylum, and two subjects straight to a phylum: they
have no ancestor at rank genus).  This module imports neither the package nor
the reference; `assign` is a plain model of the assigners for the tests that
feed the formatters directly."""
import gzip
import os
import random

import readmap_cases as R
from readmap_cases import (b6o_text, compare, digest, kept,  # noqa: F401
                           map_text, paf_text, reads_of)

BLOCK = 1 << 13             # Engine.DTOK_BLOCK of the many-block cases
VERBATIM = R.VERBATIM
MAX_K = 4095                # subjects of a read the device takes (WK_MAX_K)

GENERA = ['g', 'Ga', 'Gb', 'Gb1', 'Gc', 'Gd', 'Ge', 'Gf', 'Gg', 'Gh']
S = [f'S{i:02d}' for i in range(30)]            # subject i -> genus i // 3
X = ['X0', 'X1']                                # -> phylum P1, no genus
Z = ['Z0', 'Z1', 'z']                           # not in the tree
PHYLA = ['p', 'P1', 'P2']
LONG_ID = 'L' * 210                             # a subject whose id is 210 bytes (genus Gh)


def genus_of():
    m = {s: GENERA[i // 3] for i, s in enumerate(S)}
    m[LONG_ID] = 'Gh'
    return m


def phylum_of():
    m = {g: PHYLA[i % 3] for i, g in enumerate(GENERA)}
    m.update({x: 'P1' for x in X})
    return m


def names_of():
    """`g` has a name of one byte, `Ga` one of 200, `P1` one with blanks; `Gb`,
    `p` and the subjects but one have none."""
    return {'g': 'n', 'Ga': 'N' * 200, 'Gb1': 'b one', 'Gc': 'c c',
            'Gd': 'Gd name', 'P1': 'phylum  one', 'P2': 'two', 'S00': 'zero'}


def _map_file(d):
    return ''.join(f'{k}\t{v}\n' for k, v in d.items()).encode()


# ---- reads ----------------------------------------------------------------------
def branch_reads():
    """[(QNAME, [subjects], what)]: the reads that decide a branch."""
    return [
        ('one', [S[0]], 'one subject'),
        ('same', [S[3], S[4], S[5]], 'several subjects, one genus'),
        ('genera', [S[3], S[12]], 'two genera of one phylum (i // 3 = 1, 4)'),
        ('root', [S[0], S[3], S[6]], 'three phyla: the LCA is the root'),
        ('notree', [Z[0]], 'a subject that is not in the tree'),
        ('notree2', [Z[1], S[9]], '... next to one that is'),
        ('short', [Z[2]], 'a one-byte subject outside the tree'),
        ('nogenus', [X[0]], 'no ancestor at rank genus'),
        ('nogenus2', [X[0], X[1]], 'two of them'),
        ('nogenus3', [X[1], S[4]], '... next to a genus of the same phylum'),
        ('major-none', [X[0], X[1], Z[0], Z[1], S[6]], 'majority: none wins'),
        ('major-at', [S[27], S[28], S[29], LONG_ID, S[0]],
         'majority: 4 of 5 = 80 % exactly'),
        ('major-below', [S[6], S[7], S[8], S[21], S[22]], '3 of 5'),
        ('major-all', [S[24], S[25]], 'all of them'),
        ('long', [LONG_ID], 'a subject id of 210 bytes'),
        ('q', [S[1]], 'a QNAME of one byte'),
        ('ab', [S[2]], 'QNAMEs that are prefixes of each other'),
        ('abc', [S[2], S[1]], ''),
        ('abcd', [S[27]], ''),
        ('a', [S[28], Z[0]], ''),
        ('g-one', [S[0], S[1], S[2]], 'the genus whose id is one byte'),
        ('gb', [S[6]], 'a genus without a name'),
        ('gd', [S[15], S[16]], 'a genus with one'),
    ]


def random_reads(tag, seed, n=150, pool=None):
    rng = random.Random(seed)
    pool = pool or (S + X + Z[:2])
    out = []
    for i in range(n):
        k = rng.choice((1, 1, 1, 2, 2, 3, 5))
        if rng.random() < 0.5:      # (neighbours: mostly one genus or one phylum)
            at = rng.randrange(len(S) - 6)
            subs = rng.sample(S[at:at + 6], min(k, 6))
        else:
            subs = rng.sample(pool, k)
        out.append((f'{tag}{i}', subs))
    return out


def plain_reads(seed=1):
    return [(q, s) for q, s, _ in branch_reads()] + random_reads('r', seed)


def slash_reads():
    """Ids ending in /1 and /2 in the formats that know no mates."""
    return [('m/1', [S[0]]), ('m/2', [S[1], S[2]]), ('m', [S[3]]),
            ('m/1', [S[4]]), ('n/2', [S[5], S[20]]), ('n/1', [S[6]])]


def mate_runs():
    """[(QNAME, [(mate, subject) | None, ...], what)] as
    `readmap_cases.sam_text` takes them."""
    runs = [
        ('u', [(0, S[0]), (0, S[1])], 'unpaired'),
        ('f', [(1, S[3]), (1, S[4])], 'only1'),
        ('s', [(2, S[6]), (2, S[9])], 'only2'),
        ('b', [(1, S[0]), (2, S[12]), (1, S[1]), (2, S[13])], 'both'),
        ('t', [(0, S[15]), (2, S[16]), (1, S[17]), (0, S[15])], 'all3'),
        ('w', [(2, S[18]), (1, S[3]), (1, S[21])], '2before1'),
        ('e', [(1, S[0]), None, (2, Z[0])], 'star'),
        ('x1', [(1, X[0]), (2, S[4]), (2, X[1])], 'nogenus'),
    ]
    rng = random.Random(505)
    for i in range(80):
        runs.append((f'k{i}', [(rng.randrange(3), rng.choice(S + X + Z[:1]))
                               for _ in range(rng.randint(1, 6))], 'random'))
    return runs


EXCLUDED = 'S29'


def exclude_runs():
    """The hit on the excluded subject sits on the second mate: the whole run
    goes (align.py:47-115)."""
    return [('keep', [(1, S[0]), (2, S[1])], ''),
            ('drop', [(1, S[3]), (2, EXCLUDED), (1, S[4])], 'second mate'),
            ('keep2', [(0, S[6])], ''),
            ('drop2', [(0, S[7]), (0, EXCLUDED)], 'unpaired')] + \
        [(q, r, w) for q, r, w in mate_runs()[8:40]]


def trim_reads():
    """Subjects `<genome>_<gene>`: --trim-sub _ leaves the genome."""
    rng = random.Random(606)
    out = []
    for q, subs in plain_reads(2)[:200]:
        out.append((q, [f'{s}_{rng.randrange(4)}' for s in subs] +
                    ([f'{subs[0]}_9'] if rng.random() < 0.3 else [])))
    return out


# many blocks: subjects outside the tree (features >= n_nodes) and subjects of
# the tree keep appearing until the last block
GROW_N = 4
GROW_SHORT = 2            # blocks of the shorter file of the `--subok` case


def grow_reads(n_blocks=GROW_N):
    rng = random.Random(707)
    reads, pos, i = [], 0, 0
    until = (n_blocks - 0.05) * BLOCK
    while pos < until:
        blk = int(pos // BLOCK)
        fresh = [f'N{blk:02d}_{k}' for k in range(3)]      # not in the tree
        late = S[:3 + min(blk * 3, 27)]                    # the tree's, block by block
        subs = rng.sample(late, rng.choice((1, 1, 1, 2))) if i % 3 \
            else [rng.choice(fresh)]
        if i % 13 == 0:
            subs = [rng.choice(fresh), rng.choice(late)]
        q = f'w{i:05d}'
        reads.append((q, subs))
        pos += sum(len(q) + len(s) + 2 for s in subs)
        i += 1
    return reads


BIG_Q = 'Q'
BIG_SUBJECTS = [f'b{i:03x}' for i in range(MAX_K + 1)]


HANDOFF_BLOCK = 1 << 15


def quiet_reads(tag, size, seed):
    """Reads whose text is ``size`` bytes at least: most have a subject of
    each phylum (no line under `--uniq` or `free`: the LCA is the root), every
    eighth has one subject."""
    rng = random.Random(seed)
    reads, pos, i = [], 0, 0
    while pos < size:
        subs = [rng.choice(S)] if i % 8 == 0 else \
            [rng.choice(S[0:3]), rng.choice(S[3:6]), rng.choice(S[6:9])]
        q = f'{tag}{i:04d}'
        reads.append((q, subs))
        pos += sum(len(q) + len(s) + 2 for s in subs)
        i += 1
    return reads


def handoff_reads():
    """A read of 4096 subjects (all of genus Gc) that starts near the end of
    the first block of HANDOFF_BLOCK bytes: the second block holds all of it,
    the third what is left of the file."""
    a = quiet_reads('h', HANDOFF_BLOCK - 1200, 808)
    b = quiet_reads('i', 12000, 809)
    return a + [(BIG_Q, BIG_SUBJECTS)] + b


# ---- commands --------------------------------------------------------------------
JOB_SETS = {
    'none-uniq': dict(ranks='none', uniq=True),
    'free': dict(ranks='free'),
    'free-subok': dict(ranks='free', subok=True),
    'genus-uniq': dict(ranks='genus', uniq=True),
    'genus-above': dict(ranks='genus', above=True),
    'genus-major': dict(ranks='genus', major=80),
    'three-uniq': dict(ranks='free,phylum,genus', uniq=True),
}


def cli_cases():
    """[{'name', 'files': {relative path: bytes}, 'kwargs', 'block', 'slot',
    'host_blocks': blocks the host takes, 'gold': the case whose reference
    text is this one's too (the same command on the same files)}]"""
    genus = genus_of()
    H = {'genus.map': _map_file(genus), 'phylum.map': _map_file(phylum_of())}
    HB = dict(H)
    big = dict(genus)
    big.update({s: 'Gc' for s in BIG_SUBJECTS})
    HB['genus.map'] = _map_file(big)
    HN = dict(H)
    HN['names.txt'] = _map_file(names_of())

    def case(name, aln, hier=H, fmt='map', block=None, slot=None,
             host_blocks=0, gold=None, **kw):
        files = {f'aln/{k}': v for k, v in aln.items()}
        files.update(hier)
        kwargs = dict(input_fmt=fmt, map_rank=True,
                      map_fps=[k for k in hier if k.endswith('.map')], **kw)
        return dict(name=name, files=files, kwargs=kwargs, block=block,
                    slot=slot, host_blocks=host_blocks, gold=gold or name)
    plain = {'S.map': map_text(plain_reads())}
    out = []
    for key, js in JOB_SETS.items():
        out.append(case(key, plain, **js))
        out.append(case(key + '-unassigned', plain, unassigned=True, **js))
    sam = R.sam_text(mate_runs())
    grow = {'S.map': map_text(grow_reads())}
    out += [
        case('names', plain, HN, ranks='free,genus', uniq=True,
             name_as_id=True, names_fps=['names.txt']),
        case('names-none', plain, HN, ranks='none', uniq=True, unassigned=True,
             name_as_id=True, names_fps=['names.txt']),
        case('mates', {'S.sam': sam}, fmt='sam', ranks='free,genus',
             uniq=True),
        case('mates-none', {'S.sam': sam}, fmt='sam', ranks='none', uniq=True,
             unassigned=True),
        case('formats', {'B.b6o': b6o_text(plain_reads(3) + slash_reads()),
                         'P.paf': paf_text(plain_reads(4) + slash_reads()),
                         'M.map': map_text(slash_reads())},
             fmt=None, ranks='free'),
        case('gz', {'S.map.gz': gzip.compress(map_text(plain_reads(5)),
                                              mtime=0)},
             ranks='genus', above=True),
        case('sam-gz', {'S.sam.gz': gzip.compress(sam, mtime=0)}, fmt='sam',
             ranks='genus', major=80),
        case('trim', {'S.map': map_text(trim_reads())}, ranks='free,genus',
             uniq=True, trimsub='_'),
        case('exclude', {'S.sam': R.sam_text(exclude_runs())}, fmt='sam',
             ranks='free', exclude=EXCLUDED),
        case('plain-text', plain, ranks='genus', uniq=True,
             outmap_zip='none'),
        case('grow-none', grow, ranks='none', uniq=True, block=BLOCK),
        case('grow-free-subok', {'S.map': map_text(grow_reads(GROW_SHORT))},
             ranks='free', subok=True, block=BLOCK),
        case('grow-small-slot', grow, ranks='none', uniq=True, block=BLOCK,
             slot=4096, gold='grow-none'),
        case('handoff', {'S.map': map_text(handoff_reads())}, HB,
             ranks='free,genus', uniq=True, block=HANDOFF_BLOCK,
             host_blocks=1),
    ]
    return out


def map_ranks(case):
    """The ranks of the case's command."""
    return case['kwargs']['ranks'].split(',')


def n_blocks(case):
    """Blocks the device text route cuts the case's files into (plain files
    that are not SAM: `block` bytes at a time), or None where the case does
    not say."""
    if not case['block']:
        return None
    total = 0
    for k, v in case['files'].items():
        if k.startswith('aln/'):
            total += -(-len(v) // case['block'])
    return total


def write_cli(case, root):
    return R.write_cli(case, root)


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
    else:
        with open(out, newline='') as f:
            tables = {'out': f.read()}
    return {'maps': got, 'tables': tables}


# ---- single blocks ---------------------------------------------------------------
BLOCK_SIZES = (1, 255, 256, 257, 65537)
BLOCK_SUBJECTS = S + [LONG_ID, 'z']
_PERIOD = 96


def block_reads(n, kind='all'):
    """``n`` reads of the block cases.  'all': one subject each (assigned
    under `--rank none --uniq`); 'nobody': two subjects each (no read is
    assigned); 'last': like 'nobody' but for the last read."""
    reads = []
    for i in range(n):
        q = 'abcdefgh'[i % 8] * (1 + i % 3)
        s = BLOCK_SUBJECTS[i % len(BLOCK_SUBJECTS)]
        two = kind == 'nobody' or (kind == 'last' and i < n - 1)
        reads.append((q, [s, BLOCK_SUBJECTS[(i + 1) % len(BLOCK_SUBJECTS)]]
                      if two else [s]))
    return reads


def block_text(n, kind='all'):
    if kind == 'all' and n > _PERIOD:
        period = map_text(block_reads(_PERIOD))
        return period * (n // _PERIOD) + map_text(block_reads(n % _PERIOD))
    return map_text(block_reads(n, kind))


def block_map_text(n, kind='all', unassigned=False):
    """The map of the block under `--rank none --uniq`, by the plain model: a
    read of one subject shows it, any other has no line (or `Unassigned`)."""
    def rows(reads):
        out = []
        for q, s in reads:
            if len(s) == 1:
                out.append(f'{q}\t{s[0]}\n')
            elif unassigned:
                out.append(f'{q}\tUnassigned\n')
        return ''.join(out).encode()
    if kind == 'all' and n > _PERIOD:
        return rows(block_reads(_PERIOD)) * (n // _PERIOD) + \
            rows(block_reads(n % _PERIOD))
    return rows(block_reads(n, kind))


def block_cases():
    return {f'n{n}': n for n in BLOCK_SIZES}


# ---- a plain model of the assigners ---------------------------------------------
def _pairs(text):
    return dict(x.split('\t') for x in text.decode().split('\n')[:-1])


def hierarchy_of(case):
    """(tree: {child: parent}, rankdic: {taxon: rank}) of the case's map
    files."""
    genus = _pairs(case['files']['genus.map'])
    phylum = _pairs(case['files']['phylum.map'])
    tree = dict(genus)
    tree.update(phylum)
    rankdic = {t: 'genus' for t in genus.values()}
    rankdic.update({t: 'phylum' for t in phylum.values()})
    return tree, rankdic


def _lineage(s, tree):
    """[s, parent, ...] of a node of the tree, [] outside it (the crowns hang
    under a root of their own, which stands for "nothing")."""
    if s not in tree:
        return []
    out = [s]
    while out[-1] in tree:
        out.append(tree[out[-1]])
    return out


def _lca(nodes, tree):
    lins = [_lineage(x, tree) or ([x] if x in tree.values() else [])
            for x in nodes]
    if not all(lins):
        return None
    common = None
    for t in lins[0][::-1]:     # from the top: the last shared one is the LCA
        if all(t in lin for lin in lins[1:]):
            common = t
        else:
            break
    return common


def assign(subs, rank, hier, uniq=False, above=False, major=None,
           subok=False):
    """What classify.assign_none / assign_free / assign_rank
    (classify.py:32-127) give for the distinct subjects ``subs`` when no list
    can come back: a feature id or None."""
    tree, rankdic = hier
    subs = list(dict.fromkeys(subs))
    if rank == 'none':
        return subs[0] if len(subs) == 1 else None
    if rank == 'free':
        if len(subs) == 1:
            return subs[0] if subok else tree.get(subs[0])
        return _lca(subs, tree)

    def find_rank(x):
        while x is not None and rankdic.get(x) != rank:
            x = tree.get(x)
        return x
    taxa = [find_rank(s) for s in subs]
    tset = set(taxa)
    if len(tset) == 1:
        return taxa[0]
    if major:
        best = max(tset, key=taxa.count)
        return best if taxa.count(best) >= len(taxa) * major / 100 else None
    if above and None not in tset:
        return _lca(sorted(tset), tree)
    return None


# ---- what the cases promise --------------------------------------------------------
def check_inputs():
    cases = {c['name']: c for c in cli_cases()}
    assert len(cases) == len(cli_cases())
    for key in JOB_SETS:
        assert key in cases and key + '-unassigned' in cases
    kinds = {w for _, _, w in mate_runs()}
    assert {'unpaired', 'only1', 'only2', 'both', 'all3'} <= kinds
    reads = dict((q, s) for q, s, _ in branch_reads())
    assert len(reads['one']) == 1 and len(set(reads['major-at'])) == 5
    g = genus_of()
    assert [g.get(s) for s in reads['major-at']].count('Gh') == 4
    assert n_blocks(cases['grow-none']) == GROW_N
    text = cases['grow-none']['files']['aln/S.map']
    for blk in range(GROW_N):
        at = text.index(f'\tN{blk:02d}_'.encode())
        assert at // BLOCK == blk, (blk, at // BLOCK)
    # the 4 KB-slot variant: the lines of every block, the short last one
    # too, are more than a slot holds (a block's cut moves by a run at most)
    pos, per = 0, [0] * GROW_N
    for q, subs in grow_reads():
        if len(subs) == 1:
            per[pos // BLOCK] += len(q) + len(subs[0]) + 2
        pos += sum(len(q) + len(x) + 2 for x in subs)
    assert min(per) > 4096 + 256, per
    # the hand-off: the big read starts inside the first block, the second
    # block holds all of it, and a third one is left
    h = cases['handoff']['files']['aln/S.map']
    assert len(dict(reads_of(h, 'map'))[BIG_Q]) == MAX_K + 1
    at = h.index(f'\n{BIG_Q}\t'.encode()) + 1
    run = (MAX_K + 1) * 7
    assert 0 < HANDOFF_BLOCK - at < 2000 and run < HANDOFF_BLOCK - 2000
    assert len(h) > 2 * HANDOFF_BLOCK + 2000 and n_blocks(cases['handoff']) == 3
    for n in (1, 255, 257):
        assert reads_of(block_text(n), 'map') == block_reads(n)
        assert len(reads_of(block_text(n, 'nobody'), 'map')) == n
    assert block_map_text(300, 'nobody') == b'' and \
        block_map_text(300, 'last').count(b'\n') == 1
    assert all(a[0] != b[0] for a, b in zip(block_reads(_PERIOD),
                                            block_reads(_PERIOD + 1)[1:]))


def check_gold(gold):
    """The edges are in the reference's text (a fixture that has lost them is
    no fixture)."""
    cli = gold['cli']

    def rows(case, prefix=''):
        (text,) = [v for k, v in cli[case]['maps'].items()
                   if k.startswith(prefix)]
        assert isinstance(text, str), (case, prefix)
        return dict(x.split('\t') for x in text.split('\n')[:-1])
    for key in JOB_SETS:
        assert set(cli[key]['maps']) == set(cli[key + '-unassigned']['maps'])
    assert set(cli['three-uniq']['maps']) == {
        'free/S.txt', 'phylum/S.txt', 'genus/S.txt'}
    none = rows('none-uniq')
    assert none['one'] == 'S00' and none['notree'] == 'Z0' and \
        none['short'] == 'z' and none['long'] == LONG_ID and \
        'same' not in none and 'root' not in none
    free = rows('free')
    assert free['one'] == 'g' and free['same'] == 'Ga' and \
        free['genera'] == 'P1' and 'root' not in free and \
        'notree' not in free and 'notree2' not in free and \
        free['nogenus'] == 'P1' and free['nogenus3'] == 'P1'
    assert rows('free-subok')['one'] == 'S00' and \
        rows('free-subok')['notree'] == 'Z0' and \
        rows('free-subok')['same'] == 'Ga'
    gu = rows('genus-uniq')
    assert gu['same'] == 'Ga' and 'genera' not in gu and \
        'nogenus' not in gu and gu['g-one'] == 'g' and 'notree2' not in gu
    ga = rows('genus-above')
    assert ga['same'] == 'Ga' and ga['genera'] == 'P1' and \
        'root' not in ga and 'nogenus' not in ga
    gm = rows('genus-major')
    assert gm['major-at'] == 'Gh' and 'major-below' not in gm and \
        'major-none' not in gm and gm['major-all'] == 'Gg'
    un = rows('genus-major-unassigned')
    assert un['major-none'] == 'Unassigned' == un['major-below'] and \
        un['major-at'] == 'Gh'
    assert rows('none-uniq-unassigned')['same'] == 'Unassigned'
    for q in ('q', 'a', 'ab', 'abc', 'abcd'):
        assert q in rows('free-unassigned'), q
    nm = rows('names', 'genus')
    assert nm['g-one'] == 'n' and nm['same'] == 'N' * 200 and \
        'Gb' in nm.values() and 'Gd name' in nm.values()
    assert rows('names', 'free')['genera'] == 'phylum  one'
    nn = rows('names-none')
    assert nn['one'] == 'zero' and nn['q'] == 'S01' and \
        nn['same'] == 'Unassigned'
    mates = rows('mates-none')
    for q in ('u', 'f/1', 's/2', 'b/1', 'b/2', 't', 't/1', 't/2', 'w/1', 'w/2',
              'e/1', 'e/2'):
        assert q in mates, q
    for q in ('u/1', 'f', 'f/2', 's', 's/1', 'b', 'w'):
        assert q not in mates, q
    order = list(mates)
    assert order.index('w/1') + 1 == order.index('w/2') and \
        order.index('t') + 2 == order.index('t/2')
    assert mates['e/2'] == 'Z0' and mates['t/1'] == 'S17' and \
        mates['u'] == 'Unassigned'
    mg = rows('mates', 'genus')
    assert mg['f/1'] == 'Ga' and 'x1/1' not in mg
    for fn in ('B.txt', 'P.txt', 'M.txt'):
        text = cli['formats']['maps'][fn]
        assert 'm/1\t' in text and 'm/2\t' in text and 'n/1\t' in text
    ex = rows('exclude')
    assert 'keep/1' in ex and 'keep2' in ex and \
        not any(q.startswith('drop') for q in ex)
    assert set(cli['plain-text']['maps']) == {'S.txt'}
    tr = rows('trim', 'genus')
    assert tr['one'] == 'g'
    gn = rows('grow-none')
    for blk in range(GROW_N):
        assert any(v.startswith(f'N{blk:02d}_') for v in gn.values()), blk
    assert any(v.startswith(f'N{GROW_SHORT - 1:02d}_')
               for v in rows('grow-free-subok').values())
    # (no text of the 4 KB-slot variant fits its slot)
    assert len(cli['grow-none']['maps']['S.txt']) > GROW_N * 4096
    hf = cli['handoff']['maps']
    assert f'\n{BIG_Q}\tGc\n' in hf['genus/S.txt'] and \
        f'\n{BIG_Q}\tGc\n' in hf['free/S.txt']
    for name, n in block_cases().items():
        assert gold['blocks'][name]['lines'] == n
