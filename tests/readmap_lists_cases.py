"""Inputs of the cases of tests/golden/vectors/readmap_lists_device.json:
hand-written alignments and hierarchies whose `--outmap` text holds taxon lists
(`query <tab> taxon:count <tab> ...`) and probes the device formatter of
csrc/wk_readmap_lists.hpp at its edges -- `cli_cases` for whole commands,
`block_cases` for single blocks through `Context.dtok_readmap_lists` -- rebuilt
from fixed seeds both by tests/golden/make_readmap_lists_reference.py (which
runs the reference on them) and by tests/test_gpu_readmap_lists.py /
tests/test_readmap_lists_host.py.  Only what the reference makes of them is
committed: per map file its text (verbatim below `VERBATIM` bytes, else
`digest`), how many of its lines are lists, and the ends of the lines of
`PROBES`; the tables.

The hierarchy, the subjects and most reads are those of
tests/readmap_reads_cases.py (imported, not edited): genera `g`, `Ga`, `Gb`,
`Gb1`, ... (ids that are prefixes of each other; `g` is the shortest id and
the last in byte order), names whose order is not their ids' (`Ga` -> `NNN...`,
`Gb1` -> `b one`, `Gb` has none), subjects without a genus (`X0`, `X1`) and
outside the tree (`Z0`, `Z1`, `z`).  The `tiers` case adds 4096 subjects `tXXX`
over 97 genera `H00`..`H96` and 4095 subjects `bXXX` of genus `Gc`.

`COMMANDS` are the cases the list route takes; at least a quarter of the map
lines of each are lists (`check_gold`).  `--rank none,genus --uniq` returns no
list and is R1m's: it stands among the `NEIGHBOURS`, next to its twin without
`--uniq`, which is a command case.  The largest count a list can hold is 4094:
a read all of whose 4095 subjects share one feature is no list."""
import gzip
import random

import readmap_cases as R
import readmap_reads_cases as T0
from readmap_cases import (b6o_text, compare, digest, kept,  # noqa: F401
                           map_text, paf_text, reads_of)
from readmap_reads_cases import (BIG_Q, BIG_SUBJECTS, EXCLUDED,  # noqa: F401
                                 GENERA, HANDOFF_BLOCK, LONG_ID, MAX_K, S, X,
                                 Z, _map_file, _pairs, genus_of, hierarchy_of,
                                 map_ranks, n_blocks, names_of, phylum_of,
                                 run_cli, write_cli)

BLOCK = 1 << 13             # Engine.DTOK_BLOCK of the many-block cases
SMALL_SLOT = 1024           # a map ring's slot no block's text fits
VERBATIM = R.VERBATIM
TIERS = (2, 16, 17, 63, 64, 65, MAX_K)      # subjects of a read at the edges of the wave kernel's tiers
DIGITS = (9, 10, 99, 100, 999, 1000, MAX_K - 1)
TS = [f't{i:03x}' for i in range(MAX_K + 1)]        # -> genus H{(i * i + i // 97) % 97}
BS = [f'b{i:03x}' for i in range(MAX_K)]            # -> genus Gc
N_H = 97


def tier_genus(i):
    return f'H{(i * i + i // N_H) % N_H:02d}'


# ---- reads ----------------------------------------------------------------------
def edge_reads():
    """[(QNAME, [subjects], what)]: the reads that decide an order, a count or
    a dropped subject."""
    return [
        ('tie', [S[12], S[3]], 'Gc and Ga once each: the id decides'),
        ('prefix', [S[9], S[6]], 'Gb1 and Gb: the prefix comes first'),
        ('shortest-last', [S[0], S[27], S[3]], 'g, Gh, Ga: bytes, not lengths'),
        ('count-first', [S[12], S[13], S[3]], 'Gc:2 before Ga:1'),
        ('count-tie', [S[12], S[13], S[3], S[4], S[6]], 'Ga:2 Gc:2 Gb:1'),
        ('drop', [X[0], Z[0], S[4]], 'no genus, no node, Ga: the list is Ga:1'),
        ('drop2', [X[1], S[4], S[12], Z[1]], 'Ga:1 Gc:1 after two are dropped'),
        ('nogenus-only', [X[0], X[1]], 'two subjects, no genus: no list, no line'),
        ('long', [LONG_ID, S[0]], 'an id of 210 bytes in a list'),
        ('names', [S[3], S[6], S[9]], 'Ga, Gb, Gb1: names in another order than ids'),
        ('named-subject', [S[0], S[1]], 'S00 has a name, S01 none'),
        ('one', [S[0]], 'one subject: no list'),
        ('same', [S[3], S[4], S[5]], 'one genus: a list at none only'),
        ('q', [S[1], S[29]], 'a QNAME of one byte'),
    ]


def list_reads(tag, seed, n=110, pool=None):
    """Reads of which most are split over several genera."""
    rng = random.Random(seed)
    pool = pool or (S + X + Z[:2])
    out = []
    for i in range(n):
        k = rng.choice((1, 2, 2, 3, 3, 4, 5, 8))
        out.append((f'{tag}{i}', rng.sample(pool, k)))
    return out


def plain_reads(seed=1):
    return [(q, s) for q, s, _ in edge_reads()] + list_reads('r', seed)


def tree_reads():
    """Reads all of whose subjects have a genus (a subject without one hands
    R1's block to the host)."""
    ok = set(S) | {LONG_ID}
    return [(q, s) for q, s, _ in edge_reads() if set(s) <= ok] + \
        list_reads('p', 7, pool=S)


def orf_reads(seed=2):
    """Subjects `<genome>_<gene>` (ORF ids): `--trim-sub _` leaves the genome.
    Two genes of one genome in a read are one subject."""
    rng = random.Random(606 + seed)
    out = [('twice', [f'{S[3]}_1', f'{S[3]}_2', f'{S[12]}_0'])]
    for q, subs in plain_reads(seed):
        out.append((q, [f'{s}_{rng.randrange(4)}' for s in subs] +
                    ([f'{subs[0]}_9'] if rng.random() < 0.3 else [])))
    return out


def mate_runs():
    """`readmap_reads_cases.mate_runs` (every mate pattern) and runs whose
    mates are split over several genera."""
    rng = random.Random(515)
    runs = list(T0.mate_runs())
    for i in range(60):
        runs.append((f'j{i}', [(rng.randrange(3), rng.choice(S + X))
                               for _ in range(rng.randint(3, 9))], 'lists'))
    return runs


def exclude_runs():
    rng = random.Random(525)
    runs = list(T0.exclude_runs())
    for i in range(60):
        hit = [(rng.randrange(3), rng.choice(S[:29])) for _ in
               range(rng.randint(2, 7))]
        if i % 10 == 0:
            hit.insert(1, (hit[0][0], EXCLUDED))
        runs.append((f'y{i}', hit, 'lists'))
    return runs


GROW_N = 4


def grow_reads(n_blocks=GROW_N):
    """Many blocks: subjects outside the tree (features >= n_nodes) and
    subjects of the tree keep appearing until the last block, mostly in
    lists."""
    rng = random.Random(717)
    reads, pos, i = [], 0, 0
    until = (n_blocks - 0.05) * BLOCK
    while pos < until:
        blk = int(pos // BLOCK)
        fresh = [f'N{blk:02d}_{k}' for k in range(3)]      # not in the tree
        late = S[:3 + min(blk * 9, 27)]                    # the tree's, block by block
        if i % 13 == 0:
            subs = [rng.choice(late)]
        elif i % 3:
            subs = rng.sample(late, rng.choice((2, 3)))
        else:
            subs = [rng.choice(fresh), rng.choice(late)]
        q = f'w{i:05d}'
        reads.append((q, subs))
        pos += sum(len(q) + len(s) + 2 for s in subs)
        i += 1
    return reads


def tier_reads():
    """Reads of 2 .. 4095 distinct subjects over up to 97 genera, and reads
    whose largest count has 1, 2, 3 and 4 digits."""
    out = [(f'tier{n}', TS[n:2 * n] if 2 * n <= len(TS) else TS[:n])
           for n in TIERS]
    out += [(f'low{n}', TS[:n]) for n in TIERS[:-1]]
    out += [(f'dig{n}', BS[:n] + [S[3]]) for n in DIGITS]
    return out + list_reads('v', 9, n=40, pool=S + TS[:200])


PROBES = ['tie', 'prefix', 'shortest-last', 'count-tie', 'drop', 'long',
          'names', 'twice'] + [f'tier{n}' for n in TIERS] + \
    [f'dig{n}' for n in DIGITS]


# ---- commands --------------------------------------------------------------------
def _cases():
    genus = genus_of()
    H = {'genus.map': _map_file(genus), 'phylum.map': _map_file(phylum_of())}
    HN = dict(H)
    HN['names.txt'] = _map_file(names_of())
    big = dict(genus)
    big.update({s: 'Gc' for s in BIG_SUBJECTS})
    HB = dict(H)
    HB['genus.map'] = _map_file(big)
    tiers = dict(genus)
    tiers.update({s: tier_genus(i) for i, s in enumerate(TS)})
    tiers.update({s: 'Gc' for s in BS})
    phyla = phylum_of()
    phyla.update({f'H{k:02d}': 'P2' for k in range(N_H)})
    HT = {'genus.map': _map_file(tiers), 'phylum.map': _map_file(phyla)}

    def case(name, aln, hier=H, fmt='map', block=None, slot=None,
             host_blocks=0, gold=None, **kw):
        files = {f'aln/{k}': v for k, v in aln.items()}
        files.update(hier)
        kwargs = dict(input_fmt=fmt, map_rank=True,
                      map_fps=[k for k in hier if k.endswith('.map')], **kw)
        return dict(name=name, files=files, kwargs=kwargs, block=block,
                    slot=slot, host_blocks=host_blocks, gold=gold or name)
    plain = {'S.map': map_text(plain_reads())}
    orf = {'S.map': map_text(orf_reads())}
    sam = R.sam_text(mate_runs())
    grow = {'S.map': map_text(grow_reads())}
    names = dict(name_as_id=True, names_fps=['names.txt'])
    commands = [
        # doc/stratify.md, Method II, step 1
        case('orf-genus-names', orf, HN, ranks='genus', trimsub='_', **names),
        case('orf-phylum-genus', orf, ranks='phylum,genus', trimsub='_'),
        case('exclude', {'S.sam': R.sam_text(exclude_runs())}, fmt='sam',
             ranks='genus', exclude=EXCLUDED),
        case('none-free-genus', plain, ranks='none,free,genus'),
        case('free-genus', plain, ranks='free,genus'),
        case('none-genus', orf, ranks='none,genus', trimsub='_'),
        case('unassigned', plain, ranks='none,free,genus', unassigned=True),
        case('plain-text', plain, ranks='free,genus', outmap_zip='none'),
        case('names-mixed', plain, HN, ranks='none,free,genus', **names),
        case('mates', {'S.sam': sam}, fmt='sam', ranks='none,free,genus'),
        case('formats', {'B.b6o': b6o_text(plain_reads(3) + T0.slash_reads()),
                         'P.paf': paf_text(plain_reads(4) + T0.slash_reads()),
                         'M.map': map_text(plain_reads(6) + T0.slash_reads())},
             fmt=None, ranks='free,genus'),
        case('gz', {'S.map.gz': gzip.compress(map_text(orf_reads(5)),
                                              mtime=0)},
             ranks='genus', trimsub='_'),
        case('sam-gz', {'S.sam.gz': gzip.compress(sam, mtime=0)}, fmt='sam',
             ranks='free,genus'),
        case('grow', grow, HN, ranks='none,free,genus', unassigned=True,
             block=BLOCK, **names),
        case('grow-small-slot', grow, HN, ranks='none,free,genus',
             unassigned=True, block=BLOCK, slot=SMALL_SLOT, gold='grow',
             **names),
        case('handoff', {'S.map': map_text(T0.handoff_reads())}, HB,
             ranks='free,genus', block=HANDOFF_BLOCK, host_blocks=1),
        case('tiers', {'S.map': map_text(tier_reads())}, HT,
             ranks='none,free,genus'),
    ]
    neighbours = [
        # R1m's: no job of the set returns a list
        case('none-genus-uniq', orf, ranks='none,genus', trimsub='_',
             uniq=True),
        # R1's: plain jobs, the tokenizer's ids are the subjects', every
        # subject has a genus
        case('plain-only', {'S.map': map_text(tree_reads())},
             ranks='none,genus'),
    ]
    return commands, neighbours


def cli_cases():
    """The command cases: [{'name', 'files': {relative path: bytes},
    'kwargs', 'block', 'slot', 'host_blocks': blocks the host takes, 'gold':
    the case whose reference text is this one's too}]"""
    return _cases()[0]


def neighbour_cases():
    """Commands next to the scope, which keep their routes."""
    return _cases()[1]


# ---- single blocks ---------------------------------------------------------------
BLOCK_SIZES = (1, 255, 256, 257, 65537)
BLOCK_SUBJECTS = S + [LONG_ID, 'z', 'Gb', 'Gb1', 'g']
_PERIOD = 24 * len(BLOCK_SUBJECTS)     # queries (8), sizes (3) and subjects (35) repeat


def block_reads(n, kind='all'):
    """``n`` reads of the block cases.  'all': 2 .. 4 subjects each (a list
    under `--rank none`); 'nobody': one subject each; 'last': like 'nobody' but
    for the last read."""
    reads, m = [], len(BLOCK_SUBJECTS)
    for i in range(n):
        q = 'abcdefgh'[i % 8] * (1 + i % 3)
        one = kind == 'nobody' or (kind == 'last' and i < n - 1)
        k = 1 if one else 2 + i % 3
        reads.append((q, [BLOCK_SUBJECTS[(i + 11 * j) % m] for j in range(k)]))
    return reads


def _periodic(n, kind, fn):
    if kind == 'all' and n > _PERIOD:
        return fn(block_reads(_PERIOD)) * (n // _PERIOD) + \
            fn(block_reads(n % _PERIOD))
    return fn(block_reads(n, kind))


def block_text(n, kind='all'):
    return _periodic(n, kind, map_text)


def block_map_text(n, kind='all', shown=None):
    """The map of the block under `--rank none`, by the plain model."""
    return _periodic(n, kind, lambda reads: b''.join(
        model_line(q, model_value(s, 'none', None), shown) for q, s in reads))


def block_cases():
    return {f'n{n}': n for n in BLOCK_SIZES}


# ---- a plain model ------------------------------------------------------------------
def model_value(subs, rank, hier, uniq=False, above=False, major=None,
                subok=False):
    """What classify.assign_none / assign_free / assign_rank (classify.py:32-
    127) give for the subjects ``subs``: a feature id, None or the list of the
    distinct subjects' taxa (None where a subject has none)."""
    subs = list(dict.fromkeys(subs))
    if rank == 'free' or uniq or ((above or major) and rank != 'none'):
        return T0.assign(subs, rank, hier, uniq=uniq, above=above,
                         major=major, subok=subok)
    if rank == 'none':
        return subs[0] if len(subs) == 1 else subs
    tree, rankdic = hier

    def find_rank(x):
        while x is not None and rankdic.get(x) != rank:
            x = tree.get(x)
        return x
    taxa = [find_rank(s) for s in subs]
    return taxa[0] if len(set(taxa)) == 1 else taxa


def model_line(query, value, namedic=None, unassigned=False):
    """The line file.write_readmap (file.py:469-500) prints for it (bytes;
    empty: none)."""
    def show(t):
        return namedic.get(t, t) if namedic else t
    if isinstance(value, list):
        tally = {}
        for t in value:
            if t:
                tally[t] = tally.get(t, 0) + 1
        cols = [f'{show(t)}:{n}' for t, n in sorted(
            tally.items(), key=lambda x: (-x[1], x[0].encode()))]
    elif value:
        cols = [show(value)]
    elif unassigned:
        cols = ['Unassigned']
    else:
        return b''
    return ('\t'.join([query] + cols) + '\n').encode()


def summary(text):
    """{'lines', 'lists', 'probes': {QNAME: {'pairs', 'head', 'tail'}}} of a
    map text (bytes): what `check_gold` asks of a text the fixture keeps only
    a digest of."""
    lines = text.split(b'\n')[:-1]
    out = {'lines': len(lines), 'lists': 0, 'probes': {}}
    for line in lines:
        q, _, rest = line.partition(b'\t')
        pairs = rest.count(b'\t') + 1 if b':' in rest else 0
        out['lists'] += pairs > 0
        if q.decode() in PROBES:
            out['probes'][q.decode()] = {
                'pairs': pairs, 'head': rest[:60].decode(),
                'tail': rest[-24:].decode()}
    return out


# ---- what the cases promise --------------------------------------------------------
def check_inputs():
    cases = {c['name']: c for c in cli_cases() + neighbour_cases()}
    assert len(cases) == len(cli_cases()) + len(neighbour_cases())
    g = genus_of()
    edges = {q: s for q, s, _ in edge_reads()}
    assert [g[s] for s in edges['prefix']] == ['Gb1', 'Gb']
    assert sorted(g[s] for s in edges['shortest-last']) == ['Ga', 'Gh', 'g']
    assert [g.get(s) for s in edges['drop']] == [None, None, 'Ga']
    names = names_of()
    ids = ['Ga', 'Gb', 'Gb1']
    assert sorted(ids, key=lambda t: names.get(t, t)) != ids and \
        'Gb' not in names
    kinds = {w for _, _, w in mate_runs()}
    assert {'unpaired', 'only1', 'only2', 'both', 'all3', 'lists'} <= kinds
    orf = dict(orf_reads())
    assert len(orf['twice']) == 3 and \
        len({s.rsplit('_', 1)[0] for s in orf['twice']}) == 2
    tiers = dict(tier_reads())
    for n in TIERS:
        assert len(set(tiers[f'tier{n}'])) == n, n
    assert len({tier_genus(TS.index(s)) for s in tiers[f'tier{MAX_K}']}) == N_H
    assert len({tier_genus(TS.index(s)) for s in tiers['tier65']}) > 40
    for n in DIGITS:
        assert len(set(tiers[f'dig{n}'])) == n + 1 <= MAX_K
    assert n_blocks(cases['grow']) == GROW_N
    text = cases['grow']['files']['aln/S.map']
    for blk in range(GROW_N):
        at = text.index(f'\tN{blk:02d}_'.encode())
        assert at // BLOCK == blk, (blk, at // BLOCK)
        new = S[3 + min(blk * 9, 27) - 1]
        assert blk == 0 or text.index(f'\t{new}\n'.encode()) // BLOCK == blk
    h = cases['handoff']['files']['aln/S.map']
    assert len(dict(reads_of(h, 'map'))[BIG_Q]) == MAX_K + 1
    at = h.index(f'\n{BIG_Q}\t'.encode()) + 1
    assert 0 < HANDOFF_BLOCK - at < 2000
    assert len(h) > 2 * HANDOFF_BLOCK + 2000 and n_blocks(cases['handoff']) == 3
    for n in (1, 255, 257):
        assert reads_of(block_text(n), 'map') == block_reads(n)
        assert block_map_text(n).count(b'\n') == n == \
            block_map_text(n).count(b':1\n')
    assert b':' not in block_map_text(300, 'nobody') and \
        block_map_text(300, 'last').count(b':1\n') == 1
    assert all(a[0] != b[0] for a, b in zip(block_reads(_PERIOD),
                                            block_reads(_PERIOD + 1)[1:]))


def check_gold(gold):
    """The edges are in the reference's text (a fixture that has lost them is
    no fixture), and a quarter of every command's lines are lists."""
    cli = gold['cli']

    def rows(case, prefix=''):
        (text,) = [v for k, v in cli[case]['maps'].items()
                   if k.startswith(prefix)]
        assert isinstance(text, str), (case, prefix)
        return dict(x.split('\t', 1) for x in text.split('\n')[:-1])

    def probe(case, prefix, q):
        (s,) = [v for k, v in cli[case]['summary'].items()
                if k.startswith(prefix)]
        return s['probes'][q]
    for case in cli_cases():
        if case['gold'] != case['name']:
            continue
        s = cli[case['name']]['summary'].values()
        lists, lines = sum(x['lists'] for x in s), sum(x['lines'] for x in s)
        assert 4 * lists >= lines > 0, (case['name'], lists, lines)
    for case in neighbour_cases():
        assert case['name'] in cli
    assert not any(x['lists'] for x in
                   cli['none-genus-uniq']['summary'].values())
    gen = rows('none-free-genus', 'genus')
    assert gen['tie'] == 'Ga:1\tGc:1' and gen['prefix'] == 'Gb:1\tGb1:1' and \
        gen['shortest-last'] == 'Ga:1\tGh:1\tg:1' and \
        gen['count-first'] == 'Gc:2\tGa:1' and \
        gen['count-tie'] == 'Ga:2\tGc:2\tGb:1' and gen['drop'] == 'Ga:1' and \
        gen['drop2'] == 'Ga:1\tGc:1' and 'nogenus-only' not in gen and \
        gen['same'] == 'Ga' and gen['one'] == 'g'
    none = rows('none-free-genus', 'none')
    assert none['long'] == f'{LONG_ID}:1\tS00:1' and \
        none['same'] == 'S03:1\tS04:1\tS05:1' and \
        none['nogenus-only'] == 'X0:1\tX1:1' and none['one'] == 'S00' and \
        none['drop'] == 'S04:1\tX0:1\tZ0:1'
    free = rows('none-free-genus', 'free')
    assert not any(':' in v for v in free.values()) and free['same'] == 'Ga'
    un = rows('unassigned', 'genus')
    assert un['nogenus-only'] == 'Unassigned' and un['drop'] == 'Ga:1' and \
        un['tie'] == 'Ga:1\tGc:1'
    # under --name-as-id the ids order the list, the names are shown
    nm = rows('names-mixed', 'genus')
    assert nm['names'] == 'N' * 200 + ':1\tGb:1\tb one:1' and \
        nm['shortest-last'] == 'N' * 200 + ':1\tGh:1\tn:1'
    assert rows('names-mixed', 'none')['named-subject'] == 'zero:1\tS01:1'
    og = rows('orf-genus-names')
    assert og['twice'] == 'N' * 200 + ':1\tc c:1' and og['drop'] == og['twice'][:202]
    assert rows('orf-phylum-genus', 'genus')['twice'] == 'Ga:1\tGc:1'
    assert rows('none-genus', 'none')['twice'] == 'S03:1\tS12:1'
    assert set(cli['plain-text']['maps']) == {'free/S.txt', 'genus/S.txt'}
    mates = rows('mates', 'none')
    for q in ('u', 'f/1', 's/2', 'b/1', 'b/2', 't', 't/1', 't/2', 'w/1', 'w/2'):
        assert q in mates, q
    assert any(q.endswith('/2') and ':' in v for q, v in mates.items()) and \
        any('/' not in q and ':' in v for q, v in mates.items())
    for fn in ('B.txt', 'P.txt', 'M.txt'):
        text = cli['formats']['maps'][f'genus/{fn}']
        assert 'm/2\tg\n' in text and 'n/2\tGa:1\tGe:1\n' in text and \
            'tie\tGa:1\tGc:1\n' in text
    ex = rows('exclude')
    gone = {f'y{i}' for i in range(0, 60, 10)}
    assert 'keep/1' in ex and not any(q.startswith('drop') for q in ex) and \
        not any(q.split('/')[0] in gone for q in ex) and \
        any(q.startswith('y') and ':' in v for q, v in ex.items())
    gn = rows('grow', 'none')
    for blk in range(GROW_N):
        assert any(f'N{blk:02d}_' in v and ':' in v for v in gn.values()), blk
    assert all((len(v) if isinstance(v, str) else v['bytes']) >
               GROW_N * SMALL_SLOT * 4 for v in cli['grow']['maps'].values())
    hf = cli['handoff']['maps']
    assert f'\n{BIG_Q}\tGc\n' in hf['genus/S.txt'] and \
        '\tGa:1\tGb:1\tg:1\n' in hf['genus/S.txt']
    # the tiers of the wave kernel and the digits of the counts
    for n in TIERS:
        assert probe('tiers', 'none', f'tier{n}')['pairs'] == n, n
        assert probe('tiers', 'genus', f'tier{n}')['pairs'] == \
            len({tier_genus(TS.index(s)) for s in dict(tier_reads())[f'tier{n}']})
    assert probe('tiers', 'none', f'tier{MAX_K}')['tail'].endswith('tffe:1')
    assert probe('tiers', 'genus', f'tier{MAX_K}')['pairs'] == N_H
    for n in DIGITS:
        p = probe('tiers', 'genus', f'dig{n}')
        assert p['head'] == f'Gc:{n}\tGa:1' and p['pairs'] == 2, n
        assert probe('tiers', 'none', f'dig{n}')['pairs'] == n + 1
    for name, n in block_cases().items():
        assert gold['blocks'][name]['lines'] == n
