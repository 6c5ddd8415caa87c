"""Inputs of the read-map cases of tests/golden/vectors/readmap_device.json:
hand-written alignments and hierarchies whose `--outmap` text probes the device
writer (csrc/wk_readmap.hpp) at its edges -- `cli_cases` for whole commands,
`block_cases` for single blocks through `Context.dtok_readmap` -- rebuilt from
fixed seeds both by tests/golden/make_readmap_reference.py (which runs the
reference on them) and by tests/test_gpu_readmap.py / tests/test_readmap_host.py.
Only what the reference makes of them is committed: the text of every map file
(verbatim below `VERBATIM` bytes, else `digest`), and the tables.

Classification uses plain map files (`genus.map`, `phylum.map`), so the taxon
ids are the cases' to choose.  This module imports neither the package nor the
reference; `reads_of`, `taxa_of` and `tables_of` are a plain model of what a
read map is made from, for the tests that feed the formatters directly.

A read on the device route has at most 16 subjects, and a line whose subjects
all share one taxon carries no count: the largest count the device can print is
15 (`digits`).  The count 16 is in `handoff-big`, whose one read of 17 subjects
sends its block to the host formatter."""
import gzip
import hashlib
import os
import random

BLOCK = 1 << 15             # Engine.DTOK_BLOCK of `blocks`
SMALL = 1 << 13             # ... of the hand-off cases (their text stays verbatim)
VERBATIM = 1 << 16          # larger map texts are kept as digests
MAX_K = 16                  # subjects of a read the device takes (WK_WEIGHT_MAX_K)

# ids that are prefixes of each other and whose string order is not their
# numeric order
SUFFIX = ['', '1', '10', '100', '2', '9', 'a', 'A', '11', '1a', '20', '_',
          '-1', '.5', '0', '01']
SUBJECTS = [p + s for p in ('G', 'H', 'g') for s in SUFFIX]         # 48
TAXA = ['T', 'T1', 'T10', 'T100', 'T2', 'T9', 'Ta', 't2', 'T11', 'T1a', 't',
        't10']
PHYLA = ['P', 'P1', 'P10', 'p']
D = [f'D{i:02d}' for i in range(16)]        # 16 subjects of one taxon
E = [f'E{i:02d}' for i in range(16)]        # 16 subjects of 16 taxa
BLOCK_SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 2097152, 2097153)


def genus_of():
    """{subject: genus taxon} of the hierarchy most cases share."""
    m = {s: TAXA[(i * 7 + i // 12) % 12] for i, s in enumerate(SUBJECTS)}
    m.update({s: 'T5' for s in D})
    m.update({s: f'U{i}' for i, s in enumerate(E)})
    return m


def phylum_of():
    taxa = TAXA + ['T5'] + [f'U{i}' for i in range(16)]
    return {t: PHYLA[(3 * i + i // 5) % 4] for i, t in enumerate(taxa)}


def _map_file(d):
    return ''.join(f'{k}\t{v}\n' for k, v in d.items()).encode()


def names_of():
    """Names whose order is the reverse of their ids' order; T9 has none, T1
    and T10 share one, one name is a single byte, one 200 bytes long; two
    subjects have names too (shown at rank none)."""
    ids = sorted(t for t in TAXA if t != 'T9')
    names = sorted(['b', 'c two words', 'd  two blanks', 'e e e', 'f f',
                    'g' * 200, 'h h', 'i i', 'j j', 'k k', 'l l'])
    out = dict(zip(ids, reversed(names)))
    out['T10'] = out['T1']
    out['G1'] = 'subject one'
    out['G10'] = 'a subject'
    return out


# ---- reads ----------------------------------------------------------------------
def _spread_reads(tag, seed, n=150):
    """[(QNAME, [subjects])]: reads of 2..16 subjects; the first ones spread
    over 8, 12 and 12 taxa with (at least 8) equal counts."""
    rng = random.Random(seed)
    reads = [SUBJECTS[:8], SUBJECTS[:12], SUBJECTS[:16], SUBJECTS[12:28],
             SUBJECTS[40:48] + SUBJECTS[:8], SUBJECTS[:2]]
    reads += [rng.sample(SUBJECTS, rng.randint(2, MAX_K)) for _ in range(n)]
    return [(f'{tag}{i}', subs) for i, subs in enumerate(reads)]


def _digit_reads():
    reads = [D[:k] + [E[k]] for k in (1, 2, 9, 10, 11, 15)]
    reads += [D[:16], E[:16], D[:1], D[:9] + E[:7], D[:10] + E[10:16],
              D[3:14] + SUBJECTS[:5]]
    return [(f'd{i}', subs) for i, subs in enumerate(reads)]


def map_text(reads):
    return ''.join(f'{q}\t{s}\n' for q, subs in reads for s in subs).encode()


def b6o_text(reads):
    return ''.join(f'{q}\t{s}\t98.5\t100\t0\t0\t1\t100\t{1 + k}\t{100 + k}'
                   '\t1e-9\t200\n'
                   for q, subs in reads for k, s in enumerate(subs)).encode()


def paf_text(reads):
    return ''.join(f'{q}\t100\t0\t100\t+\t{s}\t9999999\t{k}\t{100 + k}\t100'
                   '\t100\t60\n'
                   for q, subs in reads for k, s in enumerate(subs)).encode()


FLAGS = {0: (0, 16, 256), 1: (99, 83, 355), 2: (147, 163, 403)}
LONG_Q = 'Q' * 250
STAR_Q = 'starred'


def mate_runs():
    """[(QNAME, [(mate, subject) | None, ...], what)]: the runs of `mates`;
    None is a line of another QNAME with RNAME '*' (align.py:315-319: skipped
    before the QNAME is looked at, so the run goes on)."""
    S = SUBJECTS
    runs = [
        ('m-un', [(0, S[0]), (0, S[1]), (0, S[12])], 'unpaired'),
        ('m-1', [(1, S[2]), (1, S[3]), (1, S[14])], 'only1'),
        ('m-2', [(2, S[4]), (2, S[5]), (2, S[16])], 'only2'),
        ('m-il', [(1, S[0]), (2, S[1]), (1, S[2]), (2, S[3]), (1, S[4]),
                  (2, S[5])], 'interleaved'),
        ('m-all', [(0, S[6]), (1, S[7]), (2, S[8]), (0, S[9]), (2, S[10]),
                   (1, S[11])], 'all3'),
        ('m-21', [(2, S[1]), (2, S[13]), (1, S[2]), (1, S[14])], '2before1'),
        ('m-rep', [(1, S[0]), (1, S[0]), (1, S[12]), (1, S[0])], 'repeat'),
        ('m-sh', [(1, S[0]), (2, S[0]), (1, S[1]), (2, S[2])], 'shared'),
        (STAR_Q, [(0, S[3]), None, (0, S[4])], 'star'),
        ('x', [(1, S[5]), (2, S[6]), (2, S[7])], 'short'),
        (LONG_Q, [(2, S[8]), (1, S[9]), (1, S[20])], 'long'),
        ('m-02', [(0, S[0]), (2, S[1]), (0, S[2])], 'un+2'),
        ('m-s2', [(1, S[3]), None, (2, S[4]), None], 'star2'),
    ]
    rng = random.Random(404)
    for i in range(60):
        runs.append((f'mr{i}', [(rng.randrange(3), rng.choice(S[:24]))
                                for _ in range(rng.randint(1, 12))], 'random'))
    return runs


def sam_text(runs):
    rows = ['@HD\tVN:1.0\tSO:unsorted']
    k = 0
    for q, lines, _ in runs:
        for item in lines:
            k += 1
            if item is None:
                rows.append(f'other{k}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*')
                continue
            mate, s = item
            rows.append(f'{q}\t{FLAGS[mate][k % 3]}\t{s}\t{k}\t42\t10M\t=\t1\t0'
                        '\t*\t*')
    return ('\n'.join(rows) + '\n').encode()


def _filler(tag, until, pools, rng, start=0):
    """Reads of 1..3 subjects until the text is ``until`` bytes long; `pools`:
    [(from byte, subjects)] -- a pool's subjects appear from that byte on."""
    reads, pos, i = [], start, 0
    while pos < until:
        pool = [s for at, subs in pools if pos >= at for s in subs]
        fresh = [subs for at, subs in pools if at and at <= pos < at + 400]
        subs = rng.sample(fresh[-1] if fresh else pool, rng.choice((1, 1, 2, 3)))
        q = f'{tag}{i:06d}'
        reads.append((q, subs))
        pos += sum(len(q) + len(s) + 2 for s in subs)
        i += 1
    return reads


BLOCKS_N = 42
A_SET = [f'A{i:02d}' for i in range(30)]
B_SET = [f'B{i}' for i in range(10)]
C_SET = [f'A0{i}x' for i in range(6)]
D_SET = ['A', 'A0', 'a']
NEW_AT = ((1, B_SET), (7, C_SET), (BLOCKS_N - 1, D_SET))


def _blocks_hier():
    genus = {s: f'X{i % 9}' for i, s in enumerate(A_SET)}
    genus.update({s: f'X{i % 3}{i % 2}' for i, s in enumerate(B_SET)})   # new taxa between the old
    genus.update({s: ('X', 'X10', 'X1')[i % 3] for i, s in enumerate(C_SET)})
    genus.update({'A': 'W', 'A0': 'X', 'a': 'X4'})
    taxa = list(dict.fromkeys(genus.values()))
    phylum = {t: ('PH2', 'PH10', 'PH1')[i % 3] for i, t in enumerate(taxa)}
    return genus, phylum


def _blocks_reads():
    rng = random.Random(77)
    pools = [(0, A_SET)] + [(int((k + 0.5) * BLOCK), subs)
                            for k, subs in NEW_AT]
    return _filler('b', (BLOCKS_N - 0.2) * BLOCK - 2000, pools, rng)


BIG_Q = 'the17'


def _handoff_big_reads():
    rng = random.Random(88)
    a = _filler('h', int(2.5 * SMALL), [(0, SUBJECTS)], rng)
    big = [(BIG_Q, D[:16] + [E[3]])]
    at = len(map_text(a + big))
    b = _filler('i', int(4.6 * SMALL), [(0, SUBJECTS)], rng, start=at)
    return a + big + b


MISSING = 'Zmissing'


def _handoff_rank_reads():
    rng = random.Random(99)
    a = _filler('k', int(2.5 * SMALL), [(0, SUBJECTS)], rng)
    at = len(map_text(a))
    b = _filler('l', int(4.6 * SMALL), [(0, SUBJECTS + [MISSING] * 6)], rng,
                start=at)
    return a + [('first-missing', [SUBJECTS[0], MISSING])] + b


# ---- commands --------------------------------------------------------------------
def cli_cases():
    """[{'name', 'files': {relative path: bytes}, 'kwargs', 'block',
    'slot', 'route': 'device' | 'handoff'}]"""
    H1 = {'genus.map': _map_file(genus_of())}
    ties = _spread_reads('r', 101)

    def case(name, aln, hier=H1, ranks='none,genus', fmt='map', route='device',
             block=None, slot=None, **kw):
        files = {f'aln/{k}': v for k, v in aln.items()}
        files.update(hier)
        kwargs = dict(input_fmt=fmt, ranks=ranks, map_rank=None,
                      map_fps=[k for k in hier if k.endswith('.map')], **kw)
        return dict(name=name, files=files, kwargs=kwargs, block=block,
                    slot=slot, route=route)
    names = dict(H1)
    names['names.txt'] = _map_file(names_of())
    bg, bp = _blocks_hier()
    bh = {'genus.map': _map_file(bg), 'phylum.map': _map_file(bp)}
    blocks = {'S.map': map_text(_blocks_reads())}
    two = _spread_reads('w', 303, 40)
    out = [
        case('ties', {'S.map': map_text(ties)}),
        case('digits', {'S.map': map_text(_digit_reads())}),
        case('names', {'S.map': map_text(_spread_reads('n', 202))}, names,
             name_as_id=True, names_fps=['names.txt']),
        case('mates', {'S.sam': sam_text(mate_runs())}, fmt='sam'),
        case('formats', {'B.b6o': b6o_text(ties), 'P.paf': paf_text(ties)},
             fmt=None),
        case('blocks', blocks, bh, 'none,genus,phylum', block=BLOCK),
        case('blocks-small-slot', blocks, bh, 'none,genus,phylum', block=BLOCK,
             slot=4096),
        case('gz', {'S.map.gz': gzip.compress(map_text(ties), mtime=0)}),
        case('handoff-big', {'S.map': map_text(_handoff_big_reads())},
             route='handoff', block=SMALL),
        case('handoff-rank', {'S.map': map_text(_handoff_rank_reads())}, H1,
             'genus', route='handoff', block=SMALL),
        case('two-samples', {
            'S1.map': map_text(two[:20] + [('same', SUBJECTS[:3])]),
            'S2.map': map_text([('same', SUBJECTS[5:9])] + two[20:])}),
    ]
    return out


DOOR_CASES = ('ties', 'digits', 'names', 'mates')   # also through the direct door and the host formatters


def n_blocks(case):
    """Blocks the device text route cuts the case's files into: a plain file
    that is not SAM is read `block` bytes at a time (the unfinished last run
    goes in front of the next block)."""
    total = 0
    for k, v in case['files'].items():
        if k.startswith('aln/'):
            total += -(-len(v) // case['block']) if case['block'] else 1
    return total


def block_of(case, needle):
    """Index of the block in which ``needle`` first appears."""
    (text,) = [v for k, v in case['files'].items() if k.startswith('aln/')]
    return text.index(needle) // case['block']


def write_cli(case, root):
    """The case's files under ``root``; returns workflow's keyword arguments
    (all but ``output_fp`` and ``outmap_dir``)."""
    for rel, data in case['files'].items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(data)
    kw = dict(case['kwargs'], input_fp=os.path.join(root, 'aln'),
              output_fmt=False)
    for k in ('map_fps', 'names_fps'):
        if k in kw:
            kw[k] = [os.path.join(root, x) for x in kw[k]]
    return kw


def digest(text):
    """What is kept of a map text too large to keep."""
    assert text[-1:] in (b'', b'\n')
    return {'sha256': hashlib.sha256(text).hexdigest(), 'bytes': len(text),
            'lines': text.count(b'\n')}


def kept(text):
    return text.decode() if len(text) < VERBATIM else digest(text)


def run_cli(workflow, case, root):
    """Run ``workflow`` on the case: {'maps': {relative path without .gz: bytes},
    'tables': {file name: text}}."""
    import contextlib
    import io
    kw = write_cli(case, root)
    out, maps = os.path.join(root, 'out'), os.path.join(root, 'maps')
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(output_fp=out, outmap_dir=maps, **kw)
    got = {}
    for dirpath, _, files in os.walk(maps):
        for fn in files:
            fp = os.path.join(dirpath, fn)
            assert fn.endswith('.txt.gz'), fn
            with gzip.open(fp, 'rb') as f:
                got[os.path.relpath(fp, maps)[:-3]] = f.read()
    if os.path.isdir(out):
        tables = {fn: open(os.path.join(out, fn), newline='').read()
                  for fn in sorted(os.listdir(out))}
    else:
        with open(out, newline='') as f:
            tables = {'out': f.read()}
    return {'maps': got, 'tables': tables}


def first_difference(got, want):
    """'line / read N: got ..., want ...' for two map texts (bytes): a map
    has one line per read, so N (from 0) is the read's number too."""
    a, b = got.split(b'\n'), want.split(b'\n')
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f'line / read {i}: got {x[:300]!r}, want {y[:300]!r}'
    return f'{len(a) - 1} lines, want {len(b) - 1}; the common ones are equal'


def compare(got, want, what, model=None):
    """Assert that the map text ``got`` (bytes) is what the fixture holds
    (``want``: text, or a `digest`).  ``model()``: the text the plain model
    below writes for the case -- where the fixture holds a digest, a mismatch
    is told by its first differing line against that text (which must itself
    have the fixture's digest)."""
    if isinstance(want, str):
        assert got == want.encode(), \
            f'{what}: ' + first_difference(got, want.encode())
        return
    have = digest(got)
    if have != want:
        where = ''
        if model is not None:
            text = model()
            assert digest(text) == want, f'{what}: the model misses the digest'
            where = '; ' + first_difference(got, text)
        raise AssertionError(
            f'{what}: {have["bytes"]} bytes in {have["lines"]} lines, want '
            f'{want["bytes"]} in {want["lines"]}{where}')


# ---- single blocks ---------------------------------------------------------------
BLOCK_SUBJECTS = SUBJECTS[:40]
_PERIOD = 120       # reads after which names (30), subjects (40) and the every-fourth (4) repeat


def _partners():
    g = genus_of()
    same, other = {}, {}
    for s in BLOCK_SUBJECTS:
        same[s] = next(x for x in BLOCK_SUBJECTS if x != s and g[x] == g[s])
        other[s] = next(x for x in BLOCK_SUBJECTS if g[x] != g[s])
    return same, other


def block_reads(n):
    """The first ``n`` reads of the block cases (n <= _PERIOD here; the text
    repeats)."""
    same, other = _partners()
    reads = []
    for i in range(n):
        q = 'abcdefghij'[i % 10] * (1 + i % 3)
        s = BLOCK_SUBJECTS[i % 40]
        reads.append((q, [s, same[s], other[s]] if i % 4 == 0 else [s]))
    return reads


def block_text(n):
    period = map_text(block_reads(_PERIOD))
    return period * (n // _PERIOD) + map_text(block_reads(n % _PERIOD))


def block_cases():
    return {f'n{n}': n for n in BLOCK_SIZES}


# ---- a plain model ---------------------------------------------------------------
def reads_of(text, fmt):
    """[(query as printed, [distinct subjects in order])] of a simple map or
    SAM text, the way align.py:258-347, 621-674 group them."""
    out = []
    this, pool = None, ({}, {}, {})

    def flush():
        for m, tag in enumerate(('', '/1', '/2')):
            if pool[m]:
                out.append((this + tag, list(pool[m])))
    for line in text.decode().split('\n'):
        if not line or (fmt == 'sam' and line[0] == '@'):
            continue
        f = line.split('\t')
        if fmt == 'sam':
            q, s, mate = f[0], f[2], int(f[1]) >> 6 & 3
            if s == '*':
                continue
        else:
            q, s, mate = f[0], f[1], 0
        if q != this:
            flush()
            this, pool = q, ({}, {}, {})
        pool[mate][s] = 1
    flush()
    return out


def taxa_of(subs, tax):
    """{taxon: count} of a read's subjects (``tax``: {subject: taxon}, or None
    at rank none)."""
    c = {}
    for s in subs:
        t = tax[s] if tax else s
        c[t] = c.get(t, 0) + 1
    return c


def map_line(query, subs, tax, namedic=None):
    """The read's line as file.py:469-500 prints it."""
    c = taxa_of(subs, tax)
    show = (lambda t: namedic.get(t, t)) if namedic else (lambda t: t)
    if len(c) == 1:
        return f'{query}\t{show(next(iter(c)))}'
    return '\t'.join([query] + [f'{show(t)}:{n}' for t, n in
                                sorted(c.items(), key=lambda x: (-x[1], x[0]))])


def tables_of(subjects, tax, namedic=None):
    """(slot of every subject, the slots' order by id string, bytes shown per
    slot) -- what `Context.readmap_tables` takes; slots in order of first
    appearance."""
    ids = [tax[s] if tax else s for s in subjects]
    slots = list(dict.fromkeys(ids))
    where = {t: i for i, t in enumerate(slots)}
    rank = {t: i for i, t in enumerate(sorted(slots))}
    return ([where[t] for t in ids], [rank[t] for t in slots],
            [(namedic.get(t, t) if namedic else t).encode() for t in slots])


def _pairs(text):
    return dict(x.split('\t') for x in text.decode().split('\n')[:-1])


def model_maps(case):
    """{relative path: bytes} of the map files of a command on simple maps, as
    the plain model writes them (every subject has a taxon at every rank)."""
    files, ranks = case['files'], case['kwargs']['ranks'].split(',')
    genus = _pairs(files['genus.map'])
    tax = {'none': None, 'genus': genus}
    if 'phylum.map' in files:
        phylum = _pairs(files['phylum.map'])
        tax['phylum'] = {s: phylum[t] for s, t in genus.items()}
    out = {}
    for rel, text in files.items():
        if not rel.endswith('.map') or not rel.startswith('aln/'):
            continue
        reads = reads_of(text, 'map')
        for rank in ranks:
            fn = f'{rel[4:-4]}.txt'
            out[fn if len(ranks) == 1 else f'{rank}/{fn}'] = ''.join(
                map_line(q, s, tax[rank]) + '\n' for q, s in reads).encode()
    return out


def block_map_text(n):
    """The genus map of the block case of ``n`` reads, by the plain model."""
    g = genus_of()
    def rows(k):
        return ''.join(map_line(q, s, g) + '\n'
                       for q, s in block_reads(k)).encode()
    return rows(_PERIOD) * (n // _PERIOD) + rows(n % _PERIOD)


# ---- what the cases promise --------------------------------------------------------
def check_inputs():
    g = genus_of()
    cases = {c['name']: c for c in cli_cases()}
    assert sorted(TAXA) != sorted(TAXA, key=lambda t: (len(t), t))
    assert sorted(TAXA)[:4] == ['T', 'T1', 'T10', 'T100'] and \
        sorted(TAXA).index('T2') > sorted(TAXA).index('T100')
    ties = reads_of(cases['ties']['files']['aln/S.map'], 'map')
    assert all(2 <= len(s) <= MAX_K for _, s in ties)
    spread = [taxa_of(s, g) for _, s in ties]
    assert sum(len(c) >= 8 and len(set(c.values())) == 1 for c in spread) >= 2
    assert any(sum(n == 1 for n in c.values()) >= 8 and
               max(c.values()) > 1 for c in spread)
    dig = [taxa_of(s, g) for _, s in
           reads_of(cases['digits']['files']['aln/S.map'], 'map')]
    for top in (1, 2, 9, 10, 11, 15):
        assert any(max(c.values()) == top and len(c) == 2 and
                   min(c.values()) == 1 for c in dig), top
    assert any(len(c) == 16 for c in dig) and \
        any(c == {'T5': 16} for c in dig) and any(c == {'T5': 1} for c in dig)
    nm = names_of()
    ids = sorted(t for t in TAXA if t in nm and t != 'T10')
    assert [nm[t] for t in ids] == sorted((nm[t] for t in ids), reverse=True)
    assert 'T9' not in nm and nm['T1'] == nm['T10'] and \
        {1, 200} <= {len(v) for v in nm.values()} and \
        all(' ' in v or len(set(v)) == 1 for v in nm.values())
    kinds = {what for _, _, what in mate_runs()}
    assert {'unpaired', 'only1', 'only2', 'interleaved', 'all3', '2before1',
            'repeat', 'shared', 'star', 'short', 'long'} <= kinds
    sam = reads_of(cases['mates']['files']['aln/S.sam'], 'sam')
    assert (STAR_Q, [SUBJECTS[3], SUBJECTS[4]]) in sam
    assert ('m-rep/1', [SUBJECTS[0], SUBJECTS[12]]) in sam
    assert ('m-sh/1', SUBJECTS[:2]) in sam and \
        ('m-sh/2', [SUBJECTS[0], SUBJECTS[2]]) in sam
    assert [q for q, _ in sam if q.startswith('m-21')] == ['m-21/1', 'm-21/2']
    assert {len(q) for q, _ in sam} >= {3, 252}
    assert all(len(s) <= MAX_K for _, s in sam)
    # blocks: 42 of them; new subjects (and taxa) in blocks 1, 7 and the last
    b = cases['blocks']
    assert n_blocks(b) == BLOCKS_N >= 40 and \
        cases['blocks-small-slot']['files'] == b['files']
    for k, subs in NEW_AT:
        at = min(block_of(b, f'\t{s}\n'.encode()) for s in subs)
        assert at == k, (k, at)
    assert all(len(s) <= 3 for _, s in reads_of(b['files']['aln/S.map'], 'map'))
    # hand-offs: one read of 17 subjects / a subject without a genus, in the
    # middle block of five
    hb = cases['handoff-big']
    reads = reads_of(hb['files']['aln/S.map'], 'map')
    assert [q for q, s in reads if len(s) > MAX_K] == [BIG_Q]
    assert n_blocks(hb) == 5 and block_of(hb, BIG_Q.encode()) == 2
    assert taxa_of(dict(reads)[BIG_Q], g) == {'T5': 16, 'U3': 1}
    hr = cases['handoff-rank']
    assert n_blocks(hr) == 5 and block_of(hr, MISSING.encode()) == 2
    assert MISSING not in g
    s1, s2 = (reads_of(cases['two-samples']['files'][f'aln/{s}.map'], 'map')
              for s in ('S1', 'S2'))
    assert s1[-1][0] == s2[0][0] and s1[-1][1] != s2[0][1]
    # single blocks: every line a read of its own but the every-fourth's three
    for n in (1, 255, 257):
        reads = reads_of(block_text(n), 'map')
        assert len(reads) == n and reads == block_reads(n)
    reads = block_reads(_PERIOD)
    assert block_reads(2 * _PERIOD)[_PERIOD:] == reads
    assert all(a[0] != b[0] for a, b in zip(reads, reads[1:] + reads[:1]))
    assert {len(q) for q, _ in reads} == {1, 2, 3}
    assert all((len(s) == 3 and len(taxa_of(s, g)) == 2) if i % 4 == 0
               else len(s) == 1 for i, (_, s) in enumerate(reads))


def check_gold(gold):
    """The edges are in the reference's text (a fixture that has lost them is
    no fixture)."""
    import re
    cli = gold['cli']

    def lines(case, rank):
        (text,) = [v for k, v in cli[case]['maps'].items()
                   if k.startswith(rank)]
        assert isinstance(text, str), (case, rank)
        return [x.split('\t') for x in text.split('\n')[:-1]]

    def counts(row):
        return [int(x.rsplit(':', 1)[1]) for x in row[1:]] \
            if len(row) > 2 else []
    dig = lines('digits', 'genus')
    tops = {max(counts(r)) for r in dig if counts(r)}
    assert {1, 2, 9, 10, 11, 15} <= tops, tops
    assert any(len(r) == 17 for r in dig)               # 16 columns
    assert any(len(r) == 17 for r in lines('digits', 'none'))
    assert ['d6', 'T5'] in dig and ['d8', 'T5'] in dig  # one taxon: no count
    # the count of 16: the read of 17 subjects, which the host formats
    big = cli['handoff-big']['maps']
    assert f'{BIG_Q}\tT5:16\tU3:1\n' in big['genus/S.txt']
    assert all(isinstance(v, str) for k in ('handoff-big', 'handoff-rank')
               for v in cli[k]['maps'].values())
    for case, rank in (('ties', 'genus'), ('ties', 'none'), ('names', 'none')):
        rows = lines(case, rank)
        assert any(len(r) >= 9 and len(set(counts(r))) == 1 for r in rows)
    for r in lines('ties', 'genus'):
        ids = [x.rsplit(':', 1)[0] for x in r[1:]]
        key = [(-c, t) for c, t in zip(counts(r), ids)]
        assert key == sorted(key), r
    assert all(len(r) >= 3 for r in lines('ties', 'none'))
    nm = lines('names', 'genus')
    assert any(':' in x and ' ' in x for r in nm for x in r[1:])
    assert any(x.startswith('g' * 200) for r in nm for x in r[1:])
    assert any(re.fullmatch(r'T9(:\d+)?', x) for r in nm for x in r[1:])
    mates = {r[0]: r[1:] for r in lines('mates', 'none')}
    for q in ('m-un', 'm-1/1', 'm-2/2', 'm-il/1', 'm-il/2', 'm-all', 'm-all/1',
              'm-all/2', 'm-21/1', 'm-21/2', 'x/1', 'x/2', LONG_Q + '/1',
              LONG_Q + '/2', 'm-02', 'm-02/2', 'm-s2/1', 'm-s2/2'):
        assert q in mates, q
    for q in ('m-un/1', 'm-1', 'm-1/2', 'm-2', 'm-2/1', 'm-il', 'm-21'):
        assert q not in mates, q
    order = [r[0] for r in lines('mates', 'none')]
    assert order.index('m-21/1') + 1 == order.index('m-21/2')
    assert order.index('m-all') + 2 == order.index('m-all/2')
    assert mates['m-rep/1'] == [f'{SUBJECTS[0]}:1', f'{SUBJECTS[12]}:1']
    assert mates['m-sh/1'][0].startswith('G:1') and \
        mates['m-sh/2'][0].startswith('G:1')
    assert mates[STAR_Q] == [f'{SUBJECTS[3]}:1', f'{SUBJECTS[4]}:1']
    assert not any(q.startswith('other') for q in mates)
    for name, n in block_cases().items():
        assert gold['blocks'][name]['lines'] == n
