"""SAM texts shaped after the limits of the one-kernel tokenizer
(csrc/wk_dtok_fused.hpp) and of the routes around it: deterministic recipes
(`random.Random(seed)`), regenerated wherever they are needed -- by
make_golden.py::gen_dtok_limits, which runs the reference on them, by
tests/test_dtok_limits_host.py and by tests/test_gpu_dtok_limits.py.  The texts
are never committed; tests/golden/vectors/dtok_limits.json holds their sha256
and what the reference made of them.

Pure Python; reads nothing but tests/golden/data/taxonomy/taxid.map.

Runs are made long by repeating subjects and by unmapped lines inside the run,
never by more subjects: a read names at most 16 distinct subjects per mate, so
that a long run does not turn into a "big read" (kDtokBigRead, which hands the
block to the host tokenizer for a reason of its own).

Constants named below (csrc/wk_dtok_fused.hpp unless said otherwise):
kFzTile = 16384, kFzBack = 1024, kFzFwd = 3072, kFzLines = 1024 lines per
window, kFzStreams = 4 slices, kSliceBins = 40608 subjects a slice
(csrc/wk_weigh.hpp), kMaxStreams = 8.  A tile is max(4096, block / (CUs x
dtok_fused_per_cu x rounds)) bytes, at most kFzTile (csrc/woltka_hip.hip,
dtok_scan_impl): 4 KB on blocks below about 12 MB at the default launch.
"""
import hashlib
import os
import random
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = '@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:x\tLN:5\n'
TAIL = '1\t42\t50M\t*\t0\t0\t*\t*'
UNPAIRED = (0, 16, 256, 272)
PAIRED = (99, 147, 83, 163, 355, 403)
SLICE = 40608                       # kSliceBins


def tax_subjects():
    """The first 90 genomes of the taxonomy fixture (all of them have an
    ancestor at every rank the cases ask for)."""
    with open(os.path.join(HERE, 'data', 'taxonomy', 'taxid.map')) as f:
        return [ln.split('\t')[0] for ln in f][:90]


TAX_KW = {'nodes_fps': ['$TAX/nodes.dmp'], 'map_fps': ['$TAX/taxid.map'],
          'ranks': 'none,genus'}


def _line(q, flag, s, tail=TAIL):
    return f'{q}\t{flag}\t{s}\t{tail}\n'


def _read(rng, q, subjects, k, out, unmapped=0.04, paired=None):
    """k lines of one QNAME (subjects drawn from `subjects`, repeats
    allowed), unmapped lines in between."""
    if paired is None:
        paired = rng.random() < 0.4
    for _ in range(k):
        if rng.random() < unmapped:
            out.append(f'{q}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n')
        out.append(_line(q, rng.choice(PAIRED if paired else UNPAIRED),
                         rng.choice(subjects)))


def _name_subjects():
    rng = random.Random('names')
    subj = []
    for _ in range(12):
        base = ''.join(rng.choice(NAME_ALPHABET) for _ in range(17))
        for n_ in NAME_LENGTHS:
            subj.append(base[:n_])
            subj.append(base[:n_ - 1] + rng.choice(NAME_ALPHABET))
    return sorted(set(subj))


NAME_ALPHABET = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789'
NAME_LENGTHS = (7, 8, 9, 15, 16, 17)
NAME_SUBJECTS = _name_subjects()
DENSE_SUBJECTS = [chr(65 + i) for i in range(26)] + \
    [chr(65 + i) + chr(65 + j) for i in range(6) for j in range(6)]


def _head(head, subjects):
    return [HEADER, _prologue(subjects)] if head else []


def _prologue(subjects):
    """A read per subject at the top of the file: the first block -- scanned
    the two-call way, its subjects interned -- names every subject, so that
    no later block is handed back for a subject the dictionary lacks."""
    return ''.join(f'p{i}\t0\t{s}\t*\n' for i, s in enumerate(subjects))


def _plain(rng, size, subjects, head=True):
    """The control: reads of 1-16 lines of 40-50 bytes."""
    out, n, q = _head(head, subjects), 0, 0
    while n < size:
        m = len(out)
        _read(rng, f'read{q:07d}', subjects,
              rng.choice([1, 1, 1, 2, 3, 5, 9, 16]), out)
        n += sum(map(len, out[m:]))
        q += 1
    return ''.join(out)


def _long_lines(rng, size, subjects, head=True, huge=True):
    """SEQ / QUAL kept.  One line in 12 of 1.1-3 KB: longer than kFzBack, so
    that a tile behind such a line finds no whole line in its window's back
    part and looks the run up in global memory (`fz_starts_run_slow`, :197,
    :443), and shorter than kFzFwd, so that the kernel keeps such blocks.
    With `huge`, one line in 20 of 8-40 KB, some of them unmapped, some the
    first or the last line of a run: longer than kFzFwd (a line that starts
    in a tile and does not end in its window: the trail check of e855e20,
    :358-361), than a 16 KB tile and than a 32 KB block.  The column trim
    takes these bytes away: they reach the kernel only on the untrimmed
    readers."""
    out, n, q = _head(head, subjects), 0, 0
    while n < size:
        m = len(out)
        name = f'read{q:07d}'
        paired = rng.random() < 0.4
        for _ in range(rng.choice([1, 1, 2, 3, 5, 9, 16])):
            flag = rng.choice(PAIRED if paired else UNPAIRED)
            s = rng.choice(subjects)
            tail = TAIL
            b = 0
            if rng.random() < 0.08:
                b = rng.randint(560, 1450)
            elif huge and rng.random() < 0.05:
                b = rng.choice([4000, 9000, 17000, 20000])
            if b:
                tail = f'1\t42\t{b}M\t*\t0\t0\t' + 'ACGT' * (b // 4) + \
                    '\t' + 'F' * b
                if rng.random() < 0.2:
                    flag, s = 4, '*'
            out.append(_line(name, flag, s, tail))
        n += sum(map(len, out[m:]))
        q += 1
    return ''.join(out)


def _long_runs(rng, size, subjects, head=True):
    """Runs of one QNAME of 120 (5 KB: more than kFzFwd, the look-ahead that
    must hold the rest of a tile's last run, :466-473), 420 (more than a
    16 KB tile) and 900 lines (40 KB: more than a 32 KB block), next to short
    ones.  At most six distinct subjects a run; unmapped lines at run starts,
    ends and inside."""
    out, n, q = _head(head, subjects), 0, 0
    while n < size:
        m = len(out)
        name = f'read{q:07d}'
        r = rng.random()
        k = (rng.choice([1, 2, 3, 8]) if r < 0.7 else 120 if r < 0.82 else
             420 if r < 0.92 else 900)
        pool = rng.sample(subjects, rng.randint(1, 6))
        if rng.random() < 0.5:
            out.append(f'{name}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n')
        _read(rng, name, pool, k, out, unmapped=0.03)
        if rng.random() < 0.5:
            out.append(f'{name}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n')
        n += sum(map(len, out[m:]))
        q += 1
    return ''.join(out)


def _dense(rng, size, _subjects, head=True):
    """Lines of 7-12 bytes (one- or two-character QNAMEs and subjects, an
    empty fourth field; runs of at most 8 lines): about 1 100 lines in the
    8 KB window of a 4 KB tile and 2 700 in the 20 KB window of a 16 KB one
    -- more than kFzLines (:52, :328) at both geometries."""
    lo = 'abcdefghijklmnopqrstuvwxyz0123456789'
    up = 'ABCDEFGHIJKLMNOPQRSTUVWXYZ'

    def name(chars):
        return rng.choice(chars) if rng.random() < 0.9 else \
            rng.choice(chars) + rng.choice(chars)
    out = _head(head, DENSE_SUBJECTS)
    n, run = 0, 0
    q = name(lo)
    while n < size:
        run += 1
        if rng.random() < 0.5 or run > 8:     # (runs of 8 lines at most)
            q2 = name(lo)
            while q2 == q:
                q2 = name(lo)
            q, run = q2, 1
        flag = '0' if rng.random() < 0.95 else rng.choice(['16', '256'])
        rest = '' if rng.random() < 0.9 else '1'
        sub = rng.choice(up) if rng.random() < 0.9 else \
            rng.choice(up[:6]) + rng.choice(up[:6])
        ln = f'{q}\t{flag}\t{sub}\t{rest}\n'
        out.append(ln)
        n += len(ln)
    return ''.join(out)


def _names(rng, size, _subjects, head=True):
    """QNAMEs and subjects of 7, 8, 9, 15, 16 and 17 bytes (the eight-byte
    steps of `fz_same` / `fz_hash`, the 15-byte split between names kept in
    the slot and names in the arena, `fz_probe_begin` / `_end`), prefixes of
    each other and names that differ only in their last byte, next to each
    other; QNAMEs of 300-2000 bytes (kDtokLongName of the six kernels)."""
    al, lens, subj = NAME_ALPHABET, NAME_LENGTHS, NAME_SUBJECTS
    out, n = _head(head, subj), 0
    while n < size:
        m = len(out)
        r = rng.random()
        if r < 0.15:
            ln = rng.randint(300, 2000)
        else:
            ln = rng.choice(lens)
        base = ''.join(rng.choice(al) for _ in range(ln))
        # the read, then one whose name is a prefix of it or differs from it
        # in the last byte, then one it is a prefix of
        names = [base, base[:-1] + ('x' if base[-1] != 'x' else 'y'),
                 base[:-1], base + rng.choice(al)]
        rng.shuffle(names)
        for nm in names[:rng.randint(2, 4)]:
            _read(rng, nm, rng.sample(subj, 6), rng.choice([1, 2, 3, 7]), out)
        n += sum(map(len, out[m:]))
    return ''.join(out)


def _qname_again(rng, size, subjects, head=True):
    """The same QNAME again after another one (two reads for parse_sam_file,
    align.py `if qname != this`) -- A B A, A B A B, A A B A -- everywhere, so
    across every tile and block edge; mates 64 / 128 / 0 interleaved inside
    one run; FLAG 4 with a real RNAME (a mapped line for the parsers, which
    look at RNAME only) and RNAME '*' with FLAG 0 (skipped)."""
    out, n, q = _head(head, subjects), 0, 0
    while n < size:
        m = len(out)
        a, b = f'qa{q:06d}', f'qb{q:06d}'
        for nm in rng.choice([[a, b, a], [a, b, a, b], [a, a, b, a],
                              [a, b, b, a, a]]):
            for _ in range(rng.randint(1, 4)):
                r = rng.random()
                if r < 0.1:
                    out.append(_line(nm, 0, '*'))
                elif r < 0.2:
                    out.append(_line(nm, 4, rng.choice(subjects)))
                else:
                    out.append(_line(nm, rng.choice([64, 128, 0, 65, 129, 16]),
                                     rng.choice(subjects)))
        n += sum(map(len, out[m:]))
        q += 1
    return ''.join(out)


def _late(rng, size, subjects):
    """Subjects first met late and often: two bursts, at a quarter and at
    half of the text, in which every read names a subject no block before it
    did (the block is handed back: the dictionary does not hold it), with
    hundreds of 8 KB blocks of known subjects behind each, so that the
    back-off after hand-backs in a row (2, 4, ... 32 blocks, woltka_hip.hip
    fz_handed_back) runs through and the kernel is taken again."""
    fresh = iter(f'L{i:05d}x' for i in range(100000))
    known = list(subjects[:20])
    out, n, q = [HEADER, _prologue(known)], 0, 0
    while n < size:
        m = len(out)
        burst = 0.25 * size <= n < 0.25 * size + 40000 or \
            0.5 * size <= n < 0.5 * size + 40000
        if burst:
            known.append(next(fresh))
            sub = known[-1:] + rng.sample(known, 2)
        else:
            sub = rng.sample(known, 5)
        _read(rng, f'read{q:07d}', sub, rng.choice([1, 1, 2, 3, 5]), out)
        n += sum(map(len, out[m:]))
        q += 1
    return ''.join(out)


def _slices(rng, n_subjects, _subjects):
    """`n_subjects` subjects met one after another (subject index = order of
    first appearance), each read naming a new one, so that
    the sample's subject table crosses kSliceBins boundaries mid-way and
    reads name subjects on both sides of one (three in ten: a new one and one
    met before): 4 slices at most (the kernel's
    per-slice record buffers, kFzStreams, :546-580), 5-8 (more than kFzStreams:
    the six kernels, woltka_hip.hip dtok_scan_impl), more than 8 (kMaxStreams:
    the job set is reopened unsliced, `words_roll`).  Short lines: these texts
    are long anyway."""
    out = [HEADER]
    for i in range(n_subjects):
        s = f'g{i:06d}'
        out.append(f'q{i:06d}\t0\t{s}\t*\n')
        if i >= 4 and rng.random() < 0.3:
            t = rng.randrange(i) if rng.random() < 0.5 else \
                rng.randrange(max(0, i - 2000), i)
            out.append(f'q{i:06d}\t0\tg{t:06d}\t*\n')
    return ''.join(out)


def _slices_again(rng, n_subjects, n_reads):
    """A second sample over the same subjects, every one of them known
    before its first block: reads of 1-3 subjects anywhere in the table (so
    across slices), long enough (3 MB: more than 40 blocks of 64 KB) for the
    back-off the first sample's hand-backs left to run out."""
    out = [HEADER]
    for i in range(n_reads):
        for _ in range(rng.randint(1, 3)):
            out.append(f'p{i:06d}\t0\tg{rng.randrange(n_subjects):06d}\t*\n')
    return ''.join(out)


def _exclude(rng, size, subjects, head=True):
    """Runs of 20-60 lines (1-2.7 KB: many of them cross a 4 KB tile's edge,
    few pass kFzFwd, so that the kernel keeps most blocks) whose
    last line names the excluded subject (`--exclude`: the whole read is
    dropped, align.py parse_sam_file_ft), next to runs that name it first or
    not at all."""
    ex = subjects[0]
    rest = subjects[1:]
    out, n, q = _head(head, subjects), 0, 0
    while n < size:
        m = len(out)
        name = f'read{q:07d}'
        k = rng.randint(20, 60) if rng.random() < 0.6 else rng.randint(1, 4)
        paired = rng.random() < 0.3
        pool = rng.sample(rest, 5)
        r = rng.random()
        if r < 0.2:
            out.append(_line(name, 0, ex))
        _read(rng, name, pool, k, out, unmapped=0.02, paired=paired)
        if r >= 0.2 and r < 0.7:
            out.append(_line(name, rng.choice(PAIRED if paired else UNPAIRED),
                             ex))
        n += sum(map(len, out[m:]))
        q += 1
    return ''.join(out)


def _ends(rng, size, subjects):
    """Four files: no newline behind the last line; '\\r\\n' line ends; a
    header longer than a 32 KB block; a file of header lines only."""
    a = _plain(rng, size, subjects).rstrip('\n')
    b = _plain(rng, size, subjects).replace('\n', '\r\n')
    hdr = ''.join(f'@SQ\tSN:{subjects[i % len(subjects)]}_{i}\t'
                  f'LN:{rng.randint(1000, 99999)}\n' for i in range(1500))
    c = HEADER + hdr + _plain(rng, size, subjects).split('\n', 2)[2]
    d = HEADER + hdr[:4000]
    return {'aln/S1.sam': a, 'aln/S2.sam': b, 'aln/S3.sam': c,
            'aln/S4.sam': d}


def _refusal(rng, size, subjects, which):
    """Text the kernel would take, then, past the first block, a line the
    reference raises on: FLAG with both mate bits (IndexError: `pool[mate]`
    with mate 3) or a header line in the body (ValueError: three fields)."""
    text = _plain(rng, size, subjects)
    cut = text.index('\n', int(len(text) * 0.7)) + 1
    if which == 'mates':
        bad = _line(f'read{9999999}', 195, subjects[0])
    else:
        bad = '@SQ\tSN:late\tLN:5\n'
    return text[:cut] + bad + text[cut:]


def _mixed(rng, size, subjects, shape, shape_len, plain_len, lead=0,
           plain=None, extra=()):
    """Stretches of a limit shape (`shape_len` bytes) between stretches of
    text the kernel keeps (`plain_len` bytes; `lead` bytes of them in front).
    The blocks of the shape's stretches are handed back; the back-off after
    hand-backs in a row (at most 2 ^ streak blocks) runs out inside the plain
    stretch behind, where the kernel keeps blocks again -- so that one text
    pins both the hand-back and the kernel's own work next to it.  A
    mutation that keeps what should be handed back turns the shape's
    stretches into wrong counts.  QNAMEs are renamed per stretch (`s<k>r`):
    no run goes on from one stretch into the next."""
    plain = plain or (lambda r, n: _plain(r, n, subjects, head=False))
    out = [HEADER, _prologue(list(extra) + list(subjects))]
    n, k = 0, 0

    def add(text):
        nonlocal n, k
        out.append(re.sub(r'(?m)^read', f's{k}r', text))
        n += len(text)
        k += 1
    if lead:
        add(plain(rng, lead))
    while n < size:
        add(shape(rng, shape_len))
        add(plain(rng, plain_len))
    return ''.join(out)


SHAPES = ('plain', 'long_lines', 'long_runs', 'dense', 'names', 'qname_again',
          'late_subjects', 'slices', 'ends', 'exclude', 'refusals')


def make_case(shape, seed, size, variant=None):
    """(files, kwargs) of one case: `files` maps a path under the case's
    directory to the text (str; written as UTF-8 bytes as they are, '\\r\\n'
    included); `kwargs` are `workflow.workflow`'s, with '$TAX/' for the
    taxonomy fixture and 'aln' for the directory of the files (`output_fp`
    and `output_fmt` are the caller's).  `size`: bytes of the main file
    (with `slices`: its number of subjects)."""
    rng = random.Random(f'{shape}:{variant}:{seed}:{size}')
    tax = tax_subjects()
    kw = {'input_fp': 'aln', 'input_fmt': 'sam'}
    # (the limit shapes in stretches: 24 KB of them between 128 KB the kernel
    # keeps; `t16`: 4.1 MB kept, 3.8 MB of the shape -- the second 4 MB
    # block --, 4.5 MB kept)
    lay = ((24 << 10, 128 << 10, 0) if variant != 't16' else
           (3_800_000, 4_500_000, 4_100_000))

    def mixed(fn, **k):
        return {'aln/S1.sam': _mixed(
            rng, size, tax, lambda r, n: fn(r, n, tax, head=False), *lay[:2],
            lead=lay[2], **k)}
    if shape == 'plain':
        files = {'aln/S1.sam': _plain(rng, size, tax)}
        kw.update(TAX_KW)
    elif shape == 'long_lines':
        # (the lines of 1.1-3 KB in the kept stretches make runs that pass
        # kFzFwd now and then: at 8 / 32 KB blocks most blocks still hold
        # none, of the 256 tiles of a 4 MB block some always do -- there the
        # kept stretches are plain)
        files = mixed(_long_lines, plain=None if variant == 't16' else
                      lambda r, n: _long_lines(r, n, tax, head=False,
                                               huge=False))
        kw.update(TAX_KW)
    elif shape == 'long_runs':
        files = mixed(_long_runs)
        kw.update(TAX_KW)
    elif shape == 'dense':
        files = mixed(_dense, extra=DENSE_SUBJECTS)
        kw['ranks'] = 'none'
    elif shape == 'names':
        files = mixed(_names, extra=NAME_SUBJECTS)
        kw['ranks'] = 'none'
    elif shape == 'qname_again':
        files = {'aln/S1.sam': _qname_again(rng, size, tax)}
        kw.update(TAX_KW)
    elif shape == 'late_subjects':
        files = {'aln/S1.sam': _late(rng, size, tax)}
        kw['ranks'] = 'none'
    elif shape == 'slices':
        files = {'aln/S1.sam': _slices(rng, size, tax),
                 'aln/S2.sam': _slices_again(rng, size, 75000)}
        kw['ranks'] = 'none'
    elif shape == 'ends':
        files = _ends(rng, size, tax)
        kw.update(TAX_KW)
    elif shape == 'exclude':
        files = {'aln/S1.sam': _exclude(rng, size, tax)}
        kw.update(TAX_KW)
        kw['exclude'] = tax[0]
        if variant == 'trimsub':       # (every name of both suffixes first)
            files = {k: HEADER + _prologue(
                [t + x for x in ('_1', '_2') for t in tax]) +
                _suffixed(rng, v).split('\n', 2)[2] for k, v in files.items()}
            kw['trimsub'] = '_'
            kw['exclude'] = tax[0] + '_1'
    elif shape == 'refusals':
        files = {'aln/S1.sam': _refusal(rng, size, tax, variant)}
        kw.update(TAX_KW)
    else:
        raise ValueError(shape)
    return files, kw


def _suffixed(rng, text):
    """RNAMEs of the taxonomy as `name_1` / `name_2` (`--trim-sub _`: two
    names, one subject; only `_1` of the first one is excluded)."""
    out = []
    for ln in text.split('\n'):
        f = ln.split('\t', 3)
        if len(f) == 4 and f[2].startswith('G'):
            f[2] += rng.choice(['_1', '_2'])
            ln = '\t'.join(f)
        out.append(ln)
    return '\n'.join(out)


def table_record(blob, small=2048):
    """A table as the vectors keep it: verbatim when small, else its digest
    (as ref_big_*.json)."""
    if len(blob) <= small:
        return blob.decode()
    return {'sha256': hashlib.sha256(blob).hexdigest(), 'bytes': len(blob),
            'rows': blob.count(b'\n') - 1}


def parse_digest(reads):
    """(query, subjects) pairs as `query\\tsorted subjects` lines -> sha256
    and the number of pairs."""
    h = hashlib.sha256()
    n = 0
    for q, subs in reads:
        h.update(('\t'.join([q] + sorted(subs)) + '\n').encode())
        n += 1
    return {'sha256': h.hexdigest(), 'reads': n}


# Geometries (tests/test_gpu_dtok_limits.py): the reader's block and the
# persistent workgroups per CU of the one kernel.  At the default launch (3 a
# CU) blocks of 8 / 32 KB give 4 KB tiles.  With one a CU (256 CUs), a block
# of 4 MB is one round of 16 KB tiles and one of 8 MB two rounds.  The first
# block of a file is scanned the two-call way (its subjects are interned):
# a geometry case holds at least one more whole block behind it.  Blocks of
# 64 KB for the texts of many subjects: the second sample must outlast the
# back-off the first one's hand-backs leave.
GEOMETRY = {
    'b8k': (8 << 10, None),
    'b32k': (32 << 10, None),
    'b64k': (64 << 10, None),
    'b4m_t16': (4 << 20, 1),
    'b8m_t16': (8 << 20, 1),
}

SMALL = ('b8k', 'b32k')

# name: (shape, variant, seed, size, geometries)
CASES = {
    'plain': ('plain', None, 1, 160_000, SMALL),
    'long_lines': ('long_lines', None, 2, 600_000, SMALL),
    'long_runs': ('long_runs', None, 3, 600_000, SMALL),
    'dense': ('dense', None, 4, 450_000, SMALL),
    'names': ('names', None, 5, 450_000, SMALL),
    'qname_again': ('qname_again', None, 6, 200_000, SMALL),
    'late_subjects': ('late_subjects', None, 7, 1_500_000, ('b8k',)),
    'ends': ('ends', None, 8, 80_000, SMALL),
    'exclude': ('exclude', None, 9, 250_000, SMALL),
    'exclude_trimsub': ('exclude', 'trimsub', 10, 250_000, SMALL),
    'refusal_mates': ('refusals', 'mates', 11, 120_000, SMALL),
    'refusal_header': ('refusals', 'header', 12, 120_000, SMALL),
    'slices_4': ('slices', None, 13, 150_000, ('b64k',)),
    'slices_8': ('slices', None, 14, 250_000, ('b64k',)),
    'slices_9': ('slices', None, 15, 340_000, ('b64k',)),
    'plain_t16': ('plain', None, 21, 17 << 20, ('b4m_t16', 'b8m_t16')),
    'long_lines_t16': ('long_lines', 't16', 22, 8 << 20, ('b4m_t16',)),
    'long_runs_t16': ('long_runs', 't16', 23, 8 << 20, ('b4m_t16',)),
    'dense_t16': ('dense', 't16', 24, 8 << 20, ('b4m_t16',)),
}


def case_files(name):
    shape, variant, seed, size, _ = CASES[name]
    return make_case(shape, seed, size, variant)
