"""Hand-written rows for the coord-match parsers, one numeric edge per row:
what POS and CIGAR (SAM), x[3] / x[8] / x[9] / x[11] (BLAST tabular) and
x[7] / x[8] / x[10] / x[11] (PAF) may hold, and what the three parsers of this
package -- the "ex" flavour of the device tokenizer (csrc/wk_dtok.hpp), the
host tokenizer (csrc/wk_tokenize.cpp) and the reference they restate
(align.parse_*_file_ex) -- make of it.

A case is {'name', 'fmt', 'cls', 'text', 'subject', 'query'} (+ 'ref',
'finding', 'note', 'probe').  'text' is one line, without its newline; the
cases about skipped lines, runs and mates span several lines, whose hit-bearing
lines share the case's subject.  Every case has a subject of its own (P000, P001, ...), so
a result is traced back to its row, and a query of its own.

The contract ('cls'):

  stay   the device parses the row: status 0 and the reference's integers
  back   the device hands the block back (status 1); the host tokenizer gives
         the reference's records, or raises the reference's exception
  wide   a number beyond the 32 bits coordinates are held in: status 1 on the
         device, `ValueError` matching '32 bits' on the host.  Never a wrapped
         value.  (The reference carries a Python int.)

'ref' says what the reference's parser does with the text: 'records' (the
default), 'skips' (no record at all) or 'raises'.  'finding': a negative
aligned length, which the reference's parser takes and its matcher refuses
(see `FINDING`).

tests/golden/make_coords_rows_reference.py runs the reference over every case
and checks these claims before it writes
tests/golden/vectors/coords_rows.json; tests/test_coords_rows_host.py holds the
host tokenizer to that file, tests/test_gpu_coords_rows.py the device."""
import numpy as np

STAY, BACK, WIDE = 'stay', 'back', 'wide'
FORMATS = ('sam', 'b6o', 'paf')
I32 = 2 ** 31 - 1

FINDING = """\
A negative aligned length (BLAST x[3], PAF x[10], a CIGAR number with a minus
sign: int() takes them all).  The reference's parser yields it;
ordinal.ordinal_mapper then stores it into a uint32 array (ordinal.py:205,
233), which numpy >= 2 refuses with OverflowError, while range.range_mapper
(`--outcov`) never looks at the length and accepts the row.  The host tokenizer
used to cast it: length 4294967291, counted on.  Chosen answer: what the
reference's commands do -- OverflowError wherever the length is read, the row
accepted where it is not -- because a length that cannot be is better refused
than guessed at, and because that is the one answer the reference gives with
the numpy this package is built against.  A wrapped length is the only outcome
that is never accepted."""


# ---- one line of each format, every field in its ordinary form ----------------
def sam(q, s, pos='1', cigar='10M', flag='0'):
    return f'{q}\t{flag}\t{s}\t{pos}\t42\t{cigar}\t*\t0\t0\t*\t*'


def b6o(q, s, length='10', sstart='1', send='10', score='200', tail=''):
    return (f'{q}\t{s}\t98.5\t{length}\t0\t0\t1\t10\t{sstart}\t{send}\t1e-9\t'
            f'{score}{tail}')


def paf(q, s, start='0', end='10', alen='10', mapq='60', tail=''):
    return (f'{q}\t10\t0\t10\t+\t{s}\t9999\t{start}\t{end}\t10\t{alen}\t'
            f'{mapq}{tail}')


ROW = {'sam': sam, 'b6o': b6o, 'paf': paf}
GOOD_SUBJECT = 'G0'         # the subject of the rows around a row under test
GOOD_GENE = (100, 110)      # its one gene (start0, end): matched by `good`


def good(fmt, q):
    """An ordinary row: one hit (G0, length 10, 100, 110)."""
    if fmt == 'sam':
        return sam(q, GOOD_SUBJECT, pos='101')
    if fmt == 'b6o':
        return b6o(q, GOOD_SUBJECT, sstart='101', send='110')
    return paf(q, GOOD_SUBJECT, start='100', end='110')


def around(case, k=2):
    """The case's text with `k` good rows in front and `k` behind."""
    fmt, name = case['fmt'], case['query']
    head = [good(fmt, f'{name}-a{i}') for i in range(k)]
    tail = [good(fmt, f'{name}-z{i}') for i in range(k)]
    return '\n'.join(head + [case['text']] + tail) + '\n'


# ---- the table ------------------------------------------------------------------
def _table():
    out = []

    def add(fmt, name, cls, build, ref='records', finding=False, note='',
            probe=True):
        i = len(out)
        q, s = f'q{i:03d}', f'P{i:03d}'
        text = build(q, s)
        out.append(dict(name=f'{fmt}:{name}', fmt=fmt, cls=cls, text=text,
                        subject=s, query=q, ref=ref, finding=finding,
                        note=note, probe=probe))

    def one(fmt, **kw):
        return lambda q, s: ROW[fmt](q, s, **kw)

    # ---- SAM POS: [+-]digits, at most 10 digits, the result within int32
    for name, pos, cigar in [('pos-1', '1', '10M'), ('pos-0', '0', '10M'),
                             ('pos-minus5', '-5', '10M'),
                             ('pos-plus7', '+7', '10M'),
                             ('pos-10-digits', '0000000012', '10M'),
                             ('pos-int32-max-1M', '2147483647', '1M')]:
        add('sam', name, STAY, one('sam', pos=pos, cigar=cigar))
    for name, pos in [('pos-11-digits', '00000000012'),
                      ('pos-blank-before', ' 5'), ('pos-blank-behind', '5 '),
                      ('pos-underscore', '1_0')]:
        add('sam', name, BACK, one('sam', pos=pos))
    for name, pos in [('pos-empty', ''), ('pos-letter', 'x')]:
        add('sam', name, BACK, one('sam', pos=pos), ref='raises')
    add('sam', 'pos-int32-max-10M', WIDE, one('sam', pos='2147483647'))
    add('sam', 'pos-2^31-10M', WIDE, one('sam', pos='2147483648'))

    # ---- SAM CIGAR: (digits op)+
    for cigar in ['100M', '10=5X', '5S10M5S', '3H10M', '10M2I10M', '10M3D10M',
                  '10M100N10M', '10M2P10M']:
        add('sam', f'cigar-{cigar}', STAY, one('sam', pos='201', cigar=cigar))
    add('sam', 'cigar-0M', STAY, one('sam', cigar='0M'))
    add('sam', 'cigar-empty', STAY, one('sam', cigar=''))
    # (an I / S / H / P resets the digits collected; nobody converts them)
    add('sam', 'cigar-I-alone', STAY, one('sam', cigar='I'))
    add('sam', 'cigar-S-without-digits', STAY, one('sam', cigar='S10M'))
    add('sam', 'cigar-int32-max-M', STAY, one('sam', cigar='2147483647M'))
    for name, cigar in [('digits-alone', '10'), ('digits-behind', '10M5'),
                        ('star', '*'), ('lower-case', '10m'),
                        ('underscore', '1_0M'), ('plus', '+5M'),
                        ('blank', ' 5M')]:
        add('sam', f'cigar-{name}', BACK, one('sam', cigar=cigar))
    add('sam', 'cigar-M-without-digits', BACK, one('sam', cigar='M'),
        ref='raises')
    for cigar in ['2147483648M', '4294967295M', '1099511627776M']:
        add('sam', f'cigar-{cigar}', WIDE, one('sam', cigar=cigar))
    add('sam', 'cigar-2^31-M-at-pos-0', WIDE,
        one('sam', pos='0', cigar='2147483648M'),
        note='start -1, end 2147483647, length 2^31: every number fits its '
             'array, but the host tokenizer of the parent commit asks the '
             'reference span (end - start) to fit int32 and raises "32 bits" '
             '-- so the row is wide.  The kernel of the parent commit parsed '
             'it (status 0); it now refuses a span beyond int32 as well.')
    add('sam', 'cigar-minus5M', BACK, one('sam', cigar='-5M'), finding=True)

    # ---- SAM QNAME and mate
    add('sam', 'mates-99-147-0', STAY, lambda q, s: '\n'.join([
        sam(q, s, pos='1', flag='99'), sam(q, s, pos='101', flag='147'),
        sam(q, s, pos='201', flag='0')]))
    add('sam', 'unmapped-inside-a-run', STAY, lambda q, s: '\n'.join([
        sam(q, s, pos='1'), sam(q, '*', pos='0', cigar='*', flag='4'),
        sam(q, s, pos='101')]))

    # ---- BLAST tabular
    add('b6o', 'sstart<send', STAY, one('b6o', sstart='21', send='30'))
    add('b6o', 'sstart>send', STAY, one('b6o', sstart='30', send='21'))
    add('b6o', 'sstart==send', STAY,
        one('b6o', length='1', sstart='7', send='7'))
    add('b6o', 'sstart-0', STAY, one('b6o', sstart='0', send='9'))
    add('b6o', 'sstart-minus3', STAY, one('b6o', sstart='-3', send='6'))
    # (dtok_int_field strips blanks and takes a sign, like int())
    for name, x in [('plus', '+5'), ('blank-before', ' 5'),
                    ('blank-behind', '5 ')]:
        add('b6o', f'sstart-{name}', STAY, one('b6o', sstart=x, send='14'))
    add('b6o', 'length-0', STAY, one('b6o', length='0'))
    for score in ['1e-5', '.5', '7.', '1.e3', '+.5e+2']:
        add('b6o', f'score-{score}', STAY, one('b6o', score=score))
    add('b6o', 'ends-in-cr', STAY, one('b6o', tail='\r'))
    add('b6o', '13th-field', STAY, one('b6o', tail='\tmore'))
    add('b6o', 'send-int32-max', STAY,
        one('b6o', sstart='2147483638', send='2147483647'))
    add('b6o', '4-fields', STAY, lambda q, s: f'{q}\t{s}\t98.5\t10',
        ref='skips')
    add('b6o', '2-fields', STAY, lambda q, s: f'{q}\t{s}', ref='skips')
    add('b6o', '1-field', STAY, lambda q, s: f'{q}{s}', ref='skips')
    add('b6o', 'empty-line', STAY, lambda q, s: '', ref='skips')
    add('b6o', 'short-row-inside-a-run', STAY, lambda q, s: '\n'.join([
        b6o(q, s), f'{q}\t{s}\t98.5\t10', b6o(q, s, sstart='101', send='110')]))
    add('b6o', 'short-row-of-another-query-inside-a-run', STAY,
        lambda q, s: '\n'.join([b6o(q, s), f'{q}x\t{s}\t98.5\t10',
                                b6o(q, s, sstart='101', send='110')]))
    for score in ['nan', 'inf', '1_0']:
        add('b6o', f'score-{score}', BACK, one('b6o', score=score))
    add('b6o', 'sstart-11-digits', BACK,
        one('b6o', sstart='00000000005', send='14'))
    add('b6o', 'length-underscore', BACK, one('b6o', length='1_0'))
    for name, score in [('1e', '1e'), ('point', '.'), ('empty', '')]:
        add('b6o', f'score-{name}', BACK, one('b6o', score=score),
            ref='raises')
    for length in ['1e2', '1.0']:
        add('b6o', f'length-{length}', BACK, one('b6o', length=length),
            ref='raises')
    add('b6o', '4-fields-abc', BACK, lambda q, s: f'{q}\t{s}\t98.5\tabc',
        ref='raises')
    add('b6o', 'send-2^31', WIDE,
        one('b6o', sstart='2147483639', send='2147483648'))
    add('b6o', 'length-minus5', BACK, one('b6o', length='-5'), finding=True)

    # ---- PAF
    add('paf', 'plain', STAY, one('paf', start='20', end='30'))
    add('paf', 'start>end', STAY, one('paf', start='20', end='10'),
        probe=False,
        note='passed on as it is.  A hit that ends before it starts has no '
             'overlap to speak of: the reference itself answers by the '
             'number of hits on the genome (match_read_gene_quart finds no '
             'gene, the sweep of match_read_gene would, since the hit closes '
             'before it opens and is never taken off the open reads).  So '
             'the row has no probe genome and only the cover door sees its '
             'numbers')
    add('paf', 'start-minus1', STAY, one('paf', start='-1', end='9'))
    add('paf', 'start-plus', STAY, one('paf', start='+4', end='14'))
    add('paf', 'start-blank', STAY, one('paf', start=' 4', end='14'))
    add('paf', 'alen-0', STAY, one('paf', alen='0'))
    add('paf', 'ends-in-cr', STAY, one('paf', tail='\r'))
    add('paf', '13th-field', STAY, one('paf', tail='\ttp:A:P'))
    add('paf', 'end-int32-max', STAY,
        one('paf', start='2147483637', end='2147483647'))
    add('paf', '10-fields', STAY,
        lambda q, s: f'{q}\t10\t0\t10\t+\t{s}\t9999\t0\t10\t10', ref='skips')
    add('paf', 'short-row-inside-a-run', STAY, lambda q, s: '\n'.join([
        paf(q, s), f'{q}\t10\t0\t10\t+\t{s}\t9999\t0\t10\t10',
        paf(q, s, start='100', end='110')]))
    # (the reference skips a row on ValueError; the device leaves that to the
    # host)
    for name, mapq in [('letter', 'x'), ('empty', ''), ('float', '60.0')]:
        add('paf', f'mapq-{name}', BACK, one('paf', mapq=mapq), ref='skips')
    add('paf', 'mapq-underscore', BACK, one('paf', mapq='6_0'))
    add('paf', 'alen-letter', BACK, one('paf', alen='x'), ref='skips')
    add('paf', 'start-letter', BACK, one('paf', start='x'), ref='skips')
    add('paf', 'end-2^31', WIDE,
        one('paf', start='2147483638', end='2147483648'))
    add('paf', 'alen-2^32', WIDE, one('paf', alen='4294967296'))
    add('paf', 'alen-minus5', BACK, one('paf', alen='-5'), finding=True)
    return out


_CASES = _table()


def cases(fmt=None, cls=None):
    return [c for c in _CASES if (fmt is None or c['fmt'] == fmt) and
            (cls is None or c['cls'] == cls)]


def check_cases():
    """What the table promises about itself."""
    names = [c['name'] for c in _CASES]
    assert len(names) == len(set(names))
    for key in ('subject', 'query'):
        assert len({c[key] for c in _CASES}) == len(_CASES)
    for fmt in FORMATS:
        for cls in (STAY, BACK, WIDE):
            assert cases(fmt, cls), (fmt, cls)
        assert any(c['finding'] for c in cases(fmt)), fmt
    for c in _CASES:
        assert c['ref'] in ('records', 'skips', 'raises')
        assert not (c['cls'] == STAY and c['ref'] == 'raises'), c['name']
        assert '\n' not in c['text'] or c['cls'] == STAY, c['name']


def block_of(some):
    """The cases' lines as one block of text."""
    return '\n'.join(c['text'] for c in some) + '\n'


PAD = 120       # good rows in front of and behind a command-level file


def cli_text(some):
    """The command-level file of the cases `some` (of one format): their
    lines between two pads of good rows, about 5 KB each, so that with blocks
    of 4 KB the file's first and last block hold good rows only."""
    fmt = some[0]['fmt']
    return ''.join(good(fmt, f'pad-a{i}') + '\n' for i in range(PAD)) + \
        block_of(some) + \
        ''.join(good(fmt, f'pad-z{i}') + '\n' for i in range(PAD))


def in_cli_file(case, gold):
    """Does the command-level file of the case's format hold it?  Every row
    that is not wide (there this package raises by contract, whatever the
    reference does) and on which the reference's command does not raise."""
    return case['cls'] != WIDE and gold['raises'][case['name']]['coords'] is None


# ---- probe genes ------------------------------------------------------------------
def probe_genes(hits):
    """Four genes per hit (start s, end e, length L > 0) of a case, matched
    at threshold 1.0 (a gene matches when it overlaps the hit by L or more):

      a  (s, s + L)          b  (e - L, e)            must match
      c  (s - 1, s + L - 1)  d  (e - L + 1, e + 1)    must not, by one base

    as [(name, start0, end)] sorted the way the gene tables want them.  `hits`
    are the positive-length hits of the case in order; the names carry the
    hit's index ('a0', 'b0', ..., 'a1', ...).  A gene whose coordinates leave
    int32 is left out (only d of the rows that end at 2^31 - 1); equal
    coordinates are kept once."""
    seen, out = set(), []
    for i, (s, e, ln) in enumerate(hits):
        for role, g in (('a', (s, s + ln)), ('b', (e - ln, e)),
                        ('c', (s - 1, s + ln - 1)),
                        ('d', (e - ln + 1, e + 1))):
            if g in seen or g[0] < -I32 - 1 or g[1] > I32:
                continue
            seen.add(g)
            out.append((f'{role}{i}', g[0], g[1]))
    return sorted(out, key=lambda g: (g[1:], g[0]))


def hits_of(records):
    """The positive-length hits [(s, e, L)] of a golden 'records' entry."""
    return [(s, e, ln) for _, recs in records for _, ln, s, e in recs if ln > 0]


def genes_of_case(case, gold):
    """The case's probe genes; none where the case says so ('probe')."""
    rec = gold['cases'][case['name']]['records']
    return probe_genes(hits_of(rec)) \
        if case['probe'] and isinstance(rec, list) else []


def gene_tables(some, gold, command=False):
    """(genomes, genome_off, start0, end, names) over the probe genes of the
    cases `some` and the good rows' genome, as wk_set_genes takes them.
    `command`: only the genes a coordinates file can say to every reader
    (start0 >= 0)."""
    genomes, off, start0, end, names = [GOOD_SUBJECT], [0, 1], \
        [GOOD_GENE[0]], [GOOD_GENE[1]], [f'{GOOD_SUBJECT}_g']
    for c in some:
        genes = [g for g in genes_of_case(c, gold)
                 if not command or g[1] >= 0]
        if not genes:
            continue
        genomes.append(c['subject'])
        for name, s, e in genes:
            start0.append(s)
            end.append(e)
            names.append(f'{c["subject"]}_{name}')
        off.append(len(start0))
    return genomes, np.asarray(off, np.int32), np.asarray(start0, np.int32), \
        np.asarray(end, np.int32), names


def coords_text(some, gold, command=False):
    """The same genes as a coordinates file (1-based, inclusive)."""
    genomes, off, start0, end, names = gene_tables(some, gold, command)
    out = []
    for i, g in enumerate(genomes):
        out.append(f'>{g}\n')
        for k in range(off[i], off[i + 1]):
            out.append(f'{names[k].split("_", 1)[1]}\t{start0[k] + 1}\t'
                       f'{end[k]}\n')
    return ''.join(out)
