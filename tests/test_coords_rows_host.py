"""The coord-match parsers row by row, the parts that need no GPU
(tests/coords_rows_cases.py; tests/golden/vectors/coords_rows.json is what the
reference makes of every row, written by
tests/golden/make_coords_rows_reference.py):

  * the fixture can see an error: every hit's probe genes tell a start, an
    end or a length that is off by one (the match door, through the C oracle),
    and a restatement of the device parsers with such an error built in is
    caught on every row;
  * that restatement -- `dtok_row_ex` and the SAM branch of
    `dtok_parse_kernel<true>` read line by line -- puts every row into the
    class the cases module names, and gives the reference's integers for the
    rows that stay;
  * the host tokenizer, which takes every block the device hands back, gives
    the reference's records, the reference's exception, or "32 bits" -- and
    never a wrapped value;
  * the command-level file of every format, through the host tokenizer and
    the oracle's matcher and counter, gives the reference's table."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import coords_rows_cases as T           # noqa: E402
from helpers import load_vectors        # noqa: E402
from test_tokenizer import run_native   # noqa: E402

GOLD = load_vectors('coords_rows.json')
CASES = {c['name']: c for c in T.cases()}
I32 = T.I32

# Rows whose hits the match door cannot judge in full; the cover door (which
# compares start and end themselves) judges them alone.  No more than the
# table implies: the one row that ends before it starts, and the `end + 1` of
# the four rows that end at 2^31 - 1 -- a number no int32 array can hold, so
# no kernel can produce it.
MATCH_DOOR_BLIND = {'paf:start>end'}
END_AT_INT32_MAX = {'sam:pos-int32-max-1M', 'sam:cigar-int32-max-M',
                    'b6o:send-int32-max', 'paf:end-int32-max'}
PERTURBATIONS = [('start', 1), ('start', -1), ('end', 1), ('end', -1),
                 ('length', 1), ('length', -1)]


def test_the_cases_and_the_fixture_belong_together():
    T.check_cases()
    assert set(GOLD['cases']) == set(CASES) == set(GOLD['raises'])
    for fmt in T.FORMATS:
        assert GOLD['cli'][fmt]['rows'] == [
            c['name'] for c in T.cases(fmt) if T.in_cli_file(c, GOLD)]
    for c in T.cases():
        rec = GOLD['cases'][c['name']]['records']
        assert (rec == 'ValueError') == (c['ref'] == 'raises'), c['name']
        if c['finding']:
            # see coords_rows_cases.FINDING: the parser takes the length, the
            # matcher's uint32 array refuses it, the coverage never reads it
            assert rec[0][1][0][1] == -5
            assert GOLD['cases'][c['name']]['genes'] == 'OverflowError'
            assert GOLD['raises'][c['name']] == {'coords': 'OverflowError',
                                                 'outcov': None}


# ---- the match door on the CPU --------------------------------------------------
def _matched(case, hits):
    """Per hit (s, e, L) on the case's subject: the names of the probe genes
    the C oracle matches at threshold 1.0."""
    import c_oracle
    genomes, off, start0, end, names = T.gene_tables([case], GOLD)
    if len(genomes) < 2 or not hits:
        return [set() for _ in hits]
    h = np.asarray(hits, np.int64).reshape(-1, 3)
    ph, pg = c_oracle.ordinal_match(
        off, start0, end, np.full(len(hits), 1, np.int32),
        h[:, 0].astype(np.int32), h[:, 1].astype(np.int32),
        h[:, 2].astype(np.uint32), 1.0)
    out = [set() for _ in hits]
    for i, g in zip(ph.tolist(), pg.tolist()):
        out[i].add(names[g])
    return out


def _golden_hits(case):
    """[(query, (s, e, L))] of the positive-length hits the reference parses."""
    rec = GOLD['cases'][case['name']]['records']
    return [(q, (s, e, ln)) for q, recs in rec for _, ln, s, e in recs
            if ln > 0]


def _judged(case):
    return case['cls'] == T.STAY and case['name'] not in MATCH_DOOR_BLIND


def test_the_oracle_matches_the_probe_genes_like_the_reference():
    n = 0
    for case in T.cases(cls=T.STAY):
        hits = _golden_hits(case)
        want = {}
        for (q, _), genes in zip(hits, _matched(case, [h for _, h in hits])):
            if genes:
                want.setdefault(q, set()).update(genes)
        assert GOLD['cases'][case['name']]['genes'] == [
            [q, sorted(g)] for q, g in want.items()], case['name']
        n += len(want)
    assert n >= 40


def test_every_hit_s_probe_genes_see_an_error_of_one():
    """The condition that keeps a blind fixture from passing a wrong kernel:
    start, end or length off by one, up or down, changes the set of genes a
    hit matches -- for every stay row of positive length with end - start >=
    length but those named above."""
    seen = 0
    for case in T.cases(cls=T.STAY):
        for _, (s, e, ln) in _golden_hits(case):
            if e - s < ln:
                assert case['name'] in MATCH_DOOR_BLIND, case['name']
                continue
            assert _judged(case)
            base = _matched(case, [(s, e, ln)])[0]
            assert base, case['name']
            for what, by in PERTURBATIONS:
                if (what, by) == ('end', 1) and e == I32:
                    assert case['name'] in END_AT_INT32_MAX
                    continue
                hit = (s + by * (what == 'start'), e + by * (what == 'end'),
                       ln + by * (what == 'length'))
                assert _matched(case, [hit])[0] != base, \
                    (case['name'], what, by)
                seen += 1
    assert seen >= 6 * 45
    # the lists above hold no row without need
    assert all(CASES[n]['cls'] == T.STAY for n in
               MATCH_DOOR_BLIND | END_AT_INT32_MAX)
    assert MATCH_DOOR_BLIND == {c['name'] for c in T.cases()
                                if not c['probe']}
    assert all(_golden_hits(CASES[n])[0][1][1] == I32
               for n in END_AT_INT32_MAX)


# ---- the device parsers, restated -----------------------------------------------
def _blank(ch):
    return ch == ' ' or '\t' <= ch <= '\r'


def _strip(t):
    b, e = 0, len(t)
    while b < e and _blank(t[b]):
        b += 1
    while e > b and _blank(t[e - 1]):
        e -= 1
    return t[b:e]


def _digits(t):
    return all('0' <= c <= '9' for c in t)


def _dev_int(t, strip=True):
    """dtok_int_field: blanks around, a sign, one to ten decimal digits."""
    t = _strip(t) if strip else t
    neg = t[:1] == '-'
    if t[:1] in ('-', '+'):
        t = t[1:]
    if not t or len(t) > 10 or not _digits(t):
        return None
    return -int(t) if neg else int(t)


def _dev_float(t):
    """dtok_float_field: blanks around, a sign, digits with a point, an
    exponent with digits."""
    t = _strip(t)
    if t[:1] in ('-', '+'):
        t = t[1:]
    i = n = 0
    while i < len(t) and '0' <= t[i] <= '9':
        i, n = i + 1, n + 1
    if i < len(t) and t[i] == '.':
        i += 1
        while i < len(t) and '0' <= t[i] <= '9':
            i, n = i + 1, n + 1
    if n == 0:
        return False
    if i < len(t) and t[i] in 'eE':
        i += 1
        if i < len(t) and t[i] in '+-':
            i += 1
        k = i
        while i < len(t) and '0' <= t[i] <= '9':
            i += 1
        if i == k:
            return False
    return i == len(t)


def device_row(fmt, line, bug=None):
    """One line as the "ex" flavour of the device tokenizer reads it:
    ('hit', subject, beg, end, length), ('skip',) or ('back',).  `bug`: the
    same with an error of one built in where the kernel computes the number
    ('start', +1 is the dropped `- 1` of POS and sstart)."""
    bug = bug or (None, 0)
    if fmt == 'sam':
        x = line.split('\t')
        if len(x) < 7:                      # not six tabs: kDtokShortLine
            return ('back',)
        if not x[1] or not _digits(x[1]) or len(x[1]) > 6:
            return ('back',)
        if x[2] == '*':
            return ('skip',)
        pos = _dev_int(x[3], strip=False)
        if pos is None:
            return ('back',)
        aligned = extra = num = 0
        have = False
        for ch in x[5]:
            if '0' <= ch <= '9':
                num, have = num * 10 + int(ch), True
                if num >= 1 << 40:
                    return ('back',)
            elif ch in 'M=X' or ch in 'DN':
                if not have:
                    return ('back',)
                if ch in 'DN':
                    extra += num
                else:
                    aligned += num
                num, have = 0, False
            elif ch in 'ISHP':
                num, have = 0, False
            else:
                return ('back',)
        if have:
            return ('back',)
        beg, end, n = pos - 1, pos - 1 + aligned + extra, aligned
        if not (beg >= -I32 and end <= I32 and aligned < 1 << 32 and
                aligned + extra <= I32):
            return ('back',)
        sub = x[2]
    else:
        x = line.split('\t', 12)
        b6o = fmt == 'b6o'
        if len(x) < 12:
            if b6o and len(x) >= 4 and _dev_int(x[3]) is None:
                return ('back',)
            return ('skip',)
        if b6o:
            n, a, b = _dev_int(x[3]), _dev_int(x[8]), _dev_int(x[9])
            ok = _dev_float(x[11])
        else:
            n, a, b = _dev_int(x[10]), _dev_int(x[7]), _dev_int(x[8])
            ok = _dev_int(x[11]) is not None
        if not ok or None in (n, a, b):
            return ('back',)
        beg, end = (min(a, b) - 1, max(a, b)) if b6o else (a, b)
        if not (0 <= n <= I32 and -I32 <= beg <= I32 and -I32 <= end <= I32):
            return ('back',)
        sub = x[1] if b6o else x[5]
    beg += bug[1] * (bug[0] == 'start')
    end += bug[1] * (bug[0] == 'end')
    n += bug[1] * (bug[0] == 'length')
    return ('hit', sub, beg, end, n)


def _device_rows(case, bug=None):
    return [device_row(case['fmt'], ln, bug)
            for ln in case['text'].split('\n')]


def test_the_restated_device_parsers_agree_with_the_classes_and_the_reference():
    for case in T.cases():
        rows = _device_rows(case)
        back = any(r == ('back',) for r in rows)
        assert back == (case['cls'] != T.STAY), (case['name'], rows)
        if back:
            continue
        # every line the device parses: the reference's records, in the
        # text's order (the reference orders a run by mate)
        got = sorted(r[1:] for r in rows if r[0] == 'hit')
        rec = GOLD['cases'][case['name']]['records']
        assert got == sorted((s, b, e, ln) for _, recs in rec
                             for s, ln, b, e in recs), case['name']


def _doors(case, rows):
    """What the two doors of tests/test_gpu_coords_rows.py would see of
    parsed rows: the genes of every positive hit, and the rows' ranges."""
    hits = [r for r in rows if r[0] == 'hit']
    pos = [(b, e, n) for _, _, b, e, n in hits if n > 0]
    ok = all(-2 ** 31 <= v <= I32 for h in pos for v in h)
    return (_matched(case, pos) if ok else 'not int32',
            sorted((b, e) for _, _, b, e, _ in hits))


@pytest.mark.parametrize('what,by', PERTURBATIONS)
def test_a_parser_that_is_off_by_one_is_caught_on_every_row(what, by):
    """dtok_row_ex and the SAM branch with `beg`, `end` or `llen` changed by
    one (start + 1: the `- 1` dropped), carried into the restatement above:
    the doors' view of every judged row with a hit differs from the view of
    the right numbers -- the comparisons of the GPU module would fail."""
    caught = 0
    for case in T.cases(cls=T.STAY):
        right = _device_rows(case)
        if not any(r[0] == 'hit' for r in right):
            continue
        wrong = _device_rows(case, (what, by))
        a, b = _doors(case, right), _doors(case, wrong)
        if what == 'length':
            # (the cover door never sees a length: the match door alone, on
            # the rows it judges and with a length to begin with)
            if not _judged(case) or not any(r[4] > 0 for r in right
                                            if r[0] == 'hit'):
                continue
            assert a[0] != b[0], case['name']
        else:
            assert a[1] != b[1], case['name']       # the cover door
            if _judged(case) and any(r[4] > 0 for r in right if r[0] == 'hit') \
                    and b[0] != 'not int32':
                assert a[0] != b[0], case['name']   # the match door
        caught += 1
    assert caught > 40


# ---- the host tokenizer ------------------------------------------------------------
def _expected(case, keep_empty):
    rec = GOLD['cases'][case['name']]['records']
    out = []
    for q, recs in rec:
        recs = [(s, None, ln, b, e) for s, ln, b, e in recs
                if ln or keep_empty]
        if recs:
            out.append((q, recs))
    return out


def _host(case, extra, threads=1, block=1 << 16):
    return run_native((case['text'] + '\n').encode(), threads, block,
                      extra=extra, fmt=case['fmt'])[0]


@pytest.mark.parametrize('extra', [True, 3])
@pytest.mark.parametrize('fmt', T.FORMATS)
def test_the_host_tokenizer_gives_the_reference_s_records(fmt, extra):
    """Under `extra=True` the hits of length 0 are dropped (ordinal.py:231),
    under `extra=3` they are kept (range.py:70)."""
    n = 0
    for case in T.cases(fmt):
        if case['cls'] == T.WIDE or case['ref'] == 'raises' or case['finding']:
            continue
        assert _host(case, extra) == _expected(case, extra == 3), case['name']
        n += 1
    assert n >= 15


@pytest.mark.parametrize('extra', [True, 3])
def test_wide_rows_raise_32_bits_on_the_host(extra):
    for case in T.cases(cls=T.WIDE):
        with pytest.raises(ValueError, match='32 bits'):
            _host(case, extra)


@pytest.mark.parametrize('extra', [True, 3])
def test_the_host_tokenizer_raises_where_the_reference_raises(extra):
    import builtins
    n = 0
    for case in T.cases():
        if case['ref'] != 'raises':
            continue
        err = getattr(builtins, GOLD['cases'][case['name']]['records'])
        with pytest.raises(err) as info:
            _host(case, extra)
        assert info.type is err, case['name']
        n += 1
    assert n >= 9


@pytest.mark.parametrize('fmt', T.FORMATS)
def test_a_negative_length_is_refused_and_never_wrapped(fmt):
    """coords_rows_cases.FINDING.  Wherever the lengths are read -- the
    coord-match, `extra=True`, and the coord-match with read maps, `extra=3`
    -- the host tokenizer raises what the reference's matcher raises; where
    they are not -- the coverage of `--outcov`, `extra=7` -- the row is
    accepted as the reference's command accepts it, its range as the
    reference's, its length 0.  (The parent commit gave length 4294967291.)"""
    (case,) = [c for c in T.cases(fmt) if c['finding']]
    gold = GOLD['raises'][case['name']]
    assert gold == {'coords': 'OverflowError', 'outcov': None}
    for extra in (True, 3):
        with pytest.raises(OverflowError, match='negative aligned length'):
            _host(case, extra)
    (q, recs), = _host(case, 7)
    (s, _, ln, b, e), = recs
    assert ln == 0 and q == case['query']
    assert {s: [b, e]} == GOLD['cases'][case['name']]['ranges']
    # between good rows, in a block cut small and tokenised by two threads
    text = T.around(case, k=40).encode()
    for extra in (True, 3):
        with pytest.raises(OverflowError):
            run_native(text, 2, 512, extra=extra, fmt=fmt)
    got = run_native(text, 2, 512, extra=7, fmt=fmt)[0]
    assert len(got) == 81 and all(ln != 4294967291 for _, r in got
                                  for _, _, ln, _, _ in r)


# ---- the commands, through the host tokenizer and the oracle ----------------------
def _table(text):
    rows = [x.split('\t') for x in text.splitlines()[1:]]
    return {k: int(v) for k, v in rows}


@pytest.mark.parametrize('threads,block', [(1, 1 << 16), (3, 256)])
@pytest.mark.parametrize('fmt', T.FORMATS)
def test_the_command_level_file_gives_the_reference_s_table(fmt, threads,
                                                            block):
    import woltka_oracle as O
    gold = GOLD['cli'][fmt]
    rows = [CASES[n] for n in gold['rows']]
    text = T.cli_text(rows).encode()
    # `--coords`, overlap 100
    reads, _ = run_native(text, threads, block, extra=True, fmt=fmt)
    genomes, off, start0, end, names = T.gene_tables(rows, GOLD, command=True)
    coords = {g: [(names[k].split('_', 1)[1], int(start0[k]), int(end[k]))
                  for k in range(off[i], off[i + 1])]
              for i, g in enumerate(genomes)}
    records = [(q, [(s, ln, b, e) for s, _, ln, b, e in recs])
               for q, recs in reads]
    queries, genes = O.ordinal_chunk(records, coords, 1.0, prefix=True)
    _, counts = O.classify_chunk(queries, genes, 'none')
    assert O.round_counts(counts) == _table(gold['coords']['table'])
    assert [len(queries)] == gold['coords']['classified']
    # `--outcov`: the plain table by subject, the merged ranges
    reads, _ = run_native(text, threads, block, extra=7, fmt=fmt)
    _, counts = O.classify_chunk([q for q, _ in reads],
                                 [{r[0] for r in recs} for _, recs in reads],
                                 'none')
    assert O.round_counts(counts) == _table(gold['outcov']['table'])
    assert [len(reads)] == gold['outcov']['classified']
    from woltka_amd.ranges import merge_intervals
    ids = sorted({r[0] for _, recs in reads for r in recs})
    flat = [(ids.index(s), b, e) for _, recs in reads
            for s, _, _, b, e in recs]
    k, b, e = merge_intervals(*(np.asarray(c, np.int64) for c in zip(*flat)))
    cov = ''.join(f'{ids[kk]}\t{bb}\t{ee}\n'
                  for kk, bb, ee in zip(k.tolist(), b.tolist(), e.tolist()))
    assert cov == gold['outcov']['cov']['S1.cov']
