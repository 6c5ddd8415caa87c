"""Run starts from the neighbouring lane and the subject lookup inside the line
pass of the one-kernel SAM tokenizer (csrc/wk_dtok_fused.hpp,
csrc/wk_dtok_neighbour.hpp).

Compared as tests/test_gpu_dtok_scan.py and tests/test_gpu_dtok_rounds.py
compare, on their helpers: the same 16 MB block goes through `dtok_scan_emit`
by the one kernel and by the six kernels at `dtok_fused_per_cu` = 1 (256 spans
of 64 KB, windows of 20 KB); status, lines, reads, records and cells are equal,
exactly, and a kept block also has the counts of `_model`.

The line pass deals line k of a window to thread k - first_line (mod 512): its
lane is (k - first_line) % 64, the line before it is the lane below's, the
64th lane hands over to the next wave through LDS and thread 511 to thread 0
of a second trip.  Which line of the text is which line of which window
depends on where the windows begin: `_walk` of the rounds test is that walk on
the CPU for texts of mapped lines, and span 0's first window begins at byte 0
with line 0 whatever its lines are.  Every case checks on the CPU, before
anything runs on the GPU, that its text has the shape it is named for.

Cases (all kept unless said otherwise):
  seams     24-byte lines, all mapped, reads of 1-3 lines: at every line
            first_line + 64j of a window, j = 1..12 (j = 8: threads 511 | 0 of
            two trips), a run starts in some window and continues in another;
            windows that are their span's first (the kFzBack bytes in front
            hold the line before) and windows that are not (mode 1).  Between
            them QNAMEs of 15, 16, 17, 24 and 40 bytes: equal; different at
            the last byte; 16 against 17 bytes that differ by byte 16 alone;
            17 bytes that differ at byte 16 only; 24 bytes that share 16; 40
            bytes (the tab loop's second piece)
  unmapped  32-byte lines in span 0's first window (line i = lane i % 64, 608
            lines: two trips): one unmapped line between two lines of a run
            and between two runs, at lane 63 and at lane 0 both ways; 64
            unmapped lines in a row inside a run and between two runs; a run
            across threads 511 | 0.  Behind it: runs that go on, or do not,
            behind 25-30 KB of unmapped lines (a window of unmapped lines
            only: mode 2; the run carried, nc > 0); a span whose kFzBack
            bytes in front hold no whole mapped line -- one line of 2 KB, or
            unmapped lines -- with the run going on in the span or not (the
            look-up in global memory)
  excluded  a subject map with one excluded name in runs of three lines
  beyond    handed back: a line names a subject beyond the subject map
  unknown   handed back: a line names a subject the dictionary does not hold;
            the six kernels that take the block list that one name, and the
            block through the one kernel afterwards is kept with equal counts
"""
import contextlib
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_dtok_rounds as R  # noqa: E402  (its helpers, as they are)
import test_gpu_dtok_scan as SC  # noqa: E402
import test_gpu_dtok_spans as S  # noqa: E402
from test_gpu_dtok_scan import device  # noqa: E402,F401  (the fixture)

TAIL = SC.TAIL
BLOCK, SPAN = S.BLOCK, S.SPAN
WIN, BACK, FWD, TILE = R.WIN, R.BACK, R.FWD, R.TILE
WAVE, THREADS = 64, R.THREADS
EXCLUDED = -4               # kLineExcluded


# ---- seams -----------------------------------------------------------------

def _qname_bundle(q, names, rng):
    """Mapped lines whose QNAMEs are told apart, or not, at known bytes."""
    def ln(name):
        return f'{name}\t0\t{rng.choice(names)}\t{TAIL}\n'
    k15, x16, y16 = f'K{q:014d}', f'L{q:015d}', f'J{q:015d}'
    p16, z40 = f'M{q:015d}', f'N{q:039d}'
    order = [k15, k15, k15[:-1] + 'x',                      # 15 bytes: equal; the last byte
             x16, x16, x16[:-1] + 'x',                      # 16 bytes: equal; byte 15
             y16, y16 + 'a', y16 + 'a', y16 + 'b',          # 16 | 17 by length; 17 equal; byte 16 alone
             p16 + '00000001', p16 + '00000001', p16 + '00000002',   # 24 bytes that share 16
             z40, z40, z40[:-1] + 'x', 'x' + z40[1:]]       # 40 bytes: equal; the last byte; byte 0
    assert [len(x) for x in order] == [15] * 3 + [16] * 4 + [17] * 3 + [24] * 3 + [40] * 4
    return ''.join(ln(x) for x in order)


def _seams_text(rng, names):
    out, n, q, special = [], 0, 0, 30000
    while n < BLOCK - 200:
        q += 1
        if n >= special:
            s = _qname_bundle(q, names, rng)
            special += 37000 + rng.randrange(4000)
        else:
            s = ''.join(R._line(f'q{q:09d}', rng.choice(names), 24)
                        for _ in range(rng.choice((1, 1, 2, 3))))
        out.append(s)
        n += len(s)
    return ''.join(out)


def _seam_lines(L, spans):
    """{j: {does line first_line + 64j start a run?}} over the windows of
    `spans`, first windows and others apart."""
    seen = {True: {}, False: {}}
    for s in spans:
        for w in R._walk(L, s):
            if not w['first'] or w['w0'] == 0:
                a, k0 = int(np.searchsorted(L.start, w['wpos'])), 0
            else:           # (line 0 is the rest of a line: the whole lines count from 1)
                a, k0 = int(np.searchsorted(L.start, w['w0'], 'right')), 1
            b = int(np.searchsorted(L.end, w['w1']))
            for j in range(1, 14):
                i = a + WAVE * j          # line k0 + 64j of the window: thread 64j
                if i < b and L.start[i] >= s * SPAN:
                    seen[w['first']].setdefault(j, set()).add(bool(L.flag[i]))
    return seen


def test_seams(device):  # noqa: F811
    names = device[4]
    text = _seams_text(random.Random('neighbour:seams'), names)
    L = R._Lines(text)
    seen = _seam_lines(L, range(256))
    for first in (True, False):
        for j in range(1, 13):      # (j = 8: thread 0 of the second trip)
            assert seen[first].get(j) == {True, False}, (first, j, seen[first].get(j))
    assert any(len(w) > 1 for w in (R._walk(L, s) for s in (3, 77, 200)))
    rows = text.split('\n')
    assert max(len(r.split('\t', 1)[0]) for r in rows) == 40
    R._both_kernels(device, 'neighbour_seams', text, True)


# ---- unmapped lines at known lanes -------------------------------------------

def _lanes_rows():
    """(QNAME, mapped) of 700 lines of 32 bytes: span 0's first window holds
    the first 608, line i at lane i % 64 of trip i // 512."""
    rows = [[f'r{i:07d}', True] for i in range(700)]

    def same(a, b):
        for i in range(a, b + 1):
            rows[i][0] = rows[a][0]

    def unmapped(a, b):
        for i in range(a, b + 1):
            rows[i][1] = False
    same(10, 12), unmapped(11, 11)              # one, inside a run
    unmapped(21, 21)                            # one, between two runs
    same(62, 64), unmapped(63, 63)              # at lane 63, inside a run
    unmapped(127, 127)                          # at lane 63, between two runs
    same(191, 193), unmapped(192, 192)          # at lane 0, inside a run
    unmapped(256, 256)                          # at lane 0, between two runs
    same(299, 364), unmapped(300, 363)          # 64 in a row, inside a run
    unmapped(400, 463)                          # 64 in a row, between two runs
    same(510, 513)                              # a run across threads 511 | 0
    same(575, 577)                              # ... and across lanes 63 | 0 of a second trip
    return rows


def _unmapped_text(rng, names):
    rows = _lanes_rows()
    head = ''.join(SC._line32(q, 0 if m else 4, rng.choice(names) if m else '*') for q, m in rows)
    assert len(head) == 32 * len(rows) and 512 * 32 < TILE + FWD < len(head)
    t = S._Text(rng, names)
    t.add(head)
    marks = []
    # a run, 25-30 KB of unmapped lines, and the run goes on behind them or another begins
    for span, off, nbytes, goes_on in ((50, 30000, 25 << 10, True), (90, 2000, 30 << 10, False),
                                       (130, 50000, 27 << 10, True), (170, 60000, 30 << 10, False)):
        t.plain_to(span * SPAN + off)
        q = t.run(2)
        t.unmapped(nbytes, q)
        t.run(3, q if goes_on else None)
    # nothing whole and mapped in the kFzBack bytes in front of a span
    for span, long_line, goes_on in ((200, True, True), (205, True, False), (210, False, True), (215, False, False)):
        t0 = span * SPAN
        if long_line:
            t.plain_to(t0 - 1900)
            begin, q = t.n, t.qname()
            t.add(R._line(q, rng.choice(names), t0 + 100 - t.n))
        else:
            t.plain_to(t0 - 1400)
            q = t.run(1)
            begin = t.n
            t.unmapped(t0 + 60 - t.n, q)
        marks.append((t0, begin, t.n, long_line))
        t.run(2, q if goes_on else None)
    t.plain_to(BLOCK - 256)
    return t.text(), marks


def test_unmapped(device):  # noqa: F811
    names = device[4]
    text, marks = _unmapped_text(random.Random('neighbour:unmapped'), names)
    rows = text.split('\n')
    f = [r.split('\t', 3) for r in rows[:700]]
    assert all(len(r) == 31 for r in rows[:700])
    mapped = [x[2] != '*' for x in f]
    q = [x[0] for x in f]
    lines_in_window = (TILE + FWD) // 32
    assert lines_in_window > THREADS + WAVE                     # (two trips)
    # inside a run / between two runs, at lanes 63 and 0, one and 64 in a row
    for i, n, inside in ((11, 1, True), (21, 1, False), (63, 1, True), (127, 1, False),
                         (192, 1, True), (256, 1, False), (300, 64, True), (400, 64, False)):
        assert not any(mapped[i:i + n]) and mapped[i - 1] and mapped[i + n], i
        assert (q[i - 1] == q[i + n]) == inside, i
    assert 63 % WAVE == 63 and 127 % WAVE == 63 and 192 % WAVE == 0 and 256 % WAVE == 0
    assert q[511] == q[512] and q[575] == q[576] and q[509] != q[510] and q[513] != q[514]
    assert sum(mapped) == 700 - 4 - 2 - 128
    raw = np.frombuffer(text.encode(), np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(raw == 10) + 1))
    for t0, begin, end, long_line in marks:
        # [begin, end) covers the kFzBack bytes in front of t0 and holds no whole mapped line but a first one of 2 KB
        assert begin < t0 - BACK - 16 and t0 < end < t0 + 200, (t0, begin, end)
        inside = starts[(starts > begin) & (starts < end)]
        if long_line:
            assert inside.size == 0
        else:
            assert all(text[s:s + 40].split('\t', 3)[2] == '*' for s in inside.tolist())
    R._both_kernels(device, 'neighbour_unmapped', text, True)


# ---- subjects ----------------------------------------------------------------

@contextlib.contextmanager
def _named_device():
    """test_gpu_dtok_scan.device, and the tokenizer's id of every name."""
    from woltka_amd import _native as nat
    tp, names = SC._names()
    th = tp['hier']
    with nat.Context(0) as ctx:
        ctx.set_tree(th.parent, th.last, th.rank_code)
        ctx.build_rank_table(0, th.rank_codes['genus'])
        ctx.counts_reserve(1 << 18)
        ctx.dtok_format('sam')
        jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0),
                nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)]
        tok = nat.Tokenizer(2)
        every = [k(s) for s in names for k in (str, SC._long16, SC._long29)]
        text = np.frombuffer(''.join(
            f'p{i}\t0\t{s}\t*\n' for i, s in enumerate(every)).encode(), np.uint8)
        status, n_lines = ctx.dtok_scan(tok, text, 0, text.size)
        assert status == 0 and n_lines == len(every)
        met = tok.new_subjects()
        assert sorted(met) == sorted(every)
        ctx.set_subjects(np.asarray([int(x[1:8]) for x in met], dtype=np.int32))
        assert ctx.words_begin(jobs, 0)
        assert ctx.dtok_emit()[0] == 0
        ctx.words_flush()
        ctx.counts_clear()
        try:
            yield (ctx, nat, jobs, tok, names), met
        finally:
            ctx.dtok_subject_map(None)
            ctx.tune('dtok_fused', 1)
            ctx.tune('dtok_fused_per_cu', 3)
            tok.close()


def _subjects_text(rng, names, special):
    """Plain reads; `special(t, i)` adds its lines at ten places (any lane)."""
    t = S._Text(rng, names)
    for i in range(10):
        t.plain_to((3 + 25 * i) * SPAN + 1000 + 4321 * i)
        special(t, i)
    t.plain_to(BLOCK - 256)
    return t.text()


def _through(dev, raw, fused):
    """One block through `dtok_scan_emit`: (status, lines, reads, records,
    cells, blocks kept and handed back, names met)."""
    ctx, nat, jobs, tok, _ = dev
    ctx.tune('dtok_fused_per_cu', 1)
    ctx.tune('dtok_fused', fused)
    assert ctx.words_begin(jobs, 0)
    before = ctx.dtok_fused_counts()
    status, n_lines, n_reads = ctx.dtok_scan_emit(tok, raw, 0, raw.size)
    after = ctx.dtok_fused_counts()
    return status, n_lines, n_reads, (after[0] - before[0], after[1] - before[1])


def test_excluded():
    with _named_device() as (dev, met):
        ctx, nat, jobs, tok, names = dev
        rng = random.Random('neighbour:excluded')
        ex = names[7]
        others = [s for s in names if s != ex]

        def special(t, i):
            q = t.qname()
            run = [rng.choice(others), rng.choice(others), rng.choice(others)]
            run[i % 3] = ex
            t.add(''.join(f'{q}\t{(0, 65, 129)[(i + k) % 3]}\t{s}\t{TAIL}\n' for k, s in enumerate(run)))
        text = _subjects_text(rng, others, special)
        table = np.arange(len(met), dtype=np.int32)
        table[met.index(ex)] = EXCLUDED
        ctx.dtok_subject_map(table)
        # the plain parser's grouping of the text without the dropped runs (align.py:47-115); the lines are the text's
        rows = text.split('\n')[:-1]
        gone = {r.split('\t', 1)[0] for r in rows if r.split('\t', 3)[2] == ex}
        assert len(gone) == 10
        kept = '\n'.join(r for r in rows if r.split('\t', 1)[0] not in gone) + '\n'
        _, reads, records, largest, short = SC._model(kept)
        assert len(rows) - kept.count('\n') == 30
        R._both_kernels(dev, 'neighbour_excluded', text, True, model=(len(rows), reads, records, largest, short))


def test_beyond_the_subject_map():
    with _named_device() as (dev, met):
        ctx, nat, jobs, tok, names = dev
        rng = random.Random('neighbour:beyond')
        last = met[-1]                          # (the one name the map below does not hold)
        others = [s for s in names if s != last[:8]]

        def special(t, i):
            if i == 4:
                t.add(f'{t.qname()}\t0\t{last}\t{TAIL}\n')
        text = _subjects_text(rng, others, special)
        assert text.count(f'\t{last}\t') == 1
        ctx.dtok_subject_map(np.arange(len(met) - 1, dtype=np.int32))
        raw = np.frombuffer(text.encode(), np.uint8)
        six = _through(dev, raw, 0)
        six_cells = _finish(dev, six)
        one = _through(dev, raw, 1)
        one_cells = _finish(dev, one)
        print('neighbour_beyond', six, one)
        assert six[3] == (0, 0) and one[3] == (0, 1)    # handed back
        assert six[:3] == one[:3]
        assert six_cells[0] == one_cells[0]
        assert np.array_equal(six_cells[1][0], one_cells[1][0]) and np.array_equal(six_cells[1][1], one_cells[1][1])


def _finish(dev, got):
    """The records of a block that `_through` left scanned or emitted:
    (records, cells); nothing of a block left to the host tokenizer."""
    ctx, nat, jobs, tok, _ = dev
    status, _, n_reads, _ = got
    if status == 0 and n_reads is None:
        assert ctx.dtok_emit()[0] == 0
    records = ctx.words_pending()[0]
    ctx.words_flush()
    cells = nat.canonical_counts(*ctx.counts_fetch())
    ctx.counts_clear()
    return records, cells


def test_unknown_subject():
    with _named_device() as (dev, met):
        ctx, nat, jobs, tok, names = dev
        rng = random.Random('neighbour:unknown')
        new = names[5] + '_new'

        def special(t, i):
            if i == 6:
                q = t.qname()
                t.add(f'{q}\t0\t{rng.choice(names)}\t{TAIL}\n{q}\t0\t{new}\t{TAIL}\n')
        text = _subjects_text(rng, names, special)
        assert text.count(f'\t{new}\t') == 1
        lines, reads, records, largest, short = SC._model(text)
        raw = np.frombuffer(text.encode(), np.uint8)
        # the one kernel first: it hands the block back, the six kernels scan it and list the one name
        status, n_lines, n_reads, blocks = _through(dev, raw, 1)
        assert blocks == (0, 1) and status == 0 and n_reads is None and n_lines == lines
        assert tok.new_subjects() == [new]
        ctx.words_flush()
        ctx.set_subjects(np.asarray([int(x[1:8]) for x in met + [new]], dtype=np.int32))
        assert ctx.words_begin(jobs, 0)
        st, n_reads, _ = ctx.dtok_emit()
        assert st == 0 and n_reads == reads
        first = _finish(dev, (1, None, None, None))
        assert first[0] == records
        # ... and now that the dictionary holds it, both ways as every other block
        R._both_kernels(dev, 'neighbour_unknown', text, True, model=(lines, reads, records, largest, short))
        again = _through(dev, raw, 1)
        assert again[3] == (1, 0) and again[:3] == (0, lines, reads)
        second = _finish(dev, again)
        assert second[0] == records
        assert np.array_equal(first[1][0], second[1][0]) and np.array_equal(first[1][1], second[1][1])
