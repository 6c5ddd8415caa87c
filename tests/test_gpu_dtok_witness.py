"""The witness dealing of the one-kernel SAM tokenizer's line pass
(csrc/wk_dtok_fused.hpp, csrc/wk_dtok_neighbour.hpp): lanes 1..63 of a wave own
63 consecutive lines of a window, lane 0 sums up the line in front of them once
more, so every run start is decided inside a wave; a trip of the workgroup
covers 504 lines; and the search pass behind the line pass, with its barrier,
is taken only by a window in which some wave holds a line that its lane below
did not settle.

Compared as tests/test_gpu_dtok_scan.py, _rounds.py and _spans.py compare, on
their helpers: the same 16 MB block goes through `dtok_scan_emit` by the one
kernel and by the six kernels at `dtok_fused_per_cu` = 1 (256 spans of 64 KB,
windows of 20 KB); status, lines, reads, records and cells are equal, exactly,
and a kept block also has the counts of `_model`.

Place p = k - first_line of a window's line k is lane 1 + p % 63 of wave
(p % 504) // 63 in trip p // 504.  Which line of the text is which line of
which window depends on where the windows begin: `_walk` of the rounds test is
that walk on the CPU, and every case checks with it, before anything runs on
the GPU, that its text has the shape it is named for.

Cases (all kept):
  seams   lines of 24 bytes and more, all mapped, reads of 1-3 lines: at every
          place 63j, j = 1..8 (j = 8: thread 511's wave | the second trip's
          witness), a run starts in some window and continues in another, in
          windows that are their span's first and in windows that are not
          (mode 1).  At those places also QNAMEs of 15, 16, 17 and 24 bytes:
          equal to the one before, different at the last byte; and 17 bytes
          behind 16 that differ by byte 16 alone
  counts  lines of 40 and 41 bytes, a read each: windows of exactly 503, 504
          and 505 whole lines (one trip not full, full, and a second trip of
          one line)
  pass    lines of 32 bytes, a read each but for the shapes: windows with no
          undecided line next to windows whose only undecided line stands
          behind ONE unmapped line -- the last own line of waves 0, 3 and 7
          (lane 63; the witness of the wave behind it, or of the second trip,
          holds it), and lanes 1 and 63 of other waves; between two runs and
          inside a run.  And windows whose FIRST line is undecided (mode 2:
          lane 1 of wave 0, whose witness has no line, and nothing says the
          line starts a run): a stretch of unmapped lines that ends exactly
          where the whole first window of the span behind it ends, so that the
          window behind that one begins with a mapped line and nothing is
          carried into it (the look-up in global memory answers); and a run of
          two lines that begins a whole window and is followed by unmapped
          lines to exactly that window's end, so that the next window begins
          with a mapped line behind a carried run (the carried compare
          answers).  Both with the run going on at that line and with a new
          one beginning there.
          Whether a window skipped the search pass or took it does not show
          in any output: a build that took it in every window would pass here
          and only lose the speed.  What the case pins is that windows the
          kernel is meant to skip and windows it must not skip give the six
          kernels' results side by side.
"""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_dtok_lean as LN  # noqa: E402  (its walk with carried runs and windows without a run start)
import test_gpu_dtok_rounds as R  # noqa: E402  (its helpers, as they are)
import test_gpu_dtok_scan as SC  # noqa: E402
import test_gpu_dtok_spans as S  # noqa: E402
from test_gpu_dtok_scan import device  # noqa: E402,F401  (the fixture)

BLOCK, SPAN = S.BLOCK, S.SPAN
WIN, BACK, FWD, TILE = R.WIN, R.BACK, R.FWD, R.TILE
OWNERS, TRIP = 63, 504      # kFwOwners, kFwTrip


def _window_lines(L, w):
    """(a, b): the whole lines of window `w` of `_walk` are L's lines [a, b),
    line a at place 0."""
    if not w['first'] or w['w0'] == 0:
        a = int(np.searchsorted(L.start, w['wpos']))
    else:               # (line 0 is the rest of a line: the whole lines count from 1)
        a = int(np.searchsorted(L.start, w['w0'], 'right'))
    return a, int(np.searchsorted(L.end, w['w1']))


# ---- seams -----------------------------------------------------------------

WIDTHS = (15, 16, 17, 24)


def _seams_text(rng, names):
    """Reads of 1-3 lines.  Most QNAMEs have 10 bytes (lines of 24); one read
    in four takes a QNAME of 15, 16, 17 or 24 bytes, and the read behind it
    often the same QNAME but for its last byte, or a 16-byte one a 17th."""
    out, n, q, prev = [], 0, 0, None
    while n < BLOCK - 200:
        q += 1
        kind = rng.randrange(8)
        if prev is not None and kind < 2:
            name = prev[:-1] + ('x' if prev[-1] != 'x' else 'y')    # the last byte
        elif prev is not None and len(prev) == 16 and kind < 5:
            name = prev + 'a'                                       # byte 16 alone
        elif kind < 6:
            width = rng.choice(WIDTHS)
            name = f'{"KLMN"[WIDTHS.index(width)]}{q:0{width - 1}d}'
        else:
            name = f'q{q:09d}'
        prev = name if len(name) > 10 else None
        head = f'{name}\t0\t{rng.choice(names)}\t'
        s = (head + 'x' * max(0, 23 - len(head)) + '\n') * rng.choice((1, 1, 2, 3))
        out.append(s)
        n += len(s)
    return ''.join(out)


def test_seams(device):  # noqa: F811
    names = device[4]
    text = _seams_text(random.Random('witness:seams'), names)
    L = R._Lines(text)
    qn = [r.split('\t', 1)[0] for r in text.split('\n')[:L.start.size]]
    seen = {True: {}, False: {}}
    kinds = set()
    trips = set()
    for s in range(256):
        for w in R._walk(L, s):
            a, b = _window_lines(L, w)
            trips.add(-(-(b - a) // TRIP))
            for j in range(1, 9):
                i = a + OWNERS * j          # place 63j: lane 1 of wave j, or of wave 0 in the second trip
                if i >= b or L.start[i] < s * SPAN:
                    continue
                seen[w['first']].setdefault(j, set()).add(bool(L.flag[i]))
                p, c = qn[i - 1], qn[i]
                if p == c:
                    kinds.add((len(c), 'equal'))
                elif len(p) == len(c) and p[:-1] == c[:-1]:
                    kinds.add((len(c), 'last'))
                elif len(p) == 16 and len(c) == 17 and c[:16] == p:
                    kinds.add((17, 'byte 16 alone'))
    for first in (True, False):
        for j in range(1, 9):
            assert seen[first].get(j) == {True, False}, (first, j, seen[first].get(j))
    want = {(n, k) for n in WIDTHS for k in ('equal', 'last')} | {(17, 'byte 16 alone')}
    assert want <= kinds, sorted(want - kinds)
    assert trips == {1, 2}, trips
    R._both_kernels(device, 'witness_seams', text, True)


# ---- windows of 503, 504 and 505 lines --------------------------------------

def _counts_text(rng, names):
    """A read each; the share of 41-byte lines among the 40-byte ones drifts
    from span to span, so that windows hold 502-506 lines."""
    t = R._Singles(rng, names)
    while t.n < BLOCK - 64:
        share = 0.45 + 0.35 * ((t.n // SPAN) % 8) / 7.0
        t.line(41 if rng.random() < share else 40)
    return t.text()


def test_counts(device):  # noqa: F811
    names = device[4]
    text = _counts_text(random.Random('witness:counts'), names)
    L = R._Lines(text)
    held = {}
    for s in range(256):
        for w in R._walk(L, s):
            a, b = _window_lines(L, w)
            if w['w1'] - w['w0'] == WIN:        # (whole windows: not a span's last)
                held.setdefault(b - a, set()).add(w['first'])
    print('witness_counts', {k: len(v) for k, v in sorted(held.items())})
    for n in (TRIP - 1, TRIP, TRIP + 1):
        assert n in held, (n, sorted(held))
    R._both_kernels(device, 'witness_counts', text, True)


# ---- the search pass skipped and taken ----------------------------------------

class _LinesU:
    """`_Lines` of the rounds test for lines of 32 bytes of which some are
    unmapped: a run starts at a mapped line whose QNAME is not that of the
    mapped line before it."""

    def __init__(self, rows):
        n = len(rows)
        self.n = 32 * n
        self.open_end = False
        self.start = np.arange(n, dtype=np.int64) * 32
        self.end = self.start + 31
        self.nl = self.end
        self.mapped = np.array([m for _, m in rows])
        flag, last = np.zeros(n, bool), None
        for i, (q, m) in enumerate(rows):
            if m:
                flag[i] = q != last
                last = q
        self.flag = flag


#         span: (window of the span, place of the unmapped line, inside a run?)
SHAPES = {
    10: (1, 62, False), 11: (1, 62, True),          # the last own line of wave 0
    20: (1, 251, False), 21: (2, 251, True),        # ... of wave 3
    30: (1, 503, False), 31: (2, 503, True),        # ... of wave 7: the second trip's witness holds it
    40: (1, 126, False), 41: (1, 126, True),        # lane 1 of wave 2
    50: (2, 377, False), 51: (1, 377, True),        # lane 63 of wave 5
}
# A run of two lines at 60 000 of the span, then unmapped lines to exactly the end of the next span's first window: the
# window behind that one (mode 2, nothing carried) begins with a mapped line.  span: does the run go on at that line?
STRETCH = {170: True, 180: False}
# A run of two lines that begins the span's second window, then unmapped lines to exactly that window's end: it is put
# aside, and the window behind it (mode 2, two lines carried) begins with a mapped line.  span: does the run go on?
CARRIED = {190: True, 200: False}


def _pass_rows():
    rows = [[f'r{i:07d}', True] for i in range(BLOCK // 32 - 2)]
    at = {}
    for s, (win, p, inside) in SHAPES.items():
        # (a read each: the first window ends with the line at t0 + 19 424, every whole window holds 640 lines, and
        # each begins with the last whole line of the one before)
        i = (s * SPAN + TILE + FWD) // 32 - 1 + (win - 1) * (WIN // 32 - 1) + p
        rows[i][1] = False
        if inside:
            rows[i][0] = rows[i + 1][0] = rows[i - 1][0]
        at[s] = i
    first = {}      # span: (the mode-2 window's first line, lines carried into it, does the run go on there?)
    for s, goes_on in STRETCH.items():
        i, hi = (s * SPAN + 60000) // 32, ((s + 1) * SPAN + TILE + FWD) // 32
        first[s + 1] = (hi, 0, goes_on)
        rows[i + 1][0] = rows[i][0]
        for k in range(i + 2, hi):
            rows[k] = [rows[i][0], False]
        for k in range(hi, hi + 3):
            rows[k][0] = rows[i][0] if goes_on else rows[hi][0]
    for s, goes_on in CARRIED.items():
        i = (s * SPAN + TILE + FWD) // 32 - 1           # the second window's first line
        hi = i + WIN // 32
        first[s] = (hi, 2, goes_on)
        rows[i + 1][0] = rows[i][0]
        for k in range(i + 2, hi):
            rows[k] = [rows[i][0], False]
        for k in range(hi, hi + 3):
            rows[k][0] = rows[i][0] if goes_on else rows[hi][0]
    return rows, at, first


def _undecided(L, s, w):
    """The places of window `w` of span `s` that the lane below does not
    settle (QNAMEs of 8 bytes: an unmapped line in front, or no line)."""
    a, b = _window_lines(L, w)
    und = set()
    for i in range(a, b):
        if not L.mapped[i] or L.start[i] < s * SPAN:
            continue
        if i == a:
            if w['first'] and w['w0'] != 0:
                und.add(0)
        elif not L.mapped[i - 1]:
            und.add(i - a)
    return und, a


def test_pass_skipped_and_taken(device):  # noqa: F811
    names = device[4]
    rng = random.Random('witness:pass')
    rows, at, first = _pass_rows()
    L = _LinesU(rows)
    for s, (win, p, inside) in SHAPES.items():
        wins = R._walk(L, s)
        assert len(wins) == 4 and not wins[win]['first']
        und, a = _undecided(L, s, wins[win])
        i = at[s]
        assert i - a == p and und == {p + 1}, (s, i - a, und)       # the only undecided line of its window
        assert 1 + p % OWNERS in (1, 63)                            # lane 1 or lane 63
        assert L.mapped[i - 1] and L.mapped[i + 1] and (rows[i - 1][0] == rows[i + 1][0]) == inside
        assert bool(L.flag[i + 1]) == (not inside)
        other = wins[3 - win]                                       # the whole window next to it: nothing undecided
        assert not other['first'] and _undecided(L, s, other)[0] == set()
        # (a span's first window: its first whole line lies in front of t0 and is not asked, the others have a line below)
        assert _undecided(L, s, wins[0])[0] == set()
    assert {(p % TRIP) // OWNERS for _, p, _ in SHAPES.values() if p % OWNERS == 62} >= {0, 3, 7}
    # windows whose first line is undecided: mode 2, a mapped line at place 0 at or behind t0, nothing or two lines carried
    for s, (hi, nc, goes_on) in first.items():
        ws = LN._windows(L, s)
        assert not any(w['spill'] for w in ws) and not any(w['spill'] for w in LN._windows(L, s - 1))
        w = [w for w in ws if w['wpos'] == 32 * hi]
        assert len(w) == 1 and (w[0]['mode'], w[0]['nc']) == (2, nc), (s, [(x['wpos'], x['mode'], x['nc']) for x in ws])
        assert L.mapped[hi] and not L.mapped[hi - 1] and 32 * hi >= s * SPAN and 32 * hi % 16 == 0
        assert bool(L.flag[hi]) == (not goes_on) and L.mapped[hi + 1] and not L.flag[hi + 1]
        before = ws[ws.index(w[0]) - 1]
        assert before['aside'] == (nc != 0) and before['mode'] == (1 if nc else 0)
    text = ''.join(SC._line32(q, 0 if m else 4, rng.choice(names) if m else '*') for q, m in rows)
    assert len(text) == 32 * len(rows)
    R._both_kernels(device, 'witness_pass', text, True)
