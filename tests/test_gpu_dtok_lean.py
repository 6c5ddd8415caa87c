"""Runs put aside and carried from window to window by the one-kernel SAM
tokenizer (csrc/wk_dtok_fused.hpp), at the windows where a split of the window
loop would switch bodies: a lean body (nothing carried: no carried lines, no
copy, no carried compare, unsigned line numbers) in front of the first window
that puts a run aside and the general body behind it.  That split was built
and measured and is not in the kernel: it gained
nothing.  These cases stay as what any such split has to keep.

Compared as tests/test_gpu_dtok_scan.py, _rounds.py and _spans.py compare, on
their helpers: the same 16 MB block goes through `dtok_scan_emit` by the one
kernel and by the six kernels at `dtok_fused_per_cu` = 1 (256 spans of 64 KB,
windows of 20 KB); status, lines, reads, records and cells are equal, exactly,
and a kept block also has the counts of `_model`.

`_windows` is the kernel's walk of a span written out on the CPU, carried runs
and windows without a run start included (the rounds test's `_walk` stops at
those): per window, whether it put a run aside, how many lines were carried
into it, and how it was entered.  Every case checks with it, before anything
runs on the GPU, that its text has the shape it is named for.

One block, kept -- a shape per span, plain reads of 1-3 lines between them:
  first     the text begins with a run of two lines and 25 KB of unmapped
            lines: put aside in span 0's first window (the only first window
            that can: it begins at a line)
  third     a run put aside in its span's third window
  goes_on   a run put aside in a span's second window, carried into the third,
            where it ends (another run begins behind the unmapped lines); the
            span goes on for two more windows and more
  same      ... the run goes on behind the unmapped lines and ends there
  twice     two carried runs in one span
  c256      a carried run of 256 mapped lines (kFzCarry: kept)
  never     the spans between them never put a run aside
A second block, handed back: a carried run of 257 mapped lines.
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
import test_gpu_dtok_rounds as R  # noqa: E402  (its helpers, as they are)
import test_gpu_dtok_scan as SC  # noqa: E402
import test_gpu_dtok_spans as S  # noqa: E402
from test_gpu_dtok_scan import device  # noqa: E402,F401  (the fixture)

BLOCK, SPAN = S.BLOCK, S.SPAN
WIN, BACK, FWD, TILE = R.WIN, R.BACK, R.FWD, R.TILE
CARRY = 256                 # kFzCarry


class _Rows:
    """Line starts, ends, mapped lines and run starts of a text with unmapped
    lines: a run starts at a mapped line whose QNAME is not that of the mapped
    line before it."""

    def __init__(self, text):
        assert text.endswith('\n')
        raw = np.frombuffer(text.encode(), np.uint8)
        self.n = raw.size
        self.end = np.flatnonzero(raw == 10)
        self.start = np.concatenate(([0], self.end[:-1] + 1))
        rows = text.split('\n')[:-1]
        f = [r.split('\t', 3) for r in rows]
        self.mapped = np.array([x[2] != '*' for x in f])
        flag, last = np.zeros(len(rows), bool), None
        for i, x in enumerate(f):
            if self.mapped[i]:
                flag[i] = x[0] != last
                last = x[0]
        self.flag = flag


def _windows(L, s):
    """The windows of span `s` as the kernel walks them: dicts of wpos, `mode`
    (0: the span's first, 1: begins with a run start, 2: not known), `nc`
    (mapped lines carried into it), `aside` (it puts its run aside), and
    `spill` (it hands the block back)."""
    n = text_end = L.n
    t0 = s * SPAN
    t1 = min(t0 + SPAN, n)
    span_w1 = min(t1 + FWD, text_end)
    wpos, mode, wide, nc, out = max(t0 - BACK, 0), 0, False, 0, []
    while True:
        assert len(out) < 64
        w0 = wpos & ~15
        w1 = min(t0 + TILE + FWD if mode == 0 else w0 + WIN, text_end if wide else span_w1)
        to_end, last_win = w1 == text_end, wide or w1 == span_w1
        a = int(np.searchsorted(L.start, wpos if mode != 0 or w0 == 0 else w0 + 1))
        b = int(np.searchsorted(L.end, w1))             # lines [a, b) are whole
        assert int(np.searchsorted(L.end, w1) - np.searchsorted(L.end, wpos)) + 1 <= R.LINES
        trail = int(L.end[b - 1]) + 1 if b > 0 and L.end[b - 1] >= wpos else wpos
        idx = a + np.flatnonzero(L.flag[a:b] & (L.start[a:b] >= t0))
        here, beyond = idx[L.start[idx] < t1], idx[L.start[idx] >= t1]
        o0 = int(here[0]) if here.size else None
        last = int(idx[-1]) if idx.size else None
        win = dict(wpos=wpos, mode=mode, nc=nc, aside=False, spill=False)
        out.append(win)
        if beyond.size or to_end:
            return out
        if o0 is not None and (nc or last != o0 or L.start[last] > wpos):
            wpos, mode, wide, nc = int(L.start[last]), 1, last_win, 0
        elif o0 is not None and last_win and not wide:
            mode, wide = 1, True
        elif o0 is not None or nc:
            win['aside'] = True
            nc += int(L.mapped[a:b].sum())
            if nc > CARRY or trail <= wpos:
                win['spill'] = True
                return out
            wpos, mode, wide = trail, 2, last_win
        elif not last_win:
            if trail <= wpos:
                win['spill'] = True
            if not (wpos < trail < t1):
                return out
            wpos, mode = trail, 2
        else:
            return out


#       case: (span, offset of the run in it)
PLACES = {'third': (20, 36000), 'goes_on': (40, 200), 'same': (60, 200),
          'twice': (80, 3000), 'c256': (100, 30000)}
TWICE_SECOND = 33000


def _lean_text(rng, names, lines_carried):
    t = S._Text(rng, names)
    # first: put aside in span 0's first window
    q = t.run(2)
    t.unmapped(25 << 10, q)
    t.run(2, q)

    def at(case):
        span, off = PLACES[case]
        t.plain_to(span * SPAN + off)

    at('third')
    q = t.run(2)
    t.unmapped(22 << 10, q)
    t.run(1, q)
    at('goes_on')
    q = t.run(2)
    t.unmapped(22 << 10, q)
    at('same')
    q = t.run(2)
    t.unmapped(22 << 10, q)
    t.run(3, q)
    at('twice')
    q = t.run(3)
    t.unmapped(21 << 10, q)
    t.plain_to(PLACES['twice'][0] * SPAN + TWICE_SECOND)
    q = t.run(2)
    t.unmapped(21 << 10, q)
    t.run(2, q)
    at('c256')
    q = t.run(lines_carried)
    t.unmapped(12 << 10, q)
    t.run(2, q)
    t.plain_to(BLOCK - 256)
    return t.text()


def test_switch_of_loops(device):  # noqa: F811
    names = device[4]
    text = _lean_text(random.Random('lean:kept'), names, CARRY)
    L = _Rows(text)
    walks = {s: _windows(L, s) for s in range(256)}
    assert not any(w['spill'] for ws in walks.values() for w in ws)
    aside = {s: [(i, w['mode'], w['nc']) for i, w in enumerate(ws) if w['aside']] for s, ws in walks.items()}
    # first: span 0's first window, which begins at a line
    assert aside[0] == [(0, 0, 0)] and walks[0][1]['mode'] == 2 and walks[0][1]['nc'] == 2
    # third: the span's third window, nothing carried in front of it
    s = PLACES['third'][0]
    assert aside[s] == [(2, 1, 0)] and walks[s][3]['nc'] == 2
    # goes_on / same: put aside in the second window, ended in the third, and the span goes on for two more at least
    for case in ('goes_on', 'same'):
        s = PLACES[case][0]
        ws = walks[s]
        assert aside[s] == [(1, 1, 0)] and (ws[2]['mode'], ws[2]['nc']) == (2, 2), (case, aside[s])
        assert len(ws) >= 5 and all(w['nc'] == 0 and w['mode'] == 1 for w in ws[3:]), (case, len(ws))
    # twice: two runs put aside in one span, the second behind a carried one
    s = PLACES['twice'][0]
    assert [x[1:] for x in aside[s]] == [(1, 0), (1, 0)] and aside[s][1][0] >= aside[s][0][0] + 2, aside[s]
    # c256: exactly kFzCarry lines carried
    s = PLACES['c256'][0]
    assert len(aside[s]) == 1 and walks[s][aside[s][0][0] + 1]['nc'] == CARRY, aside[s]
    # never: no other span puts a run aside, the neighbours of those that do among them
    carrying = {s for s, x in aside.items() if x}
    assert carrying == {0} | {p[0] for p in PLACES.values()}, sorted(carrying)
    assert all(len(walks[s]) >= 4 for s in range(256) if s not in carrying)
    R._both_kernels(device, 'lean_kept', text, True)


def test_257_carried_lines_are_handed_back(device):  # noqa: F811
    ctx, nat, jobs, tok, names = device
    text = _lean_text(random.Random('lean:back'), names, CARRY + 1)
    L = _Rows(text)
    s = PLACES['c256'][0]
    ws = _windows(L, s)
    assert ws[-1]['spill'] and ws[-1]['aside'] and ws[-1]['mode'] == 1, ws[-1]
    lines, reads, records, largest, short = SC._model(text)
    assert short == 0 and largest <= SC.MAX_K
    raw = np.frombuffer(text.encode(), np.uint8)
    ctx.tune('dtok_fused_per_cu', 1)
    got = {}
    for fused in (0, 1):
        ctx.tune('dtok_fused', fused)
        assert ctx.words_begin(jobs, 0)
        before = ctx.dtok_fused_counts()
        status, n_lines, n_reads = ctx.dtok_scan_emit(tok, raw, 0, raw.size)
        if status == 0 and n_reads is None:     # (scanned only: the second call)
            st, n_reads, _ = ctx.dtok_emit()
            assert st == 0, fused
        n_records = ctx.words_pending()[0]
        ctx.words_flush()
        after = ctx.dtok_fused_counts()
        cells = nat.canonical_counts(*ctx.counts_fetch())
        ctx.counts_clear()
        got[fused] = (status, n_lines, n_reads, n_records, cells, (after[0] - before[0], after[1] - before[1]))
    print('lean_back', got[1][:4], got[1][5])
    assert got[0][5] == (0, 0) and got[1][5] == (0, 1)      # handed back
    assert got[0][:4] == got[1][:4] == (0, lines, reads, records)
    assert np.array_equal(got[0][4][0], got[1][4][0]) and np.array_equal(got[0][4][1], got[1][4][1])
