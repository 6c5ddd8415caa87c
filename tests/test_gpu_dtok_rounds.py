"""Full staging rounds and the one-barrier emission of the one-kernel SAM
tokenizer (csrc/wk_dtok_fused.hpp, csrc/wk_dtok_rounds.hpp).

Compared as tests/test_gpu_dtok_scan.py compares, on its helpers: the same
block goes through `dtok_scan_emit` by the one kernel and by the six kernels;
status, lines, reads, records and cells are equal, exactly, and a kept block
also has the counts of `_model`.

Geometry: blocks of 16 MB at `dtok_fused_per_cu` = 1 -- 256 spans of 64 KB,
windows of 20 KB (1 280 chunks of 16 bytes).  Waves 0-3 of a workgroup take
192 chunks of a window each, waves 4-7 take 128: the seams are at chunks 192,
384, 576, 768, 896, 1 024, 1 152 and the window's end, 1 280.  Which chunk of
which window a byte of the text falls into depends on where the windows
begin, and a window begins at the last run start the window before saw:
`_walk` is that walk written out on the CPU for texts of mapped lines (no run
longer than a window), and every case checks with it, before anything runs on
the GPU, that its text has the shape it is named for.

Cases (kept = the one kernel keeps the block):
  seams              kept  lines of 23, 29, 31 and 37 bytes in random order, a
                           read each: in windows that are not their span's
                           first, newlines at the last byte of chunk 191, the
                           first of 192, the last of 767, the first of 768 and
                           the last of 1 279; about 680 owned lines a window,
                           two trips of the records loop
  open_end           kept  no last newline, and the text ends where a window
                           of the last span ends (w0 + 20 480): the byte that
                           stands for the newline is the chunk behind the
                           dealt ones, which is never text of the window
  open_end_minus_1   kept  ... one byte in front of that: the newline that is
                           not there is the last byte of chunk 1 279
  open_end_minus_16  kept  ... 16 bytes in front
  blank              back  1 024 newlines at window offsets 2 048-3 071 of span
                           0 (wave 0's third round) and a chunk of 9 newlines
                           (kDtokShortLine: empty lines)
  fill_1024          kept  one slice; a trip of span 0 ends with 1 024 records
                           in the buffer (kFzCap: not full)
  fill_1025          kept  ... with 1 025: the buffer leaves first
  fill_trips         kept  24-byte lines behind 19 KB of 60-byte ones: a
                           window of more than 512 owned lines whose second
                           trip finds the buffer full
  fill_skew          kept  four slices (40 608 subjects each): one fills again
                           and again, three hold a few records
  slices_1 .. _4     kept  1-4 slices (the ballots per slice and the packed
                           fill's fields), plain and with a subject map (the
                           identity: `--trim-sub`'s branch of the kernel)
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
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dtok_limits as D  # noqa: E402
import test_gpu_dtok_scan as SC  # noqa: E402  (its helpers, as they are)
import test_gpu_dtok_spans as S  # noqa: E402
from test_gpu_dtok_scan import device  # noqa: E402,F401  (the fixture)

TAIL = SC.TAIL
BLOCK, SPAN = S.BLOCK, S.SPAN
WIN, BACK, FWD, TILE = 20480, 1024, 3072, 16384     # kFzWin, kFzBack, kFzFwd, kFzTile
CAP, THREADS, LINES = 1024, 512, 1024               # kFzCap, kFzThreads, kFzLines
assert SPAN == 65536 and BLOCK == 256 * SPAN and SPAN > TILE


class _Lines:
    """Line starts, line ends (the newline, or n for an open last line) and
    run starts of a text whose lines are all mapped."""

    def __init__(self, text):
        raw = np.frombuffer(text.encode(), np.uint8)
        self.n = raw.size
        self.open_end = not text.endswith('\n')
        nl = np.flatnonzero(raw == 10)
        self.nl = nl
        self.end = np.append(nl, self.n) if self.open_end else nl
        self.start = np.concatenate(([0], nl + 1))[:self.end.size]
        rows = text.split('\n')[:self.end.size]
        q = [r.split('\t', 1)[0] for r in rows]
        assert all(r.split('\t', 3)[2] != '*' for r in rows[:2000])
        self.flag = np.array([True] + [a != b for a, b in zip(q[1:], q[:-1])])


def _walk(L, s):
    """The windows of span `s` as the kernel walks them: dicts of w0, wpos, w1,
    `first` and the owned lines [ka, kb) (indices into L.start)."""
    n = L.n
    text_end = n + (1 if L.open_end else 0)
    t0 = s * SPAN
    t1 = min(t0 + SPAN, n)
    span_w1 = min(t1 + FWD, text_end)
    wpos, mode, wide, out = max(t0 - BACK, 0), 0, False, []
    while True:
        w0 = wpos & ~15
        w1 = min(t0 + TILE + FWD if mode == 0 else w0 + WIN,
                 text_end if wide else span_w1)
        to_end, last_win = w1 == text_end, wide or w1 == span_w1
        a = int(np.searchsorted(L.start, max(wpos, t0)))
        b = int(np.searchsorted(L.end, w1))                 # lines [.., b) end in front of w1
        seen = int(np.searchsorted(L.end, w1) - np.searchsorted(L.end, wpos))
        assert seen + 1 <= LINES, ('too many lines in a window', s, wpos)
        idx = a + np.flatnonzero(L.flag[a:b])
        assert mode == 0 or (idx.size and idx[0] == a and L.start[a] == wpos)
        here = idx[L.start[idx] < t1]
        beyond = idx[L.start[idx] >= t1]
        o0 = int(here[0]) if here.size else None
        last = int(idx[-1]) if idx.size else None
        win = dict(w0=w0, wpos=wpos, w1=w1, first=mode == 0, ka=0, kb=0)
        out.append(win)
        if beyond.size:
            win['kb'] = int(beyond[0])
            win['ka'] = o0 if o0 is not None else win['kb']
            return out
        if to_end:
            win['kb'] = b
            win['ka'] = o0 if o0 is not None else b
            return out
        assert o0 is not None, ('no run start in a window', s, wpos)
        if last != o0 or L.start[last] > wpos:
            win['ka'], win['kb'] = o0, last
            wpos, mode, wide = int(L.start[last]), 1, last_win
        else:
            assert last_win and not wide, ('a run longer than a window', s, wpos)
            mode, wide = 1, True


def _hits(L, spans):
    """(chunk, byte) of every newline a window that is not its span's first
    looks at."""
    got = set()
    for s in spans:
        for w in _walk(L, s):
            if w['first']:
                continue
            p = L.nl[np.searchsorted(L.nl, w['wpos']):np.searchsorted(L.nl, w['w1'])] - w['w0']
            got.update(zip((p // 16).tolist(), (p % 16).tolist()))
    return got


def _fills(L, s):
    """The trips of span `s`: (window, trip, fill before, records) of the one
    slice -- every line is a read of one subject here."""
    fill, out = 0, []
    for wi, w in enumerate(_walk(L, s)):
        for ti, k0 in enumerate(range(w['ka'], w['kb'], THREADS)):
            new = min(w['kb'], k0 + THREADS) - k0
            out.append((wi, ti, fill, new))
            fill = new if fill + new > CAP else fill + new
    return out


def _line(q, name, length):
    """A mapped line of `length` bytes (newline included)."""
    head = f'{q}\t0\t{name}\t'
    assert len(head) + 1 <= length, (q, name, length)
    return head + 'x' * (length - len(head) - 1) + '\n'


class _Singles:
    """Reads of one line each, QNAMEs of ten bytes that never repeat."""

    def __init__(self, rng, names):
        self.rng, self.names, self.out, self.n, self.q = rng, names, [], 0, 0

    def add(self, s):
        self.out.append(s)
        self.n += len(s)

    def line(self, length, name=None):
        self.q += 1
        self.add(_line(f'q{self.q:09d}', name or self.rng.choice(self.names), length))

    def lines_to(self, size, lengths, name=None):
        while self.n < size:
            self.line(self.rng.choice(lengths), name)

    def text(self):
        return ''.join(self.out)


def _seams_text(rng, names):
    t = _Singles(rng, names)
    t.lines_to(BLOCK - 64, (23, 29, 31, 37))
    return t.text()


SEAMS = {(191, 15), (192, 0), (767, 15), (768, 0), (1279, 15)}


def _open_end_text(rng, names, short):
    """Plain reads; in the last span three runs of 300 lines, each across the
    end of a window, so that the span's fourth window begins at the third
    run's first line -- early enough for the text to end where that window
    does, `short` bytes in front of it, inside the block's last span."""
    t = S._Text(rng, names)
    t0 = 255 * SPAN
    for off in (15000, 30000, 43000):
        t.plain_to(t0 + off)
        begin = t.n
        t.run(300)
    stop = (begin & ~15) + WIN - short           # the text's end
    assert 255 * (SPAN - 16) + SPAN - 16 < stop <= BLOCK and t.n + 400 < stop
    while stop - t.n > 200:
        t.run(1)
    t.add(_line(t.qname(), names[1], stop - t.n + 1)[:-1])   # (no newline: the line ends at `stop`)
    assert t.n == stop
    return t.text()


def _blank_text(rng, names):
    t = _Singles(rng, names)
    t.lines_to(2048 - 80, (41, 45))
    t.line(2048 - t.n)                           # (its newline is byte 2 047)
    t.add('\n' * 1024)                           # window offsets 2 048-3 071 of span 0: wave 0's third round
    t.lines_to(3 * SPAN + 30000, (41, 45))
    t.line(32 + (1 - t.n) % 16)                  # (its newline is the first byte of a chunk)
    assert (t.n - 1) % 16 == 0
    t.add('\n' * 8)                              # ... and eight more in that chunk
    t.lines_to(BLOCK - 64, (41, 45))
    return t.text()


def _fill_text(rng, names, target):
    """One slice.  The first `m` lines are 38 bytes, the others 40: the m for
    which a trip of span 0 ends with `target` records in the buffer."""
    one = names[0]
    for m in range(0, 1100, 7):
        t = _Singles(rng, names)
        for _ in range(m):
            t.line(38, one)
        t.lines_to(SPAN + 2 * FWD, (40,), one)
        tail = t.n
        L = _Lines(t.text())
        L.n = BLOCK - 16                          # (as if the text went on: the block's size is known)
        if any(f + new == target for _, _, f, new in _fills(L, 0)):
            t.lines_to(BLOCK - 64, (40, 44))
            assert tail > SPAN + FWD
            return t.text()
    raise AssertionError('no text of that fill')


def _trips_text(rng, names):
    t = _Singles(rng, names)
    t.lines_to(TILE + FWD - 256, (60,))
    t.lines_to(3 * SPAN, (24,))
    t.lines_to(BLOCK - 64, (40, 44))
    return t.text()


def _sliced_text(rng, names, weights=None):
    """Reads of 1-3 lines over `names` (`weights`: per name)."""
    out, n, q = [], 0, 0
    pick = rng.choices(names, weights=weights, k=(BLOCK // 36) + 8)
    i = 0
    while n < BLOCK - 200:
        q += 1
        for _ in range((1, 1, 1, 2, 3)[q % 5]):
            ln = f'r{q:08d}\t0\t{pick[i]}\t{TAIL}\n'
            i += 1
            out.append(ln)
            n += len(ln)
    return ''.join(out)


def _big_names(n_subjects):
    _, small = SC._names()
    return [f'{small[i % len(small)]}{i:06d}' for i in range(n_subjects)]   # 14 bytes; [1:8]: the tree's subject


@contextlib.contextmanager
def _big_device(n_subjects):
    """test_gpu_dtok_scan.device with `n_subjects` subjects under one name
    each: subject i is name i (slice i // 40 608)."""
    from woltka_amd import _native as nat
    tp, _ = SC._names()
    names = _big_names(n_subjects)
    th = tp['hier']
    with nat.Context(0) as ctx:
        ctx.set_tree(th.parent, th.last, th.rank_code)
        ctx.build_rank_table(0, th.rank_codes['genus'])
        ctx.counts_reserve(1 << 20)
        ctx.dtok_format('sam')
        jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0),
                nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)]
        tok = nat.Tokenizer(2)
        text = np.frombuffer(''.join(
            f'p{i}\t0\t{s}\t*\n' for i, s in enumerate(names)).encode(), np.uint8)
        status, n_lines = ctx.dtok_scan(tok, text, 0, text.size)
        assert status == 0 and n_lines == len(names)
        met = tok.new_subjects()
        assert [x if isinstance(x, str) else x.decode() for x in met[:3]] == names[:3] and \
            len(met) == len(names)
        ctx.set_subjects(np.asarray([int(x[1:8]) for x in met], dtype=np.int32))
        assert ctx.words_begin(jobs, 0)
        assert ctx.dtok_emit()[0] == 0
        ctx.words_flush()
        ctx.counts_clear()
        try:
            yield ctx, nat, jobs, tok, names
        finally:
            ctx.dtok_subject_map(None)
            ctx.tune('dtok_fused', 1)
            ctx.tune('dtok_fused_per_cu', 3)
            tok.close()


def _both_kernels(dev, case, text, kept, model=None):
    """test_gpu_dtok_scan.test_block_through_both_kernels for a text of this
    module, at `dtok_fused_per_cu` = 1."""
    ctx, nat, jobs, tok, names = dev
    lines, reads, records, largest, short = model or SC._model(text)
    assert SPAN * 255 < len(text) <= BLOCK, len(text)        # (256 spans of 64 KB)
    assert largest <= SC.MAX_K and (short > 0) == (not kept), (case, largest, short)
    raw = np.frombuffer(text.encode(), np.uint8)
    ok, begin, stop, _ = nat.Tokenizer.sam_span(raw, True, False, 'sam')
    assert ok and begin == 0 and stop == raw.size
    ctx.tune('dtok_fused_per_cu', 1)
    got = {}
    for fused in (0, 1):
        ctx.tune('dtok_fused', fused)
        assert ctx.words_begin(jobs, 0)
        before = ctx.dtok_fused_counts()
        status, n_lines, n_reads = ctx.dtok_scan_emit(tok, raw, begin, stop)
        if status == 0 and n_reads is None:     # (scanned only: the second call)
            st, n_reads, _ = ctx.dtok_emit()
            assert st == 0, (case, fused)
        n_records = ctx.words_pending()[0]
        ctx.words_flush()
        after = ctx.dtok_fused_counts()
        cells = nat.canonical_counts(*ctx.counts_fetch())
        ctx.counts_clear()
        got[fused] = (status, n_lines if status == 0 else None,
                      n_reads if status == 0 else None, n_records, cells,
                      (after[0] - before[0], after[1] - before[1]))
    print('rounds', case, got[1][:4], got[1][5], 'model',
          (lines, reads, records, largest, short))
    assert got[0][5] == (0, 0), case
    assert got[0][:4] == got[1][:4], case
    assert np.array_equal(got[0][4][0], got[1][4][0]) and \
        np.array_equal(got[0][4][1], got[1][4][1]), case
    assert got[1][5] == ((1, 0) if kept else (0, 1)), case
    if kept:
        assert got[1][:4] == (0, lines, reads, records), case
    else:       # (the six kernels leave such a block to the host tokenizer)
        assert got[1][0] == 1, case


def test_seams(device):  # noqa: F811
    names = device[4]
    text = _seams_text(random.Random('rounds:seams'), names)
    L = _Lines(text)
    hits = _hits(L, range(0, 256, 3))
    assert SEAMS <= hits, sorted(SEAMS - hits)
    assert {b for _, b in hits} == set(range(16))           # (every byte of a chunk)
    assert any(w['kb'] - w['ka'] > THREADS for w in _walk(L, 7))   # (two trips)
    _both_kernels(device, 'seams', text, True)


@pytest.mark.parametrize('short', [0, 1, 16])
def test_open_end(device, short):  # noqa: F811
    names = device[4]
    text = _open_end_text(random.Random(f'rounds:open_end:{short}'), names, short)
    assert not text.endswith('\n')
    wins = _walk(_Lines(text), 255)
    assert any(not w['first'] and w['w0'] + WIN - short == len(text) for w in wins), \
        (len(text), [(w['w0'], w['w1']) for w in wins])
    _both_kernels(device, f'open_end_minus_{short}' if short else 'open_end', text, True)


def test_blank(device):  # noqa: F811
    names = device[4]
    text = _blank_text(random.Random('rounds:blank'), names)
    raw = np.frombuffer(text.encode(), np.uint8)
    per_chunk = (raw[:raw.size & ~15].reshape(-1, 16) == 10).sum(axis=1)
    assert (per_chunk[128:192] == 16).all() and per_chunk[127] == 1 and per_chunk[192] < 2   # (chunks of span 0's first window: w0 = 0)
    assert (per_chunk[192:] == 9).sum() == 1 and (per_chunk[192:] > 9).sum() == 0
    _both_kernels(device, 'blank', text, False)


@pytest.mark.parametrize('target', [CAP, CAP + 1])
def test_fill(device, target):  # noqa: F811
    names = device[4]
    text = _fill_text(random.Random(f'rounds:fill:{target}'), names, target)
    trips = _fills(_Lines(text), 0)
    assert any(f + new == target for _, _, f, new in trips), trips
    _both_kernels(device, f'fill_{target}', text, True)


def test_fill_trips(device):  # noqa: F811
    names = device[4]
    text = _trips_text(random.Random('rounds:fill_trips'), names)
    trips = _fills(_Lines(text), 0)
    # (a second trip that finds the buffer full, behind a first one that did not)
    assert any(ti == 1 and f <= CAP < f + new for _, ti, f, new in trips), trips
    _both_kernels(device, 'fill_trips', text, True)


def test_fill_skew():
    n = 4 * D.SLICE - 200
    with _big_device(n) as dev:
        names = dev[4]
        rng = random.Random('rounds:fill_skew')
        # (slice 2 takes the records; one line in 300 names a subject of another slice)
        main = names[2 * D.SLICE:2 * D.SLICE + 500]
        rare = [names[5], names[D.SLICE + 5], names[3 * D.SLICE + 5]]
        text = _sliced_text(rng, main + rare, [1.0] * len(main) + [0.6] * 3)
        rows = text.split('\n')[:-1]
        sl = np.array([int(r.split('\t', 3)[2][8:]) // D.SLICE for r in rows])
        per = np.bincount(sl, minlength=4)
        assert per[2] > 200 * CAP and all(256 < per[k] < 3000 for k in (0, 1, 3)), per
        _both_kernels(dev, 'fill_skew', text, True)


@pytest.mark.parametrize('mapped', [False, True], ids=['plain', 'map'])
@pytest.mark.parametrize('slices', [1, 2, 3, 4])
def test_slices(slices, mapped):
    n = slices * D.SLICE - 200
    with _big_device(n) as dev:
        ctx, names = dev[0], dev[4]
        rng = random.Random(f'rounds:slices:{slices}')
        # (subjects of every slice, those next to the slices' seams among them)
        pool = [names[i] for k in range(slices) for i in
                list(range(k * D.SLICE, k * D.SLICE + 40)) +
                list(range(min(n, (k + 1) * D.SLICE) - 40, min(n, (k + 1) * D.SLICE)))]
        text = _sliced_text(rng, pool)
        if mapped:
            ctx.dtok_subject_map(np.arange(n, dtype=np.int32))
        _both_kernels(dev, f'slices_{slices}_{"map" if mapped else "plain"}', text, True)
