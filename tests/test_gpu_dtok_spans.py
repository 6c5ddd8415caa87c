"""Spans of the one-kernel SAM tokenizer (csrc/wk_dtok_fused.hpp): a workgroup
walks one contiguous share of the block window by window instead of taking
16 KB tiles round-robin, each with its own halos.

Geometry: that of tests/test_gpu_dtok_exit.py -- `dtok_fused_per_cu` = 1 (256
workgroups) and blocks of 16 MB read untrimmed: 256 spans of 64 KB, four
windows each, the smallest shape with several windows per span.

Every case is checked twice.

`test_block_through_both_kernels`: one 16 MB block through `dtok_scan_emit`, by
the one kernel and by the six: lines, reads, records and cells are equal.  The
text is the block, so the test knows where the spans lie and states whether the
one kernel keeps the block:
  kept          plain, with and without a last newline; runs of 120 and 420
                lines (5 and 17 KB, both more than kFzFwd) inside a span and
                across a span's end (the wide look from the run's start);
                stretches of unmapped lines of 25-30 KB, longer than a
                window -- at the start of the text, inside a span, across a
                span's end and over the whole first window of the next span
                -- with the run in front going on behind the stretch (one
                run: its lines are carried from window to window) or a new
                one beginning there; lines of 1.1-3 KB; a block of 1 MB whose
                last span is shorter than 4 KB and ends without a newline
  handed back   a run of 900 lines (more lines than are carried); more than
                kFzLines lines in a window.
`test_file_through_three_routes`: the same shapes in the 16 MB block of a
sample of 23.5 MB (the layout of test_buffers_that_fill_before_the_last_tile:
a small first sample that names every subject, then blocks of 1, 4 and 16 MB
and a rest; the shapes stay clear of the 4 MB block and of the rest, whose
spans are single windows), through the one kernel, the six kernels
(WOLTKA_NO_FUSED=1) and the host tokenizer (WOLTKA_NO_DTOK=1, pinned to the
reference by the CPU tests): same tables, same log, and the second sample's
blocks kept and handed back say what the case is for.

`test_short_blocks_and_an_open_end`: blocks of 256 KB at the default launch --
64 spans of 4 KB for 768 workgroups -- of a text whose last byte is no
newline."""
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
import test_gpu_dtok_exit as X  # noqa: E402  (its helpers, as they are)

TAIL = X.TAIL
BLOCK = 1 << 24
SPAN = 1 << 16              # max(4096, round_up_16(ceil(BLOCK / 256)))
UNMAPPED = '\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n'


class _Text:
    """Reads of 1-3 lines of 36-45 bytes (QNAMEs of 2-14 bytes: run starts fall
    on every offset mod 16) up to a given size, and the cases' shapes."""

    def __init__(self, rng, subjects):
        self.rng, self.subjects = rng, subjects
        self.out, self.n, self.q = [], 0, 0

    def add(self, s):
        self.out.append(s)
        self.n += len(s)

    def qname(self):
        self.q += 1
        return 'q' + 'x' * (self.q % 7) + str(self.q)

    def run(self, k, q=None):
        """k lines of one QNAME, at most six distinct subjects."""
        q = q or self.qname()
        pool = self.rng.sample(self.subjects, min(6, 1 + k // 2))
        self.add(''.join(f'{q}\t0\t{self.rng.choice(pool)}\t{TAIL}\n'
                         for _ in range(k)))
        return q

    def plain_to(self, size):
        while self.n < size:
            self.run(self.rng.choice([1, 1, 1, 2, 3]))

    def unmapped(self, nbytes, q):
        ln = q + UNMAPPED
        self.add(ln * (nbytes // len(ln) + 1))

    def text(self):
        return ''.join(self.out)


def _dense15(rng, size, subjects):
    """Lines of 15 bytes (the context's subjects have eight), runs of 1-4:
    about 1 360 lines in 20 KB."""
    out, n, q = [], 0, 0
    while n < size:
        q += 1
        ln = f'{"abcdefghijklmnopqrstuvwxyz"[q % 26]}{q % 7}\t0\t' \
             f'{rng.choice(subjects)}\t\n' * rng.choice([1, 2, 4])
        out.append(ln)
        n += len(ln)
    return ''.join(out)


def _body(case, rng, subjects, size, whole_block, dense=None):
    """`size` bytes (a read more or less) of the case's text.  `whole_block`:
    the text is the block, `at(span, offset)` is that place in that span of
    the block; else the spans lie where the reader's cuts put them."""
    t = _Text(rng, subjects)

    def at(span, off):
        t.plain_to(span * SPAN + off)

    if case in ('plain', 'plain_open', 'open_short'):
        pass
    elif case in ('runs', 'runs_900'):
        # inside a span: early, late, and in its last window
        for span, off, k in ((3, 8000, 420), (5, 45000, 120), (40, 30000, 420),
                             (41, 100, 120), (100, 44000, 420),
                             (150, 60000, 120)):
            at(span, off)
            t.run(k)
        if whole_block:
            # across a span's end, more than kFzFwd behind it: the span's
            # second look, from the run's start
            for span, off, k in ((180, 65000, 120), (200, 60000, 420),
                                 (220, 50000, 420)):
                at(span, off)
                t.run(k)
        if case == 'runs_900':
            at(230, 8000)
            t.run(900)
    elif case == 'unmapped_first':
        assert whole_block
        t.unmapped(27 << 10, 'nobody')
    elif case in ('unmapped_same', 'unmapped_new'):
        # inside a span; across a span's end; over the next span's whole
        # first window (that span steps over it and looks the run up)
        for span, off, nbytes in ((50, 30000, 25 << 10), (90, 2000, 30 << 10),
                                  (130, 50000, 27 << 10),
                                  (170, 60000, 30 << 10)):
            at(span, off)
            q = t.run(2)
            t.unmapped(nbytes, q)
            t.run(3, q if case == 'unmapped_same' else None)
    elif case == 'long_lines':
        t.add(D._long_lines(rng, size - (128 << 10), subjects, head=False,
                            huge=False))
    elif case == 'dense':
        at(80, 20000)
        t.add(dense(rng, 24 << 10))
    else:
        raise ValueError(case)
    t.plain_to(size)
    return t.text()[:-1] if case in ('plain_open', 'open_short') else t.text()


#        case: (kept by the one kernel, what ROUTES must say)
CASES = {
    'plain': (True, 'none_back'),
    'plain_open': (True, 'none_back'),
    'open_short': (True, None),
    'runs': (True, 'none_back'),
    'runs_900': (False, 'some_back'),
    'unmapped_first': (True, None),
    'unmapped_same': (True, 'none_back'),
    'unmapped_new': (True, 'none_back'),
    'long_lines': (True, 'none_back'),
    'dense': (False, 'some_back'),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_block_through_both_kernels(case):
    """Lines, reads, records (`words_pending`) and cells of one 16 MB block,
    as test_block_totals_equal_the_six_kernels checks them, and whether the
    one kernel kept the block (see the module's docstring)."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        ctx.tune('dtok_fused_per_cu', 1)
        job, tok, names = X._totals_context(ctx, nat)
        try:
            _both_kernels(ctx, nat, job, tok, names, case)
        finally:
            ctx.tune('dtok_fused', 1)
            tok.close()


def _both_kernels(ctx, nat, job, tok, names, case):
    rng = random.Random(f'spans:{case}')
    if case == 'open_short':
        # (256 spans of 4112 bytes, the last one of about 1 000)
        text = _body(case, rng, names, 255 * 4112 + 900, True)
        span = max(4096, (-(-len(text) // 256) + 15) & ~15)
        assert span == 4112 and -(-len(text) // span) == 256
        assert 0 < len(text) - 255 * span < 4096
    else:
        text = _body(case, rng, names, BLOCK - 256, True,
                     dense=lambda r, n: _dense15(r, n, names))
        assert SPAN * 256 - 16 * 256 < len(text) <= SPAN * 256   # (64 KB)
    raw = np.frombuffer(text.encode(), np.uint8)
    ok, begin, stop, _ = nat.Tokenizer.sam_span(raw, True, False, 'sam')
    assert ok and begin == 0 and stop == raw.size
    got = {}
    for fused in (0, 1):
        ctx.tune('dtok_fused', fused)
        assert ctx.words_begin(job, 0)
        before = ctx.dtok_fused_counts()
        status, n_lines, reads = ctx.dtok_scan_emit(tok, raw, begin, stop)
        assert status == 0, (case, fused)
        if reads is None:               # (scanned only: the second call)
            st, reads, _ = ctx.dtok_emit()
            assert st == 0, (case, fused)
        records = ctx.words_pending()[0]
        ctx.words_flush()
        after = ctx.dtok_fused_counts()
        cells = nat.canonical_counts(*ctx.counts_fetch())
        ctx.counts_clear()
        got[fused] = (n_lines, reads, records, cells,
                      (after[0] - before[0], after[1] - before[1]))
    print('spans', case, got[1][:3], got[1][4])
    assert got[0][4] == (0, 0), case
    assert got[0][:3] == got[1][:3], case
    assert np.array_equal(got[0][3][0], got[1][3][0]) and \
        np.array_equal(got[0][3][1], got[1][3][1]), case
    assert got[1][0] == text.count('\n') + (not text.endswith('\n')), case
    assert got[1][4] == ((1, 0) if CASES[case][0] else (0, 1)), case


@pytest.mark.parametrize('case', sorted(c for c in CASES if CASES[c][1]))
def test_file_through_three_routes(tmp_path, monkeypatch, case):
    """The case's shape in the 16 MB block of the second sample (from 5.5 MB to
    20.5 MB of 23.5 MB), plain text around it; three routes, equal tables and
    logs.  The second sample's first block is scanned the two-call way, the
    three behind it go to the one kernel."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', BLOCK)
    monkeypatch.setattr(device_text, 'TRIM', False)
    X._per_cu(monkeypatch, 1)
    rng = random.Random(f'spans:file:{case}')
    subjects = [f'g{i:06d}' for i in range(90)]
    lead = _Text(rng, subjects)
    lead.add(D.HEADER)
    lead.plain_to(5 << 20 | 1 << 19)
    body = _body(case, rng, subjects, 15 << 20, False,
                 dense=lambda r, n: D._dense(r, n, None, head=False))
    tail = _Text(rng, subjects)
    tail.q = 1 << 24
    tail.plain_to(3 << 20)
    end = tail.text()[:-1] if case == 'plain_open' else tail.text()
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(D.HEADER +
                                  D._prologue(D.DENSE_SUBJECTS + subjects))
    (indir / 'S2.sam').write_text(lead.text() + body + end)
    per_file = X._spy_counts(monkeypatch)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    tables, routes = X._three_routes(tmp_path, monkeypatch, **kw)
    # (the second sample of the one-kernel run)
    fused, back = [x - y for x, y in zip(per_file[2], per_file[1])]
    print('routes', case, routes, per_file)
    assert routes.get('host_block', 0) == 0, routes
    assert routes['dtok_fused'] > 0 and fused > 0, (routes, per_file)
    want = CASES[case][1]
    if want == 'none_back':
        assert (fused, back) == (3, 0), (routes, per_file)
    elif want == 'some_back':
        assert back > 0, (routes, per_file)


def test_short_blocks_and_an_open_end(tmp_path, monkeypatch):
    """Blocks of 256 KB at the default launch: 64 spans of 4 KB, fewer than
    workgroups.  The file's last byte is no newline.  (A last span shorter
    than 4 KB: `open_short` above, where the test knows the block.)"""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 18)
    monkeypatch.setattr(device_text, 'TRIM', False)
    rng = random.Random('spans:open_end')
    subjects = [f'g{i:06d}' for i in range(90)]
    t = _Text(rng, subjects)
    t.add(D.HEADER + D._prologue(subjects))
    t.plain_to(900_000)
    text = t.text().rstrip('\n')
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(text)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    tables, routes = X._three_routes(tmp_path, monkeypatch, **kw)
    print('routes open_end', routes)
    assert routes['dtok_fused'] > 0, routes
    assert routes.get('dtok_fused_back', 0) == 0, routes
    assert routes.get('host_block', 0) == 0, routes
