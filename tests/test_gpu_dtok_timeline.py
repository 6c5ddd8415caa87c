"""The timeline of the one-kernel SAM tokenizer's measuring instance
(csrc/wk_dtok_fused.hpp, kFzTl*; `wk_dtok_fused_timeline`): with bit 4096 of
`wk_tune("fz_ablate")` thread 0 of every 64th workgroup stores the wall clock
at the kernel's entry and exit and at the phases of each window.  The bit
leaves nothing out: lines, reads, records and cells are the product's.  The
product's instance never writes the buffer."""
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
import test_gpu_dtok_exit as E  # noqa: E402  (`_totals_context`)
import test_gpu_dtok_instances as I  # noqa: E402  (`_plain_file`)

HEAD, PER, WINDOWS = 4, 12, 24      # (kFzTlHead, kFzTlPer, kFzTlWindows)
STAMPS = 10                         # a window's stamps; its info word behind them


def _pass(ctx, nat, job, tok, blocks, ablate):
    """The blocks through `dtok_scan_emit` with `fz_ablate` = ablate: per
    block (lines, reads, records) and the stamps behind it; the cells."""
    ctx.tune('fz_ablate', ablate)
    assert ctx.words_begin(job, 0)
    before = ctx.dtok_fused_counts()
    sums, stamps = [], []
    for raw in blocks:
        status, n_lines, reads = ctx.dtok_scan_emit(tok, raw, 0, raw.size)
        assert status == 0 and reads is not None, ablate
        sums.append((n_lines, reads, ctx.words_pending()[0]))
        stamps.append(ctx.dtok_fused_timeline())
    ctx.words_flush()
    after = ctx.dtok_fused_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (len(blocks), 0)
    cells = nat.canonical_counts(*ctx.counts_fetch())
    ctx.counts_clear()
    return sums, cells, stamps


def _check_rows(rows, every, grid, windows):
    """One row per sampled workgroup; its stamps rise; one record per window
    it walked (`windows`: how many that is, where the test knows)."""
    assert every == 64 and rows.shape == ((grid + 63) // 64, HEAD + WINDOWS * PER)
    for i, r in enumerate(rows.astype(np.int64)):
        entry, exit_, trips, wg = r[:HEAD]
        assert wg == i * every and entry > 0 and trips >= 1
        if windows is not None:
            assert trips == windows
        kept = int(min(trips, WINDOWS))
        w = r[HEAD:].reshape(WINDOWS, PER)
        seq = [entry] + w[:kept, :STAMPS].ravel().tolist() + [exit_]
        assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[0] < seq[-1], \
            (i, seq)
        assert not w[kept:].any(), 'a record beyond the windows walked'
        info = w[:kept, STAMPS]
        # (a span's first window is mode 0 and loads its own text; the last
        # one says that none follows)
        assert (info[0] & 31) == 0 and not (info[-1] & 32)
        assert all(x & 32 for x in info[:-1])


def test_timeline_of_three_blocks():
    """Three 256 KB blocks in one context (spans of 4 KB: 64 workgroups, one
    sampled, one window each): bit 4096 alone and with bit 2048 give the
    product's lines, reads, records and cells; the fetched stamps rise within
    a workgroup and carry one window record per trip; the product's instance,
    launched afterwards, gives its results again and leaves the buffer as the
    last stamping launch wrote it."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        job, tok, names = E._totals_context(ctx, nat)
        rng = random.Random('timeline:context')
        blocks = [np.frombuffer(
            I._plain_file(rng, names, 1 << 18).split('\n', 2)[2].encode(),
            np.uint8) for _ in range(3)]
        try:
            empty, every = ctx.dtok_fused_timeline()
            assert empty.size == 0 and every == 64  # (nothing has stamped yet)
            want = _pass(ctx, nat, job, tok, blocks, 0)
            for _, (rows, _) in zip(blocks, want[2]):
                assert rows.size == 0       # (the product's instance)
            last = None
            for ablate in (4096, 4096 + 2048):
                got = _pass(ctx, nat, job, tok, blocks, ablate)
                assert got[0] == want[0], ablate
                assert np.array_equal(got[1][0], want[1][0]) and \
                    np.array_equal(got[1][1], want[1][1]), ablate
                for raw, (rows, ev) in zip(blocks, got[2]):
                    grid = (raw.size + 4095) // 4096
                    _check_rows(rows, ev, grid, 1)
                last = got[2][-1][0]
            again = _pass(ctx, nat, job, tok, blocks, 0)
            assert again[0] == want[0]
            assert np.array_equal(again[1][0], want[1][0]) and \
                np.array_equal(again[1][1], want[1][1])
            for rows, _ in again[2]:
                assert np.array_equal(rows, last), 'the product wrote stamps'
        finally:
            ctx.tune('fz_ablate', 0)
            tok.close()


def test_timeline_of_spans_of_several_windows():
    """`dtok_fused_per_cu` = 1 and one block of 16 MB: spans of 64 KB, a
    sampled workgroup in every 64, four windows and more each.  With bit 4096
    alone every window behind a span's first has its text loaded a window
    ahead; with bit 2048 none has.  Lines, reads, records and cells are the
    product's both times."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        ctx.tune('dtok_fused_per_cu', 1)
        job, tok, names = E._totals_context(ctx, nat)
        rng = random.Random('timeline:spans')
        text = I._plain_file(rng, names, (1 << 24) - 4096).split('\n', 2)[2]
        blocks = [np.frombuffer(text.encode(), np.uint8)]
        assert blocks[0].size <= 1 << 24
        try:
            want = _pass(ctx, nat, job, tok, blocks, 0)
            for ablate in (4096 + 2048, 4096):
                got = _pass(ctx, nat, job, tok, blocks, ablate)
                assert got[0] == want[0], ablate
                assert np.array_equal(got[1][0], want[1][0]) and \
                    np.array_equal(got[1][1], want[1][1]), ablate
                rows, ev = got[2][0]
                assert rows.shape[0] >= 2
                span = (blocks[0].size + rows.shape[0] * ev - 1) // \
                    (rows.shape[0] * ev)
                _check_rows(rows, ev, rows.shape[0] * ev, None)
                for r in rows.astype(np.int64):
                    trips = int(r[2])
                    assert 4 <= trips <= WINDOWS, (trips, span)
                    info = r[HEAD:].reshape(WINDOWS, PER)[:trips, STAMPS]
                    ahead = [(x >> 4) & 1 for x in info]
                    assert ahead == [0] + [0 if ablate & 2048 else 1] * \
                        (trips - 1), (ablate, ahead)
        finally:
            ctx.tune('fz_ablate', 0)
            tok.close()
