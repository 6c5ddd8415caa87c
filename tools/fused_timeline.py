"""When do the workgroups of the one-kernel tokenizer (csrc/wk_dtok_fused.hpp)
do what?  The headline workload's text resident in HBM goes through the
measuring instance with bit 4096 of wk_tune "fz_ablate" (thread 0 of every
64th workgroup stores the 100 MHz wall clock at the phases of each window;
nothing is left out) -- once with bit 2048 as well (every window's text loaded
at the window's top, as before round 16) and once without (loaded a window
ahead, as the product's instance does).  For both: per phase the mean and the
spread over the sampled workgroups, windows and blocks; how long thread 0's
wave waits for its text per window; how far apart the sampled workgroups
reach the same window's top.

  python tools/fused_timeline.py [scale] [out]

`out`: the file the report goes to besides stdout (default
profiles/r16_fused_timeline.txt)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                    # noqa: E402
from woltka_amd import _native as nat           # noqa: E402

HEAD, PER = 4, 12       # (kFzTlHead, kFzTlPer)
BARRIER, TOP, TEXT, STAGED, NUMBERED, PROBED, LINES, AHEAD, PLANES, END, INFO = \
    range(11)
TICK_US = 0.01          # the wall clock runs at 100 MHz
PHASES = [
    ('top barrier -> loads issued (or found under way)', BARRIER, TOP),
    ('loads issued -> text arrived (the wait for the text)', TOP, TEXT),
    ('text -> staged (LDS stores, newline masks, scan, barrier)', TEXT, STAGED),
    ('staged -> numbered (line starts, barrier)', STAGED, NUMBERED),
    ('numbered -> probed (tabs, FLAG, RNAME, dictionary)', NUMBERED, PROBED),
    ('probed -> behind the line pass\'s barrier', PROBED, LINES),
    ('-> chain done, next loads issued (search, ownership)', LINES, AHEAD),
    ('-> behind the planes\' barrier (duplicate walk, ballots)', AHEAD, PLANES),
    ('-> window end (records, buffered emission)', PLANES, END),
]


def collect(ctx, wl, mask):
    """The stamps of every block of one pass (a pass before it warms up)."""
    ctx.tune('fz_ablate', mask)
    blocks = []
    for rep in range(2):
        ctx.words_begin(wl.jobs, 0)
        for view, begin, stop, hdr in wl.blocks:
            ctx.dtok_scan_emit(wl.tok, view, begin, stop)
            wl.tok.set_header_state(hdr)
            if rep:
                blocks.append(ctx.dtok_fused_timeline()[0].astype(np.int64))
        ctx.words_flush()
    ctx.tune('fz_ablate', 0)
    return blocks


def stats(x):
    x = np.asarray(x, dtype=np.float64) * TICK_US
    return (f'{x.mean():7.2f} us  sd {x.std():6.2f}  min {x.min():6.2f}  '
            f'p50 {np.median(x):6.2f}  max {x.max():6.2f}  (n {x.size})')


def report(tag, blocks, say):
    say(f'## {tag}')
    dur, entry, per, nxt, top_spread, windows, ahead = [], [], [], [], {}, [], 0
    for b in blocks:
        rows = b[b[:, 0] != 0]
        if not rows.size:
            continue
        t0 = rows[:, 0].min()
        dur.append(rows[:, 1].max() - t0)
        entry.append(rows[:, 0].max() - t0)
        tops = {}
        for r in rows:
            n = int(min(r[2], (r.size - HEAD) // PER))
            windows.append(int(r[2]))
            w = r[HEAD:HEAD + n * PER].reshape(n, PER)
            per.append(w)
            ahead += int(((w[:, INFO] >> 4) & 1).sum())
            nxt.extend((w[1:, BARRIER] - w[:-1, END]).tolist())
            for k in range(n):
                tops.setdefault(k, []).append(w[k, BARRIER] - t0)
        for k, v in tops.items():
            if len(v) > 1:
                top_spread.setdefault(k, []).append(max(v) - min(v))
    w = np.concatenate(per)
    say(f'blocks {len(blocks)}, sampled workgroups per block '
        f'{len(windows) // max(len(blocks), 1)}, windows per workgroup '
        f'{min(windows)}-{max(windows)}, window records {w.shape[0]} '
        f'({ahead} with their text loaded a window ahead)')
    say(f'kernel, first entry to last exit of the sampled: {stats(dur)}')
    say(f'entries of the sampled workgroups, last - first:  {stats(entry)}')
    for name, a, b in PHASES:
        say(f'  {name:58s} {stats(w[:, b] - w[:, a])}')
    for name, x in (("window end -> behind the next window's top barrier", nxt),
                    ('a whole window, top barrier -> end',
                     w[:, END] - w[:, BARRIER])):
        say(f'  {name:58s} {stats(x)}')
    first = w[:, INFO] & 15
    for name, sel in (('a span\'s first window', first == 0),
                      ('the windows behind it', first != 0)):
        if sel.any():
            say(f'  top barrier -> text arrived, {name:26s} '
                f'{stats(w[sel, TEXT] - w[sel, BARRIER])}')
    say('the same window\'s top over the sampled workgroups of a block, '
        'last - first (in phase: near 0):')
    for k in sorted(top_spread):
        say(f'  window {k:2d}: {stats(top_spread[k])}')
    return float(np.mean(dur)) * TICK_US, \
        float((w[:, TEXT] - w[:, BARRIER]).mean()) * TICK_US


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.1
    out = sys.argv[2] if len(sys.argv) > 2 else \
        os.path.join(ROOT, 'profiles', 'r16_fused_timeline.txt')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with nat.Context(0) as ctx:
        wl = bench.TextLcaWorkload(ctx, 1003, scale)
        say(f'# tools/fused_timeline.py {scale}: dtok_fused_measure_kernel, '
            f'fz_ablate 4096 + 2048 (loads at the top) and 4096 (loads a '
            f'window ahead); build {nat.build_id()}; blocks {len(wl.blocks)} '
            f'fused {wl.fused_blocks} back {wl.handed_back}; stamps of thread '
            f'0 of every 64th workgroup, 100 MHz wall clock (10 ns a tick)')
        res = {}
        for tag, mask in (('loads at the top (4096 + 2048)', 4096 + 2048),
                          ('loads a window ahead (4096)', 4096)):
            res[tag] = report(tag, collect(ctx, wl, mask), say)
        (d0, t0), (d1, t1) = res.values()
        say(f'## kernel {d0:.1f} -> {d1:.1f} us; top barrier -> text arrived per '
            f'window {t0:.2f} -> {t1:.2f} us')
        wl.blocks = []
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
