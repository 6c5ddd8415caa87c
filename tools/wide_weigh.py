#!/usr/bin/env python3
"""The wide layout of the weighted histogram (csrc/wk_weigh_wide.hpp) by itself:
kernel-family times per flush over resident packed words.

    python tools/wide_weigh.py [--records 50000000] [--runs 5] [--out FILE]

50 M packed words (reads of 1..16 hits) are made with numpy, appended once and
flushed again and again under `wk_tune "words_keep"`; every flush is timed per
kernel family with the context's event timers ("weigh_wide_part": count, scan
and scatter; "weigh_wide": the histogram; "classify": the team layout's
histogram; "weigh_merge").  Subject tables of 1 299 456 (the last one the team
layout takes), 1 299 457, 4 M and 2^23 subjects; the subject of a record drawn

  zipf      Zipf-like over the order of first appearance, P(i) ~ 1 / (i + 1.5)
            (index 0 the hottest),
  uniform   uniformly,
  hot_tail  the Zipf head at the highest indices (a late sample's subjects).

At 1 299 456 subjects the default team layout and the wide one ("weigh_wide"
= 1) take turns over the same resident words, and their count tables are
compared once.  Ranges over the runs are written, not means alone.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from woltka_amd import _native as nat  # noqa: E402

BINS = 40608
TABLES = (32 * BINS, 32 * BINS + 1, 4_000_000, 1 << 23)
DISTS = ('zipf', 'uniform', 'hot_tail')


def read_fields(rng, n_records):
    """Position and size fields of n_records words: reads of 1 hit (half) or
    2..16."""
    k = np.where(rng.random(n_records // 2 + 16) < 0.5, 1,
                 rng.integers(2, 17, n_records // 2 + 16)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(k)])
    n_reads = int(np.searchsorted(off, n_records, side='right')) - 1
    n = int(off[n_reads])
    size = np.repeat(k[:n_reads], k[:n_reads])
    pos = np.arange(n, dtype=np.int64) - np.repeat(off[:n_reads], k[:n_reads])
    return ((pos << 23) | (size << 27)).astype(np.uint32), n_reads


def subjects(rng, dist, n_subjects, n):
    if dist == 'uniform':
        return rng.integers(0, n_subjects, n).astype(np.uint32)
    # (the inverse of the continuous CDF ln(i + 1) / ln(n + 1): P(i) close to
    # 1 / (i + 1.5), in a second for 50 M draws where a table look-up takes 20)
    s = np.exp(rng.random(n) * np.log(n_subjects + 1.0)).astype(np.int64) - 1
    s = s.clip(0, n_subjects - 1)
    if dist == 'hot_tail':
        s = n_subjects - 1 - s
    return s.astype(np.uint32)


def flush_ms(c, wide):
    c.tune('weigh_wide', wide)
    c.counts_clear()
    c.words_flush()
    # (only the families this flush launched: another one's events are stale)
    part = c.last_kernel_ms('weigh_wide_part') if wide else 0.0
    hist = c.last_kernel_ms('weigh_wide' if wide else 'classify')
    merge = c.last_kernel_ms('weigh_merge')
    return {'part': part, 'hist': hist, 'merge': merge,
            'total': part + hist + merge}


def span(rows, key):
    v = [r[key] for r in rows]
    return {'min': round(min(v), 4), 'max': round(max(v), 4),
            'median': round(float(np.median(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=50_000_000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_weigh.json'))
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    fields, n_reads = read_fields(rng, a.records)
    job = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)]
    results = []
    with nat.Context(0) as c:
        device = c.device_name
        c.counts_reserve(1 << 25)
        c.profile_kernels(True)
        for n_subjects in TABLES:
            for dist in DISTS:
                t0 = time.perf_counter()
                words = fields | subjects(rng, dist, n_subjects, fields.size)
                c.tune('words_keep', 0)
                c.counts_clear()
                c.set_subjects(np.arange(n_subjects, dtype=np.int32))
                # (the forced layout also opens the accumulation unsliced; above
                # 8 slices it is unsliced anyway)
                c.tune('weigh_wide', 1)
                assert c.words_begin(job, 0)
                step = 1 << 23
                for lo in range(0, words.size, step):
                    c.words_append(words[lo:lo + step], 0)
                c.tune('words_keep', 1)
                layouts = [('wide', 1)]
                if n_subjects <= 32 * BINS:
                    layouts.append(('team', 0))
                tables = {}
                for name, wide in layouts:          # warm-up, and the tables
                    flush_ms(c, wide)
                    tables[name] = nat.canonical_counts(*c.counts_fetch())
                same = all(np.array_equal(tables['wide'][0], t[0]) and
                           np.array_equal(tables['wide'][1], t[1])
                           for t in tables.values())
                if not same:
                    sys.exit(f'{n_subjects} {dist}: the layouts differ')
                total = int(tables['wide'][1].astype(object).sum())
                runs = {name: [] for name, _ in layouts}
                for _ in range(a.runs):             # taking turns
                    for name, wide in layouts:
                        runs[name].append(flush_ms(c, wide))
                for name, _ in layouts:
                    row = {'n_subjects': n_subjects, 'dist': dist,
                           'layout': name, 'records': int(words.size),
                           'weight_total': total, 'runs': runs[name]}
                    for key in ('part', 'hist', 'merge', 'total'):
                        row[key + '_ms'] = span(runs[name], key)
                    results.append(row)
                    print(n_subjects, dist, name,
                          {k: row[k + '_ms'] for k in ('part', 'hist', 'merge', 'total')},
                          f'(set-up {time.perf_counter() - t0:.1f} s)', flush=True)
                c.tune('words_keep', 0)
                c.counts_clear()
        c.tune('weigh_wide', 0)
    doc = {'device': device, 'records': int(fields.size), 'reads': n_reads,
           'runs': a.runs, 'unit': 'ms per flush, HIP events around the family',
           'results': results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
