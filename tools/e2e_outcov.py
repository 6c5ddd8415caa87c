#!/usr/bin/env python3
"""`woltka classify ... --outcov` end to end, the host route of the coverage
(`WOLTKA_NO_DCOVER=1`: the host tokenizer's "ex" columns, numpy sort + merge)
against the device route (csrc/wk_cover.hpp), alternating in one process.

Config-4-style SAM text (POS and CIGAR on every line) from the generator of
bench.py / tools/native/libwk_synth.so, in the page cache; two depths:

    deep      500 subjects of 5 Mb, many rows each: the merged set is smaller
              than the rows (whole-genome SAM against a few hundred genomes)
    shallow   1 M subjects of 5 Mb, a few rows each: the merged set is about
              as large as the rows -- the spill path's worst case (and a .cov
              line per record to write).  `--subjects N` sets another number
              (up to the packed record's 2^23; tables beyond 1 299 456 go
              through the wide layout of the weighted histogram)

    python tools/e2e_outcov.py --records 50000000 --reps 5 \
        --json profiles/outcov_e2e.json

Prints per depth and route the median and min-max of the wall time, records/s
and the sha256 over the .cov files (equal between the routes, or the tool
fails).  `--route new --reps 1 --depth deep` is the run to put under
`rocprofv3 --kernel-trace --output-format csv`; `--trace <kernel_trace.csv>
--csv profiles/outcov_kernel_stats.csv` then sums, per kernel of the coverage
pile, its dispatches' times and the bytes each had to move (rows from the grid
size x BYTES_PER_ROW) into GB/s and a share of the HBM peak.  `--tree DIR` runs
the package of another checkout (the parent commit, built there) with `--route
old`, for the one-off check that `WOLTKA_NO_DCOVER=1` is the parent's route."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--tree' in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from woltka_amd.hostio import ROUTES  # noqa: E402
from woltka_amd.workflow import workflow  # noqa: E402

DEPTHS = {'deep': 500, 'shallow': 1_000_000}
HBM_PEAK = 8.0e12       # bytes/s, MI355X

# bytes a kernel moves per row of the pile (12 B = key + end)
# (kernel: bytes per row, rows per workgroup of its grid).  The scan kernels
# work on the digit x chunk matrix: 256 counters of 4 B per 1024 rows = 1 B per
# row, read (sum_tiles) or read + written (scan_apply); a workgroup of theirs
# covers 2048 counters = 8192 rows.  cover_max_scan / tile_scan: one workgroup
# over 8 B per 2048 rows -- launch-bound, no traffic to speak of.
BYTES_PER_ROW = {
    'cover_append_kernel': (12 + 12, 256),   # lsubj / lbeg / lend in, a row out (a thread per line)
    'cover_hist_kernel': (8, 4096),          # the keys (4: the ends, on an `end` pass)
    'cover_sum_tiles_kernel': (1, 8192),
    'cover_scan_apply_kernel': (2, 8192),
    'cover_scatter_kernel': (12 + 12, 4096),
    'cover_max_tiles_kernel': (12, 2048),
    'cover_max_scan_kernel': (0, 0),
    'cover_reach_kernel': (12 + 4, 2048),    # + reach out
    'cover_compact_kernel': (12 + 4, 2048),  # + the merged rows out (<= 12 more)
}


def trace_summary(trace, out_csv):
    """Per coverage kernel: dispatches, total time, rows (upper bound: whole
    workgroups), bytes, GB/s, share of the HBM peak -- from a rocprofv3
    kernel trace in CSV."""
    import csv
    acc = {}
    with open(trace, newline='') as fh:
        for row in csv.DictReader(fh):
            name = row['Kernel_Name']
            key = next((k for k in BYTES_PER_ROW if k in name), None)
            if key is None:
                continue
            grid = int(row.get('Grid_Size') or row.get('Grid_Size_X'))
            wg = int(row.get('Workgroup_Size') or row.get('Workgroup_Size_X'))
            ns = int(row['End_Timestamp']) - int(row['Start_Timestamp'])
            per, rows_wg = BYTES_PER_ROW[key]
            a = acc.setdefault(key, [0, 0, 0])
            a[0] += 1
            a[1] += ns
            a[2] += grid // wg * rows_wg
    lines = ['kernel,dispatches,total_ms,rows,bytes,GB_per_s,share_of_hbm_peak']
    for key in BYTES_PER_ROW:
        if key not in acc:
            continue
        n, ns, rows = acc[key]
        nbytes = rows * BYTES_PER_ROW[key][0]
        rate = nbytes / (ns * 1e-9) if ns else 0.0
        lines.append(f'{key},{n},{ns / 1e6:.3f},{rows},{nbytes},'
                     f'{rate / 1e9:.1f},{rate / HBM_PEAK:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_text(path, n_records, n_subjects, seed):
    rng = np.random.default_rng(seed)
    hits = rng.integers(1, 4, n_records // 2 + 1)
    read_of = np.repeat(np.arange(hits.size, dtype=np.int64), hits)[:n_records]
    subject = rng.integers(0, n_subjects, n_records).astype(np.int32)
    span = 5_000_000
    pos = rng.integers(1, span, n_records).astype(np.int32)
    alen = rng.integers(50, 251, n_records).astype(np.int32)
    flag = np.where(rng.random(n_records) < 0.5, 0, 16).astype(np.int32)
    return bench.write_sam(path, read_of, subject, flag=flag, pos=pos,
                           alen=alen)


def cov_digest(cov):
    h = hashlib.sha256()
    for fn in sorted(os.listdir(cov)):
        h.update(fn.encode() + b'\0')
        with open(os.path.join(cov, fn), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def one_run(sam_dir, tmp, new):
    if new:
        os.environ.pop('WOLTKA_NO_DCOVER', None)
    else:
        os.environ['WOLTKA_NO_DCOVER'] = '1'
    cov = tempfile.mkdtemp(dir=tmp)
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=sam_dir, input_fmt='sam', ranks='none',
                 output_fp=os.path.join(cov, 'profile.tsv'),
                 outcov_dir=os.path.join(cov, 'cov'))
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('dcover')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    return dt, cov_digest(os.path.join(cov, 'cov')), routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=50_000_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--depth', choices=sorted(DEPTHS) + ['both'],
                    default='both')
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--subjects', type=int, default=0,
                    help='subjects of the shallow depth')
    ap.add_argument('--tree', default=None,
                    help='run the package of this checkout instead')
    ap.add_argument('--trace', default=None,
                    help='summarise this rocprofv3 kernel trace (CSV) and stop')
    ap.add_argument('--csv', default=None)
    a = ap.parse_args()
    if a.trace:
        trace_summary(a.trace, a.csv)
        return
    if a.subjects:
        DEPTHS['shallow'] = a.subjects
    out = {'records': a.records, 'reps': a.reps, 'cpus': len(
        os.sched_getaffinity(0)), 'depths': {}}
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        for depth in (sorted(DEPTHS) if a.depth == 'both' else [a.depth]):
            sam_dir = os.path.join(tmp, depth)
            os.makedirs(sam_dir)
            size = write_text(os.path.join(sam_dir, 'S1.sam'), a.records,
                              DEPTHS[depth], 7)
            routes = [True, False] if a.route == 'both' else \
                [a.route == 'new']
            for new in routes:          # warm-up: page cache, first contexts
                one_run(sam_dir, tmp, new)
            times = {r: [] for r in routes}
            digests, seen = {}, {}
            for _ in range(a.reps):
                for new in routes:
                    dt, dg, rt = one_run(sam_dir, tmp, new)
                    times[new].append(dt)
                    digests[new], seen[new] = dg, rt
            res = {'subjects': DEPTHS[depth], 'text_bytes': size}
            for new in routes:
                t = times[new]
                name = 'device' if new else 'host'
                res[name] = {'median_s': statistics.median(t), 'min_s': min(t),
                             'max_s': max(t), 'records_per_s':
                             a.records / statistics.median(t),
                             'cov_sha256': digests[new], 'routes': seen[new]}
                print(f'{depth} ({DEPTHS[depth]} subjects, {a.records} '
                      f'records, {size / 1e9:.2f} GB) {name} route: median '
                      f'{statistics.median(t):.3f} s (min {min(t):.3f}, max '
                      f'{max(t):.3f}) = {a.records / statistics.median(t) / 1e6:.1f}'
                      f' M records/s; cov {digests[new][:16]}; {seen[new]}',
                      flush=True)
            if len(set(digests.values())) > 1:
                raise SystemExit(f'{depth}: the routes wrote different '
                                 f'.cov files: {digests}')
            out['depths'][depth] = res
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
