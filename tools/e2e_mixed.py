#!/usr/bin/env python3
"""`woltka classify -i reads.sam --rank none,free,phylum,class,order,family,
genus,species` (the call of the reference's doc/wolsop.sh) on a directory of
one file, end to end: the route of before (`WOLTKA_NO_MIXED=1`: a set of whole-read jobs next to
plain ones goes through the host tokenizer and the general evaluator, R3)
against the packed-record route (R1: text tokenised on the device, the
sample's records kept once and counted by both evaluators at the flush,
wk_words_begin_mixed), alternating in one process after a warm-up of each.

Config-3-shaped SAM text (`woltka_amd/synth.py::lca_problem`, 100 k subjects
under 2 M nodes, written by the generator of bench.py) in the page cache.

    python tools/e2e_mixed.py --records 50000000 --reps 3 \
        --json profiles/mixed_e2e.json

Prints per route the median and min-max of the wall time, records/s and the
sha256 over the tables (equal between the routes, or the tool fails).
`--route old` needs nothing of the new route but the environment variable, so
the same file run in a checkout of the commit before gives the baseline
(`--json` then holds that one route).  `--route new --reps 1` is the run to
put under `rocprofv3 --kernel-trace --output-format csv`; `--trace
<kernel_trace.csv> --csv profiles/mixed_kernel_stats.csv` then sums the
dispatches of every kernel of the traced run: count, total and mean time,
share of the kernels' time; the kernels of the flush are marked."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from woltka_amd import synth  # noqa: E402
from woltka_amd.hostio import ROUTES  # noqa: E402
from woltka_amd.workflow import workflow  # noqa: E402

N_SUBJECTS = 100_000
RANKS = 'none,free,phylum,class,order,family,genus,species'
# what wk_words_flush launches for a mixed set (csrc/wk_free.hpp, wk_weigh.hpp,
# wk_weigh_wide.hpp)
FLUSH = ('free_stream_kernel', 'free_log_kernel', 'free_counts_kernel',
         'weigh_bins_kernel', 'weigh_merge_kernel', 'weigh_wide_kernel',
         'wide_count_kernel', 'wide_scan_kernel', 'wide_scatter_kernel')


def trace_summary(trace, out_csv):
    import csv
    acc = {}
    with open(trace, newline='') as fh:
        for row in csv.DictReader(fh):
            # (`void wk::name<..>(..)`, `(anonymous namespace)::name(..)`)
            m = re.search(r'(\w+)\s*(?:<[^(]*)?(?:\(|$)', row['Kernel_Name'].replace(
                '(anonymous namespace)::', ''))
            name = m.group(1) if m else row['Kernel_Name']
            ns = int(row['End_Timestamp']) - int(row['Start_Timestamp'])
            a = acc.setdefault(name, [0, 0])
            a[0] += 1
            a[1] += ns
    total = sum(ns for _, ns in acc.values()) or 1
    lines = ['kernel,of_the_flush,dispatches,total_ms,mean_us,share_of_kernel_time']
    for name, (n, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'{name},{int(name in FLUSH)},{n},'
                     f'{ns / 1e6:.3f},{ns / n / 1e3:.2f},{ns / total:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_inputs(tmp, n_records, seed):
    """A directory with the one SAM file (a sample per file: a single-file
    input would be demultiplexed) and nodes.dmp; returns (directory,
    nodes.dmp, records, reads, bytes)."""
    rng = np.random.default_rng(seed)
    n_reads = max(1000, n_records // 4)      # (4.75 records per read on average)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=N_SUBJECTS, n_reads=n_reads,
        with_names=False))
    n_reads = int(min(n_reads, np.searchsorted(p['qoff'], n_records)))
    indir = os.path.join(tmp, 'aln')
    os.mkdir(indir)
    records, size = bench.write_sam_lca(os.path.join(indir, 'S1.sam'), p,
                                        n_reads)
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    return indir, nodes, int(records), n_reads, int(size)


def tables_digest(out):
    h = hashlib.sha256()
    for fn in sorted(os.listdir(out)):
        h.update(fn.encode() + b'\0')
        with open(os.path.join(out, fn), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def one_run(inputs, tmp, new):
    fp, nodes = inputs[:2]
    if new:
        os.environ.pop('WOLTKA_NO_MIXED', None)
    else:
        os.environ['WOLTKA_NO_MIXED'] = '1'
    out = tempfile.mkdtemp(dir=tmp)
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=fp, input_fmt='sam', nodes_fps=[nodes], ranks=RANKS,
                 output_fmt=False, output_fp=os.path.join(out, 'tables'))
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('mixed')) or new != bool(routes.get('dtok')) or \
            (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    return dt, tables_digest(os.path.join(out, 'tables')), routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=50_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--trace', default=None,
                    help='summarise this rocprofv3 kernel trace (CSV) and stop')
    ap.add_argument('--csv', default=None)
    a = ap.parse_args()
    if a.trace:
        trace_summary(a.trace, a.csv)
        return
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        t0 = time.perf_counter()
        inputs = write_inputs(tmp, a.records, 7)
        records, reads, size = inputs[2:]
        print(f'{records} records of {reads} reads, {size / 1e9:.2f} GB of SAM, '
              f'written in {time.perf_counter() - t0:.0f} s', flush=True)
        routes = [True, False] if a.route == 'both' else [a.route == 'new']
        for new in routes:          # warm-up: page cache, first contexts
            one_run(inputs, tmp, new)
        times = {r: [] for r in routes}
        digests, seen = {}, {}
        for _ in range(a.reps):
            for new in routes:
                dt, dg, rt = one_run(inputs, tmp, new)
                times[new].append(dt)
                digests[new], seen[new] = dg, rt
        out = {'records_asked': a.records, 'records': records, 'reads': reads,
               'subjects': N_SUBJECTS, 'ranks': RANKS, 'text_bytes': size,
               'reps': a.reps, 'cpus': len(os.sched_getaffinity(0))}
        for new in routes:
            t = times[new]
            label = 'mixed' if new else 'general'
            out[label] = {'median_s': statistics.median(t), 'min_s': min(t),
                          'max_s': max(t), 'times_s': t, 'records_per_s':
                          records / statistics.median(t),
                          'tables_sha256': digests[new], 'routes': seen[new]}
            print(f'{label} route: median {statistics.median(t):.3f} s (min '
                  f'{min(t):.3f}, max {max(t):.3f}) = '
                  f'{records / statistics.median(t) / 1e6:.1f} M records/s; '
                  f'tables {digests[new][:16]}; {seen[new]}', flush=True)
        if len(routes) == 2:
            out['mixed_over_general'] = out['general']['median_s'] / \
                out['mixed']['median_s']
        if len(set(digests.values())) > 1:
            raise SystemExit(f'the routes wrote different tables: {digests}')
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
