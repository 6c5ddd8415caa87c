#!/usr/bin/env python3
"""`woltka classify -i aln/ --rank species --stratify maps/` on one sample, end
to end: plain classification stratified by a read -> genus map, on the device
route (R1s: the map joined on the device, csrc/wk_strata_reads.hpp; every
block staged as a CSR chunk and counted without leaving HBM) against the host
route (`WOLTKA_NO_DSTRATA=1`: the host tokenizer and its hash join on all
threads, CSR chunks through pinned rings -- R3, every such call's route
before), alternating in one process after a warm-up of each.

One sample S1: reads with the ids of config 5's generator (`R` + nine digits,
bench.py::write_sam) and the hits of config 3 (`woltka_amd/synth.py::
lca_problem`, 100 k subjects under 2 M nodes), SAM text in the page cache; the
map `maps/S1.txt` names a genus -- one of 2000, drawn evenly -- for 90 % of the
reads.

    python tools/e2e_strata_plain.py --reads 20000000 --reps 3 \
        --json profiles/strata_plain_e2e.json

Prints per route the median and min-max of the wall time, records/s and the
sha256 over the table (equal between the routes, or the tool fails).
`--package-root DIR` measures the package of another tree (a checkout of the
parent commit, built: there `--route old` is the only route);
`--route new --reps 1` is the run to put under `rocprofv3 --kernel-trace
--output-format csv`; `--trace <kernel_trace.csv> --csv
profiles/strata_plain_kernel_stats.csv` then sums the dispatches of every
kernel of the traced run: count, total and mean time, share of the kernels'
time; the kernels of csrc/wk_strata.hpp and wk_strata_reads.hpp are marked."""
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
N_SUBJECTS = 100_000
N_GENERA = 2000
RANKS = 'species'
COVER = 0.9             # share of the reads the map holds


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
    lines = ['kernel,of_wk_strata,dispatches,total_ms,mean_us,share_of_kernel_time']
    for name, (n, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'{name},{int(name.startswith("strata_"))},{n},'
                     f'{ns / 1e6:.3f},{ns / n / 1e3:.2f},{ns / total:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_map(path, n_reads, rng):
    """`R<read:09d>\\tGenus<genus:05d>\\n` for COVER of the reads, in read
    order."""
    held = np.flatnonzero(rng.random(n_reads) < COVER)
    genus = rng.integers(0, N_GENERA, held.size)
    row = np.frombuffer(b'R000000000\tGenus00000\n', dtype=np.uint8)
    with open(path, 'wb') as f:
        for lo in range(0, held.size, 4_000_000):
            ids, gs = held[lo:lo + 4_000_000], genus[lo:lo + 4_000_000]
            text = np.tile(row, (ids.size, 1))
            for k in range(9):
                text[:, 9 - k] = 48 + ids // 10 ** k % 10
            for k in range(5):
                text[:, 20 - k] = 48 + gs // 10 ** k % 10
            f.write(text.tobytes())
    return int(held.size)


def write_inputs(tmp, n_reads, seed, bench, synth):
    """aln/S1.sam, maps/S1.txt and nodes.dmp; returns (aln, maps, nodes.dmp,
    records, reads in the map, bytes of SAM)."""
    rng = np.random.default_rng(seed)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=N_SUBJECTS, n_reads=n_reads,
        with_names=False))
    aln, maps = os.path.join(tmp, 'aln'), os.path.join(tmp, 'maps')
    os.makedirs(aln)
    os.makedirs(maps)
    records, size = bench.write_sam_lca(os.path.join(aln, 'S1.sam'), p, n_reads)
    held = write_map(os.path.join(maps, 'S1.txt'), n_reads, rng)
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    return aln, maps, nodes, records, held, size


def table_digest(path):
    with open(path, 'rb') as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def one_run(inputs, tmp, new, workflow, ROUTES):
    aln, maps, nodes = inputs[:3]
    if new:
        os.environ.pop('WOLTKA_NO_DSTRATA', None)
    else:
        os.environ['WOLTKA_NO_DSTRATA'] = '1'
    out = os.path.join(tempfile.mkdtemp(dir=tmp), 'table.tsv')
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=aln, input_fmt='sam', nodes_fps=[nodes], ranks=RANKS,
                 strata_dir=maps, output_fmt=False, output_fp=out)
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('dreads_strata')) or \
            (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    return dt, table_digest(out), routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=20_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--package-root', default=ROOT,
                    help='the tree whose package (and bench.py) is measured')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--trace', default=None,
                    help='summarise this rocprofv3 kernel trace (CSV) and stop')
    ap.add_argument('--csv', default=None)
    a = ap.parse_args()
    if a.trace:
        trace_summary(a.trace, a.csv)
        return
    sys.path.insert(0, os.path.abspath(a.package_root))
    import bench
    from woltka_amd import synth
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        t0 = time.perf_counter()
        inputs = write_inputs(tmp, a.reads, 9, bench, synth)
        records, held, size = inputs[3:]
        print(f'{records} records of {a.reads} reads, {held} of them in the '
              f'map, {size / 1e9:.2f} GB of SAM, written in '
              f'{time.perf_counter() - t0:.0f} s', flush=True)
        routes = [True, False] if a.route == 'both' else [a.route == 'new']
        for new in routes:          # warm-up: page cache, first contexts
            one_run(inputs, tmp, new, workflow, ROUTES)
            print('warmed up', flush=True)
        times = {r: [] for r in routes}
        digests, seen = {}, {}
        for _ in range(a.reps):
            for new in routes:
                dt, dg, rt = one_run(inputs, tmp, new, workflow, ROUTES)
                times[new].append(dt)
                digests[new], seen[new] = dg, rt
                print(f'{"device" if new else "host"} {dt:.3f} s', flush=True)
        out = {'reads': a.reads, 'records': records, 'reads_in_map': held,
               'subjects': N_SUBJECTS, 'genera': N_GENERA, 'ranks': RANKS,
               'text_bytes': size, 'reps': a.reps,
               'package_root': os.path.basename(os.path.relpath(
                   os.path.abspath(a.package_root), ROOT)),
               'cpus': len(os.sched_getaffinity(0))}
        for new in routes:
            t = times[new]
            label = 'device' if new else 'host'
            out[label] = {'median_s': statistics.median(t), 'min_s': min(t),
                          'max_s': max(t), 'times_s': t, 'records_per_s':
                          records / statistics.median(t),
                          'table_sha256': digests[new], 'routes': seen[new]}
            print(f'{label} route: median {statistics.median(t):.3f} s (min '
                  f'{min(t):.3f}, max {max(t):.3f}) = '
                  f'{records / statistics.median(t) / 1e6:.1f} M records/s; '
                  f'table {digests[new][:16]}; {seen[new]}', flush=True)
        if len(routes) == 2:
            out['device_over_host'] = out['host']['median_s'] / \
                out['device']['median_s']
        if len(set(digests.values())) > 1:
            raise SystemExit(f'the routes wrote different tables: {digests}')
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
