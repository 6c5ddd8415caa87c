#!/usr/bin/env python3
"""`woltka classify -i reads.sam --rank phylum,genus,species` on one
multiplexed file, end to end: the host tokenizer's route (`WOLTKA_NO_DDEMUX=1`:
every read's sample cut from its id on the host's threads, the route before
csrc/wk_demux.hpp) against the device route (R1d: samples looked up, the block
staged as a CSR chunk and counted without leaving HBM), alternating in one
process after a warm-up of each.

Config-3-shaped SAM text (`woltka_amd/synth.py::lca_problem`, 100 k subjects
under 2 M nodes, written by the generator of bench.py) in the page cache.  The
reads belong to `--samples` samples (64) in interleaved runs of 1 to 400 reads;
an id is `S<sample:02d>_<read of the sample:06d>`.  (The generator writes a
letter and nine digits; the tool then turns the third digit of every line into
the `_` -- the lines are of one width.)

    python tools/e2e_demux.py --records 50000000 --reps 3 \
        --json profiles/demux_e2e.json

Prints per route the median and min-max of the wall time, records/s and the
sha256 over the tables (equal between the routes, or the tool fails).
`--route new --reps 1` is the run to put under `rocprofv3 --kernel-trace
--output-format csv`; `--trace <kernel_trace.csv> --csv
profiles/demux_kernel_stats.csv` then sums the dispatches of every kernel of
the traced run: count, total and mean time, share of the kernels' time; the
kernels of csrc/wk_demux.hpp are marked."""
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
HEADER = 23             # b'@HD\tVN:1.0\tSO:unsorted\n'
LINE = 42               # S + 9 digits, flag 0, T + 7 digits, pos 1, 42, 150M, ...
RANKS = 'phylum,genus,species'


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
    lines = ['kernel,of_wk_demux,dispatches,total_ms,mean_us,share_of_kernel_time']
    for name, (n, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'{name},{int(name.startswith("demux_"))},{n},'
                     f'{ns / 1e6:.3f},{ns / n / 1e3:.2f},{ns / total:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_inputs(tmp, n_records, n_samples, seed):
    """The multiplexed SAM file and nodes.dmp; returns (file, nodes.dmp,
    records, reads, bytes)."""
    rng = np.random.default_rng(seed)
    n_reads = max(1000, n_records // 4)      # (4.75 records per read on average)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=N_SUBJECTS, n_reads=n_reads,
        with_names=False))
    n_reads = int(min(n_reads, np.searchsorted(p['qoff'], n_records)))
    # samples in interleaved runs; a read's number counts within its sample
    runs = rng.integers(1, 401, n_reads // 100 + n_samples + 1)
    owner = rng.integers(0, n_samples, runs.size)
    owner[:n_samples] = np.arange(n_samples)    # (every sample has a run)
    sample = np.repeat(owner, runs)[:n_reads].astype(np.int64)
    if sample.size < n_reads:
        raise SystemExit('the runs do not cover the reads')
    order = np.argsort(sample, kind='stable')
    first = np.searchsorted(sample[order], np.arange(n_samples))
    within = np.empty(n_reads, dtype=np.int64)
    within[order] = np.arange(n_reads) - first[sample[order]]
    if int(within.max()) >= 10 ** 6 or n_samples > 100:
        raise SystemExit('an id holds 2 digits of sample and 6 of read')
    qoff = p['qoff']
    records = int(qoff[n_reads])
    # nine digits: sample, a digit that becomes the `_`, the read
    rid = np.repeat(sample * 10 ** 7 + within, np.diff(qoff[:n_reads + 1]))
    fp = os.path.join(tmp, 'reads.sam')
    size = bench.write_sam(fp, rid, p['subj'][:records], qprefix=b'S')
    if size != HEADER + LINE * records:
        raise SystemExit(f'lines of another width: {size} bytes for {records} records')
    text = np.memmap(fp, dtype=np.uint8, mode='r+', offset=HEADER,
                     shape=(records, LINE))
    if not (text[:, LINE - 1] == 10).all() or not (text[:, 3] == 48).all():
        raise SystemExit('the ids are not where the tool expects them')
    text[:, 3] = ord('_')
    text.flush()
    del text
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    return fp, nodes, records, n_reads, size


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
        os.environ.pop('WOLTKA_NO_DDEMUX', None)
    else:
        os.environ['WOLTKA_NO_DDEMUX'] = '1'
    out = tempfile.mkdtemp(dir=tmp)
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=fp, input_fmt='sam', nodes_fps=[nodes], ranks=RANKS,
                 output_fmt=False, output_fp=os.path.join(out, 'tables'))
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('ddemux')) or (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    return dt, tables_digest(os.path.join(out, 'tables')), routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=50_000_000)
    ap.add_argument('--samples', type=int, default=64)
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
        inputs = write_inputs(tmp, a.records, a.samples, 7)
        records, reads, size = inputs[2:]
        print(f'{records} records of {reads} reads, {a.samples} samples, '
              f'{size / 1e9:.2f} GB of SAM, written in '
              f'{time.perf_counter() - t0:.0f} s', flush=True)
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
               'samples': a.samples, 'subjects': N_SUBJECTS, 'ranks': RANKS,
               'text_bytes': size, 'reps': a.reps,
               'cpus': len(os.sched_getaffinity(0))}
        for new in routes:
            t = times[new]
            label = 'device' if new else 'host'
            out[label] = {'median_s': statistics.median(t), 'min_s': min(t),
                          'max_s': max(t), 'times_s': t, 'records_per_s':
                          records / statistics.median(t),
                          'tables_sha256': digests[new], 'routes': seen[new]}
            print(f'{label} route: median {statistics.median(t):.3f} s (min '
                  f'{min(t):.3f}, max {max(t):.3f}) = '
                  f'{records / statistics.median(t) / 1e6:.1f} M records/s; '
                  f'tables {digests[new][:16]}; {seen[new]}', flush=True)
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
