#!/usr/bin/env python3
"""`woltka classify ... --rank phylum,genus,species --sizes length.map --scale
1M --digits 3` end to end: the general route (`WOLTKA_NO_DSIZES=1`: host
tokenizer, generic evaluator, contribution log folded on the host) against the
words route with the sized flush (csrc/wk_sized.hpp), alternating in one
process after a warm-up of each.

Config-3-shaped SAM text (`woltka_amd/synth.py::lca_problem`, written by the
generator of bench.py) in the page cache, with a generated size map; two
inputs:

    config3   100 k subjects under 2 M nodes
    wide      1 M subjects: the unsliced layout, a sub-slice per workgroup

    python tools/e2e_sizes.py --records 50000000 --reps 3 \
        --json profiles/sizes_e2e.json

Prints per input and route the median and min-max of the wall time, records/s
and the sha256 over the tables (equal between the routes, or the tool fails).
`--route new --reps 1 --input config3` is the run to put under `rocprofv3
--kernel-trace --output-format csv`; `--trace <kernel_trace.csv> --records N
--csv profiles/sizes_kernel_stats.csv` then sums the dispatches of the new
kernels: time, and for `sized_bins_kernel` GB/s over 4 B per record times the
number of workgroups that read a record (the sub-slices of its stream: the
grid size / teams is not in a trace, so the tool takes `--reads-per-record`
-- 16 for streams whose slices are full, the sub-slices of the whole table
for the unsliced layout -- and `--runs`, the classify calls in the trace).

`--jobs free | genus-uniq | mixed` runs a job set that looks at whole reads
instead: every chunk then goes through the general evaluator's contribution
log, and the routes alternated are the log reduced on the device
(csrc/wk_logred.hpp) against `WOLTKA_NO_DLOG=1`, the log downloaded and folded
on the host:

    python tools/e2e_sizes.py --jobs free --records 20000000 --reps 3 \
        --json profiles/logred_e2e.json

With `--trace`, `--log-rows N` (the rows the logs of the traced run held, the
sum of `log_rows` the run printed) gives `log_reduce_kernel` its GB/s over the
16 B per row the algorithm has to read."""
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
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from woltka_amd import synth  # noqa: E402
from woltka_amd.hostio import ROUTES  # noqa: E402
from woltka_amd.workflow import workflow  # noqa: E402

INPUTS = {'config3': 100_000, 'wide': 1_000_000}
HBM_PEAK = 8.0e12       # bytes/s, MI355X
KERNELS = ('sized_bins_kernel', 'sized_rows_kernel', 'log_reduce_kernel',
           'log_emit_kernel')
# --jobs: keyword arguments of workflow for job sets that look at whole reads
JOBS = {'free': dict(ranks='free'),
        'genus-uniq': dict(ranks='genus', uniq=True),
        'mixed': dict(ranks='free,genus,none')}


def trace_summary(trace, out_csv, records, reads_per_record, runs, log_rows=0):
    import csv
    acc = {}
    with open(trace, newline='') as fh:
        for row in csv.DictReader(fh):
            key = next((k for k in KERNELS if k in row['Kernel_Name']), None)
            if key is None:
                continue
            if key == 'sized_rows_kernel':
                key += '<emit>' if 'ILb1' in row['Kernel_Name'] or \
                    '<true>' in row['Kernel_Name'] else '<count>'
            ns = int(row['End_Timestamp']) - int(row['Start_Timestamp'])
            a = acc.setdefault(key, [0, 0])
            a[0] += 1
            a[1] += ns
    lines = ['kernel,dispatches,total_ms,bytes,GB_per_s,share_of_hbm_peak']
    for key, (n, ns) in sorted(acc.items()):
        nbytes = 4 * records * reads_per_record * runs \
            if key == 'sized_bins_kernel' else \
            16 * log_rows if key == 'log_reduce_kernel' else 0
        rate = nbytes / (ns * 1e-9) if ns else 0.0
        lines.append(f'{key},{n},{ns / 1e6:.3f},{nbytes},{rate / 1e9:.1f},'
                     f'{rate / HBM_PEAK:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_inputs(tmp, n_records, n_subjects, seed):
    """SAM, nodes.dmp and size map; returns (directory of the SAM, nodes.dmp,
    size map, records, bytes)."""
    rng = np.random.default_rng(seed)
    n_reads = max(1000, n_records // 5)      # (4.75 records per read on average)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=n_subjects, n_reads=n_reads,
        with_names=False))
    # (as many reads as give the records asked for)
    n_reads = int(min(n_reads, np.searchsorted(p['qoff'], n_records)))
    sam_dir = os.path.join(tmp, 'aln')
    os.makedirs(sam_dir)
    records, size = bench.write_sam_lca(os.path.join(sam_dir, 'S1.sam'), p,
                                        n_reads)
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    sizes = os.path.join(tmp, 'length.map')
    subjects = np.unique(p['subj'])
    lengths = rng.integers(500_000, 12_000_000, subjects.size)
    with open(sizes, 'w') as f:
        f.writelines(f'T{s:07d}\t{n}\n' for s, n in zip(subjects.tolist(),
                                                        lengths.tolist()))
    return sam_dir, nodes, sizes, records, size


def tables_digest(out):
    h = hashlib.sha256()
    for fn in sorted(os.listdir(out)):
        h.update(fn.encode() + b'\0')
        with open(os.path.join(out, fn), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def one_run(inputs, tmp, new, jobs=None):
    sam_dir, nodes, sizes = inputs[:3]
    switch, route = ('WOLTKA_NO_DLOG', 'log_reduce') if jobs else \
        ('WOLTKA_NO_DSIZES', 'sized_flush')
    if new:
        os.environ.pop(switch, None)
    else:
        os.environ[switch] = '1'
    kw = dict(JOBS[jobs]) if jobs else dict(ranks='phylum,genus,species')
    out = tempfile.mkdtemp(dir=tmp)
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=sam_dir, input_fmt='sam', nodes_fps=[nodes],
                 sizes=sizes, scale='1M', digits=3, output_fmt=False,
                 output_fp=os.path.join(out, 'tables'), **kw)
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get(route)) or (jobs and routes.get('sized_flush')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    tables = os.path.join(out, 'tables')
    if os.path.isfile(tables):      # (one rank: one file)
        with open(tables, 'rb') as fh:
            return dt, hashlib.sha256(fh.read()).hexdigest(), routes
    return dt, tables_digest(tables), routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=50_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--input', choices=sorted(INPUTS) + ['both'],
                    default='both')
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--jobs', choices=sorted(JOBS), default=None,
                    help='a job set of the general route: alternate the '
                    'device-side reduction of its log with WOLTKA_NO_DLOG=1')
    ap.add_argument('--log-rows', type=int, default=0)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--trace', default=None,
                    help='summarise this rocprofv3 kernel trace (CSV) and stop')
    ap.add_argument('--csv', default=None)
    ap.add_argument('--reads-per-record', type=int, default=16)
    ap.add_argument('--runs', type=int, default=2,
                    help='classify calls in the trace (warm-up + repetitions)')
    a = ap.parse_args()
    if a.trace:
        trace_summary(a.trace, a.csv, a.records, a.reads_per_record, a.runs,
                      a.log_rows)
        return
    out = {'records_asked': a.records, 'reps': a.reps, 'jobs': a.jobs, 'cpus': len(
        os.sched_getaffinity(0)), 'inputs': {}}
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        for name in (sorted(INPUTS) if a.input == 'both' else [a.input]):
            work = os.path.join(tmp, name)
            os.makedirs(work)
            t0 = time.perf_counter()
            inputs = write_inputs(work, a.records, INPUTS[name], 7)
            records, size = inputs[3:]
            print(f'{name}: {records} records, {size / 1e9:.2f} GB of SAM, '
                  f'written in {time.perf_counter() - t0:.0f} s', flush=True)
            routes = [True, False] if a.route == 'both' else \
                [a.route == 'new']
            for new in routes:          # warm-up: page cache, first contexts
                one_run(inputs, work, new, a.jobs)
            times = {r: [] for r in routes}
            digests, seen = {}, {}
            for _ in range(a.reps):
                for new in routes:
                    dt, dg, rt = one_run(inputs, work, new, a.jobs)
                    times[new].append(dt)
                    digests[new], seen[new] = dg, rt
            res = {'subjects': INPUTS[name], 'records': records,
                   'text_bytes': size}
            for new in routes:
                t = times[new]
                label = 'device' if new else 'host'
                res[label] = {'median_s': statistics.median(t), 'min_s': min(t),
                              'max_s': max(t), 'records_per_s':
                              records / statistics.median(t),
                              'tables_sha256': digests[new],
                              'routes': seen[new]}
                print(f'{name} ({INPUTS[name]} subjects, {records} records) '
                      f'{label} route: median {statistics.median(t):.3f} s '
                      f'(min {min(t):.3f}, max {max(t):.3f}) = '
                      f'{records / statistics.median(t) / 1e6:.1f} M records/s; '
                      f'tables {digests[new][:16]}; {seen[new]}', flush=True)
            if len(set(digests.values())) > 1:
                raise SystemExit(f'{name}: the routes wrote different tables: '
                                 f'{digests}')
            out['inputs'][name] = res
            if a.json:      # (after every input: a long run leaves what it has)
                os.makedirs(os.path.dirname(os.path.abspath(a.json)),
                            exist_ok=True)
                with open(a.json, 'w') as fh:
                    json.dump(out, fh, indent=1, sort_keys=True)
                    fh.write('\n')


if __name__ == '__main__':
    main()
