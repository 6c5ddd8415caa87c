#!/usr/bin/env python3
"""`woltka classify -i reads.sam --coords coords.txt` on one file, end to end:
the host tokenizer's route (`WOLTKA_NO_DDEMUX=1`: every read's sample cut from
its id on the host's threads, CSR arrays over the link -- the route of such a
call before `_run_dhits_demux`) against the device route (R2d: samples looked
up, the block's hits staged with a group per read, matched and counted without
leaving HBM), alternating in one process after a warm-up of each.

Two inputs, both in the page cache:

  A   config 4's text (`woltka_amd/synth.py::ordinal_problem`: paired SAM on
      5 000 genomes x 100 genes, written by the generator of bench.py) as one
      single-sample file: the ids hold no `_`, the one sample is ''.
  B   the multiplexed file of tools/e2e_demux.py (config-3-shaped records, 64
      samples in interleaved runs) with a coordinates table that gives every
      second subject one gene under its hits.

    python tools/e2e_demux_coords.py --reps 3 \
        --json profiles/demux_coords_e2e.json
    python tools/e2e_demux_coords.py --route old --reps 3 \
        --json profiles/demux_coords_e2e_parent.json      # (on the parent commit)

Prints per input and route the median and min-max of the wall time, records/s
and the sha256 over the table (equal between the routes, or the tool fails).
`--route new --reps 1` is the run to put under `rocprofv3 --kernel-trace
--output-format csv`; `--trace <kernel_trace.csv> --csv
profiles/demux_coords_kernel_stats.csv` then sums the dispatches of every
kernel of the traced run (tools/e2e_demux.py's summary)."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench  # noqa: E402
import e2e_demux  # noqa: E402
from woltka_amd import synth  # noqa: E402
from woltka_amd.hostio import ROUTES  # noqa: E402
from woltka_amd.workflow import workflow  # noqa: E402


def write_a(tmp, n_reads):
    """Input A; returns (file, coords, records, bytes)."""
    d = os.path.join(tmp, 'a')
    os.makedirs(d)
    prob = synth.ordinal_problem(np.random.default_rng(1002),
                                 n_pairs=n_reads // 2)
    n_reads = min(n_reads, int(prob['n_reads']))
    sam, coords, n_rec, size = bench.write_ordinal_inputs(d, prob, n_reads)
    return sam, coords, n_rec, size


def write_b(tmp, n_records, n_samples):
    """Input B; returns (file, coords, records, bytes)."""
    d = os.path.join(tmp, 'b')
    os.makedirs(d)
    fp, _, records, _, size = e2e_demux.write_inputs(d, n_records, n_samples, 7)
    coords = os.path.join(d, 'coords.txt')
    with open(coords, 'w') as f:    # (the hits are 150M at POS 1)
        f.writelines(f'>T{v:07d}\n1\t1\t200\n'
                     for v in range(0, e2e_demux.N_SUBJECTS, 2))
    return fp, coords, records, size


def one_run(inp, tmp, new):
    fp, coords = inp[:2]
    if new:
        os.environ.pop('WOLTKA_NO_DDEMUX', None)
    else:
        os.environ['WOLTKA_NO_DDEMUX'] = '1'
    out = os.path.join(tempfile.mkdtemp(dir=tmp), 'out.tsv')
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=fp, input_fmt='sam', coords_fp=coords, overlap=80,
                 output_fmt=False, output_fp=out)
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('dhits_demux')) or \
            (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    with open(out, 'rb') as fh:
        return dt, hashlib.sha256(fh.read()).hexdigest(), routes


def measure(name, inp, tmp, routes, reps):
    records, size = inp[2:]
    for new in routes:          # warm-up: page cache, first contexts
        one_run(inp, tmp, new)
    times = {r: [] for r in routes}
    digests, seen = {}, {}
    for _ in range(reps):
        for new in routes:
            dt, dg, rt = one_run(inp, tmp, new)
            times[new].append(dt)
            digests[new], seen[new] = dg, rt
    out = {'records': records, 'text_bytes': size}
    for new in routes:
        t = times[new]
        label = 'device' if new else 'host'
        out[label] = {'median_s': statistics.median(t), 'min_s': min(t),
                      'max_s': max(t), 'times_s': t,
                      'records_per_s': records / statistics.median(t),
                      'table_sha256': digests[new], 'routes': seen[new]}
        print(f'input {name}, {label} route: median '
              f'{statistics.median(t):.3f} s (min {min(t):.3f}, max '
              f'{max(t):.3f}) = {records / statistics.median(t) / 1e6:.1f} M '
              f'records/s; table {digests[new][:16]}; {seen[new]}', flush=True)
    if len(routes) == 2:
        out['device_over_host'] = out['host']['median_s'] / \
            out['device']['median_s']
    if len(set(digests.values())) > 1:
        raise SystemExit(f'the routes wrote different tables: {digests}')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads-a', type=int, default=270_000_000)
    ap.add_argument('--records-b', type=int, default=50_000_000)
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--inputs', default='ab')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--trace', default=None,
                    help='summarise this rocprofv3 kernel trace (CSV) and stop')
    ap.add_argument('--csv', default=None)
    a = ap.parse_args()
    if a.trace:
        e2e_demux.trace_summary(a.trace, a.csv)
        return
    routes = [True, False] if a.route == 'both' else [a.route == 'new']
    out = {'reps': a.reps, 'cpus': len(os.sched_getaffinity(0)),
           'samples_b': a.samples}
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        for name in a.inputs:
            t0 = time.perf_counter()
            inp = write_a(tmp, a.reads_a) if name == 'a' else \
                write_b(tmp, a.records_b, a.samples)
            print(f'input {name}: {inp[2]} records, {inp[3] / 1e9:.2f} GB of '
                  f'SAM, written in {time.perf_counter() - t0:.0f} s',
                  flush=True)
            out[name] = measure(name, inp, tmp, routes, a.reps)
            for fp in inp[:2]:
                os.remove(fp)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
