#!/usr/bin/env python3
"""`woltka classify -i aln/ --uniq --outmap maps/` and `... --rank genus --uniq
--outmap maps/` on one sample, end to end, with `--zipmap gz` and `none`: the
read maps of whole-read assignments on the device route (R1m: every block
staged as a CSR chunk, counted with the assignment codes left in HBM, the map
lines formatted there, csrc/wk_readmap_reads.hpp; only finished text crosses
to the host) against the host route (`WOLTKA_NO_DREADMAPS=1`: the host
tokenizer on all threads, the codes copied back, numpy and `wk_format_readmap`
on helper threads -- R3, every such call's route before), alternating in one
process after a warm-up of each.

One sample S1: the reads and hits of config 3 (`woltka_amd/synth.py::
lca_problem`, 100 k subjects under 2 M nodes) as SAM text in the page cache.
The first command has no hierarchy (the OGU recipe: the features are the
subjects, `--uniq` keeps the reads of one), the second one `nodes.dmp`.

    python tools/e2e_readmap_reads.py --reads 20000000 --reps 3 \\
        --json profiles/readmap_reads_e2e.json

Prints per command, compression and route the median and min-max of the wall
time, records/s and the sha256 over the table and over the (inflated) map
text -- equal between the routes, or the tool fails.  `--package-root DIR`
measures the package of another tree (a checkout of the parent commit, built:
there `--route old` is the only route); `--expect FILE.json` then requires
the digests of that earlier result.  `--route new --reps 1 --only genus-none`
is the run to put under `rocprofv3 --kernel-trace --output-format csv`;
`--trace <kernel_trace.csv> --csv profiles/readmap_reads_kernel_stats.csv`
then sums the dispatches of every kernel of the traced run: count, total and
mean time, share of the kernels' time; the kernels of
csrc/wk_readmap_reads.hpp and the scan they share with wk_readmap.hpp are
marked."""
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
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SUBJECTS = 100_000
COMMANDS = {'none': dict(uniq=True), 'genus': dict(ranks='genus', uniq=True)}
ZIPS = ('gz', 'none')
MARKED = ('readmap_leaders_kernel', 'readmap_reads_len_kernel',
          'readmap_reads_write_kernel', 'u64_tile_sum_kernel',
          'u64_tile_prefix_kernel', 'tile_scan_kernel',
          'strata_place_reads_kernel')


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
    lines = ['kernel,of_readmap_reads,dispatches,total_ms,mean_us,share_of_kernel_time']
    for name, (n, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'{name},{int(name in MARKED)},{n},'
                     f'{ns / 1e6:.3f},{ns / n / 1e3:.2f},{ns / total:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_inputs(tmp, n_reads, seed, bench, synth):
    """aln/S1.sam and nodes.dmp; returns (aln, nodes.dmp, records, bytes of
    SAM)."""
    rng = np.random.default_rng(seed)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=N_SUBJECTS, n_reads=n_reads,
        with_names=False))
    aln = os.path.join(tmp, 'aln')
    os.makedirs(aln)
    records, size = bench.write_sam_lca(os.path.join(aln, 'S1.sam'), p, n_reads)
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    return aln, nodes, records, size


def file_digest(path, gz=False):
    """sha256 of the file's bytes -- of the text a chain of gzip members
    inflates to, for a compressed map -- and the number of bytes hashed."""
    h, n = hashlib.sha256(), 0
    with open(path, 'rb') as fh:
        d = zlib.decompressobj(31) if gz else None
        while True:
            piece = fh.read(1 << 24)
            if not piece:
                break
            while gz and piece:
                text = d.decompress(piece)
                h.update(text)
                n += len(text)
                piece = d.unused_data
                if d.eof:
                    d = zlib.decompressobj(31)
                else:
                    break
            if not gz:
                h.update(piece)
                n += len(piece)
    return h.hexdigest(), n


def one_run(inputs, tmp, command, outzip, new, workflow, ROUTES, digests=True):
    aln, nodes = inputs[:2]
    if new:
        os.environ.pop('WOLTKA_NO_DREADMAPS', None)
    else:
        os.environ['WOLTKA_NO_DREADMAPS'] = '1'
    work = tempfile.mkdtemp(dir=tmp)
    out, maps = os.path.join(work, 'table.tsv'), os.path.join(work, 'maps')
    kw = dict(COMMANDS[command])
    if command != 'none':
        kw['nodes_fps'] = [nodes]
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=aln, input_fmt='sam', output_fmt=False,
                 output_fp=out, outmap_dir=maps, outmap_zip=outzip, **kw)
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('dreads_maps')) or \
            (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    dg = None
    if digests:
        fn = 'S1.txt.gz' if outzip == 'gz' else 'S1.txt'
        m, n = file_digest(os.path.join(maps, fn), outzip == 'gz')
        dg = {'table_sha256': file_digest(out)[0], 'map_sha256': m,
              'map_bytes': n}
    import shutil
    shutil.rmtree(work)
    return dt, dg, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=20_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--only', default=None,
                    help='one configuration: <command>-<zip>, e.g. genus-none')
    ap.add_argument('--package-root', default=ROOT,
                    help='the tree whose package (and bench.py) is measured')
    ap.add_argument('--expect', default=None,
                    help='an earlier result whose digests must come out again')
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
    expect = None
    if a.expect:
        with open(a.expect) as fh:
            expect = json.load(fh)['configs']
    configs = [(c, z) for c in COMMANDS for z in ZIPS
               if a.only in (None, f'{c}-{z}')]
    routes = [True, False] if a.route == 'both' else [a.route == 'new']
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        t0 = time.perf_counter()
        inputs = write_inputs(tmp, a.reads, 9, bench, synth)
        records, size = inputs[2:]
        print(f'{records} records of {a.reads} reads, {size / 1e9:.2f} GB of '
              f'SAM, written in {time.perf_counter() - t0:.0f} s', flush=True)
        out = {'reads': a.reads, 'records': records, 'subjects': N_SUBJECTS,
               'text_bytes': size, 'reps': a.reps,
               'package_root': os.path.basename(os.path.relpath(
                   os.path.abspath(a.package_root), ROOT)),
               'cpus': len(os.sched_getaffinity(0)), 'configs': {}}
        for command, outzip in configs:
            key = f'{command}-{outzip}'
            for new in routes:      # warm-up: page cache, first contexts
                one_run(inputs, tmp, command, outzip, new, workflow, ROUTES,
                        digests=False)
            print(f'{key}: warmed up', flush=True)
            times = {r: [] for r in routes}
            digests, seen = {}, {}
            for rep in range(a.reps):
                for new in routes:
                    dt, dg, rt = one_run(inputs, tmp, command, outzip, new,
                                         workflow, ROUTES,
                                         digests=rep == a.reps - 1)
                    times[new].append(dt)
                    seen[new] = rt
                    if dg:
                        digests[new] = dg
                    print(f'{key} {"device" if new else "host"} {dt:.3f} s',
                          flush=True)
            res = out['configs'][key] = {}
            for new in routes:
                t = times[new]
                label = 'device' if new else 'host'
                res[label] = dict(digests[new], median_s=statistics.median(t),
                                  min_s=min(t), max_s=max(t), times_s=t,
                                  records_per_s=records / statistics.median(t),
                                  routes=seen[new])
                print(f'{key} {label} route: median {statistics.median(t):.3f}'
                      f' s (min {min(t):.3f}, max {max(t):.3f}) = '
                      f'{records / statistics.median(t) / 1e6:.1f} M records/s;'
                      f' table {digests[new]["table_sha256"][:16]}, map '
                      f'{digests[new]["map_sha256"][:16]} '
                      f'({digests[new]["map_bytes"]} bytes); {seen[new]}',
                      flush=True)
            if len(routes) == 2:
                res['device_over_host'] = res['host']['median_s'] / \
                    res['device']['median_s']
            said = {(d['table_sha256'], d['map_sha256'])
                    for d in digests.values()}
            if expect is not None:
                said |= {(d['table_sha256'], d['map_sha256'])
                         for k, d in expect[key].items() if isinstance(d, dict)}
            if len(said) > 1:
                raise SystemExit(f'{key}: different tables or maps: {said}')
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
