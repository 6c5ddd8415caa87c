#!/usr/bin/env python3
"""`woltka classify -i sample.sam --rank genus --uniq --outmap maps/` and
`... --rank none,free,genus --outmap maps/` on ONE file, end to end, with
`--zipmap none`: a single-file input is demultiplexed, so these are read maps
under demultiplexing -- on the device route (R1dm: every block staged as a CSR
chunk with a group and a sample id per read, counted with the assignment codes
left in HBM, the map lines formatted there and cut into one run per sample,
csrc/wk_readmap_demux.hpp) against the host route (`WOLTKA_NO_DDEMUXMAPS=1`:
the host tokenizer on all threads, the read ids as Python strings,
`demux_labels` and the Python writer -- R3, every such call's route before),
alternating in one process after a warm-up of each.

The reads and hits are those of tools/e2e_readmap_reads.py (config 3 of
`woltka_amd/synth.py::lca_problem`, 100 k subjects under 2 M nodes), written
twice: `mux64` -- the QNAMEs `S<read % 64>_R<read>`, 64 samples interleaved
read by read -- and `single` -- every QNAME `S1_R<read>`, one sample.

    python tools/e2e_readmap_demux.py --reads 12000000 --reps 3 \\
        --json profiles/readmap_demux_e2e.json

Prints per input, command and route the median and min-max of the wall time,
records/s and one sha256 over the tables and one over all map files (by name,
in order) -- equal between the routes, or the tool fails.  `--package-root
DIR` measures the package of another tree (a checkout of the parent commit,
built: there `--route old` is the only route); `--expect FILE.json` then
requires the digests of that earlier result.  `--route new --reps 1 --only
mux64-mixed` is the run to put under `rocprofv3 --kernel-trace
--output-format csv`; `--trace <kernel_trace.csv> --csv
profiles/readmap_demux_kernel_stats.csv` then sums the dispatches of every
kernel of the traced run; the kernels of csrc/wk_readmap_demux.hpp are
marked.

`--cross` adds a check that needs no run of the host route (one of which takes
minutes under a list job): the same records are written once more WITHOUT the
sample in front of the QNAMEs, as a directory of one file per sample
(`S1.sam`; `S00.sam` .. `S63.sam`), and classified there without
demultiplexing -- the routes of read maps that are not demultiplexed (R1m /
R1l, csrc/wk_readmap_reads.hpp, wk_readmap_lists.hpp: the formatters whose
text the host route was held to at this size, profiles/readmap_lists_e2e.json).
A sample's map file must then have the same name and bytes either way, and the
tables must be equal; the tool fails if the digests differ.  `--only` takes
several configurations, separated by commas."""
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
COMMANDS = {'genus': dict(ranks='genus', uniq=True),
            'mixed': dict(ranks='none,free,genus')}
INPUTS = ('mux64', 'single')
MARKED = ('readmap_reads_len_demux_kernel', 'readmap_reads_write_demux_kernel',
          'readmap_lists_build_demux_kernel',
          'readmap_lists_write_demux_kernel', 'readmap_demux_mark_kernel',
          'readmap_demux_rank_kernel', 'readmap_demux_tile_kernel',
          'readmap_demux_columns_kernel', 'readmap_demux_across_kernel',
          'readmap_demux_add_kernel')


def trace_summary(trace, out_csv):
    import csv
    acc = {}
    with open(trace, newline='') as fh:
        for row in csv.DictReader(fh):
            m = re.search(r'(\w+)\s*(?:<[^(]*)?(?:\(|$)', row['Kernel_Name'].replace(
                '(anonymous namespace)::', ''))
            name = m.group(1) if m else row['Kernel_Name']
            ns = int(row['End_Timestamp']) - int(row['Start_Timestamp'])
            a = acc.setdefault(name, [0, 0])
            a[0] += 1
            a[1] += ns
    total = sum(ns for _, ns in acc.values()) or 1
    lines = ['kernel,of_readmap_demux,dispatches,total_ms,mean_us,share_of_kernel_time']
    for name, (n, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'{name},{int(name in MARKED)},{n},'
                     f'{ns / 1e6:.3f},{ns / n / 1e3:.2f},{ns / total:.4f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def write_inputs(tmp, n_reads, seed, bench, synth, cross=False):
    """mux64.sam, single.sam and nodes.dmp; returns ({input: path}, nodes.dmp,
    records, bytes of one SAM file).  ``cross``: also `dir_single/S1.sam` and
    `dir_mux64/S<nn>.sam`, the same records per sample with the QNAMEs
    `R<read>` (paths 'dir_single', 'dir_mux64')."""
    rng = np.random.default_rng(seed)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=N_SUBJECTS, n_reads=n_reads,
        with_names=False))
    qoff = p['qoff']
    records = int(qoff[n_reads])
    read_of = np.repeat(np.arange(n_reads, dtype=np.int64),
                        np.diff(qoff[:n_reads + 1]))
    paths = {k: os.path.join(tmp, f'{k}.sam') for k in INPUTS}
    plain = os.path.join(tmp, 'plain.sam')      # QNAMEs `R<read>`
    bench.write_sam(plain, read_of, p['subj'][:records])
    # (lines of one width behind the header: the sample goes in front)
    text = np.memmap(plain, dtype=np.uint8, mode='r')
    head = int(np.flatnonzero(text[:256] == 10)[0]) + 1
    width = int(np.flatnonzero(text[head:head + 512] == 10)[0]) + 1
    if (text.size - head) != records * width:
        raise SystemExit('the SAM lines are not of one width')
    size = 0
    for which, k in (('single', 3), ('mux64', 4)):
        with open(paths[which], 'wb') as fh:
            fh.write(text[:head].tobytes())
            for lo in range(0, records, 1 << 22):
                hi = min(records, lo + (1 << 22))
                lines = np.empty((hi - lo, width + k), dtype=np.uint8)
                lines[:, k:] = text[head + lo * width:
                                    head + hi * width].reshape(-1, width)
                lines[:, 0] = ord('S')
                lines[:, k - 1] = ord('_')
                if which == 'single':
                    lines[:, 1] = ord('1')
                else:
                    s = read_of[lo:hi] % 64
                    lines[:, 1] = 48 + s // 10
                    lines[:, 2] = 48 + s % 10
                fh.write(lines.tobytes())
        size = max(size, os.path.getsize(paths[which]))
    if cross:
        for d in ('dir_single', 'dir_mux64'):
            paths[d] = os.path.join(tmp, d)
            os.makedirs(paths[d])
        fhs = [open(os.path.join(paths['dir_mux64'], f'S{k:02d}.sam'), 'wb')
               for k in range(64)]
        for fh in fhs:
            fh.write(text[:head].tobytes())
        for lo in range(0, records, 1 << 22):
            hi = min(records, lo + (1 << 22))
            s = read_of[lo:hi] % 64
            order = np.argsort(s, kind='stable')
            lines = text[head + lo * width:
                         head + hi * width].reshape(-1, width)[order]
            cuts = np.searchsorted(s[order], np.arange(65))
            for k, fh in enumerate(fhs):
                fh.write(lines[cuts[k]:cuts[k + 1]].tobytes())
        for fh in fhs:
            fh.close()
    del text
    if cross:
        os.rename(plain, os.path.join(paths['dir_single'], 'S1.sam'))
    else:
        os.remove(plain)
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    return paths, nodes, records, size


def tree_digest(top):
    """(sha256 over the names and bytes of every file under ``top`` in
    order, files, bytes)."""
    h, n, k = hashlib.sha256(), 0, 0
    paths = [top] if os.path.isfile(top) else sorted(
        os.path.join(d, f) for d, _, fs in os.walk(top) for f in fs)
    for path in paths:
        h.update(os.path.relpath(path, top).encode() + b'\0')
        with open(path, 'rb') as fh:
            while True:
                piece = fh.read(1 << 24)
                if not piece:
                    break
                h.update(piece)
                n += len(piece)
        k += 1
    return h.hexdigest(), k, n


def one_run(inputs, tmp, which, command, new, workflow, ROUTES, digests=True):
    paths, nodes = inputs[:2]
    if new:
        os.environ.pop('WOLTKA_NO_DDEMUXMAPS', None)
    else:
        os.environ['WOLTKA_NO_DDEMUXMAPS'] = '1'
    work = tempfile.mkdtemp(dir=tmp)
    out, maps = os.path.join(work, 'out'), os.path.join(work, 'maps')
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=paths[which], input_fmt='sam', output_fmt=False,
                 output_fp=out, outmap_dir=maps, outmap_zip='none',
                 nodes_fps=[nodes], **COMMANDS[command])
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('dreads_demux')) or \
            (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    dg = None
    if digests:
        m, k, n = tree_digest(maps)
        dg = {'table_sha256': tree_digest(out)[0], 'map_sha256': m,
              'map_files': k, 'map_bytes': n}
    import shutil
    shutil.rmtree(work)
    return dt, dg, routes


def cross_run(inputs, tmp, which, command, workflow, ROUTES):
    """The records of input ``which`` as a directory of one file per sample,
    not demultiplexed: (seconds, digests, routes)."""
    paths, nodes = inputs[:2]
    work = tempfile.mkdtemp(dir=tmp)
    out, maps = os.path.join(work, 'out'), os.path.join(work, 'maps')
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=paths[f'dir_{which}'], input_fmt='sam',
                 output_fmt=False, output_fp=out, outmap_dir=maps,
                 outmap_zip='none', nodes_fps=[nodes], **COMMANDS[command])
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if routes.get('dreads_demux') or routes.get('host_block') or not (
            routes.get('dreads_lists') or routes.get('dreads_maps')):
        raise SystemExit(f'the cross-check took another route: {routes}')
    m, k, n = tree_digest(maps)
    dg = {'table_sha256': tree_digest(out)[0], 'map_sha256': m,
          'map_files': k, 'map_bytes': n}
    import shutil
    shutil.rmtree(work)
    return dt, dg, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=12_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--only', default=None,
                    help='configurations: <input>-<command>[,...], e.g. mux64-mixed')
    ap.add_argument('--cross', action='store_true',
                    help='check the device route against the same records, '
                    'one file per sample, not demultiplexed')
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
    only = a.only.split(',') if a.only else None
    configs = [(i, c) for c in COMMANDS for i in INPUTS
               if only is None or f'{i}-{c}' in only]
    if a.cross and a.route == 'old':
        raise SystemExit('--cross checks the device route')
    routes = [True, False] if a.route == 'both' else [a.route == 'new']
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        t0 = time.perf_counter()
        inputs = write_inputs(tmp, a.reads, 9, bench, synth, cross=a.cross)
        records, size = inputs[2:]
        print(f'{records} records of {a.reads} reads, 2 x {size / 1e9:.2f} GB '
              f'of SAM, written in {time.perf_counter() - t0:.0f} s',
              flush=True)
        out = {'reads': a.reads, 'records': records, 'subjects': N_SUBJECTS,
               'text_bytes': size, 'reps': a.reps,
               'package_root': os.path.basename(os.path.relpath(
                   os.path.abspath(a.package_root), ROOT)),
               'cpus': len(os.sched_getaffinity(0)), 'configs': {}}
        for which, command in configs:
            key = f'{which}-{command}'
            for new in routes:      # warm-up: page cache, first contexts
                one_run(inputs, tmp, which, command, new, workflow, ROUTES,
                        digests=False)
            print(f'{key}: warmed up', flush=True)
            times = {r: [] for r in routes}
            digests, seen = {}, {}
            for rep in range(a.reps):
                for new in routes:
                    dt, dg, rt = one_run(inputs, tmp, which, command, new,
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
                      f' tables {digests[new]["table_sha256"][:16]}, maps '
                      f'{digests[new]["map_sha256"][:16]} '
                      f'({digests[new]["map_files"]} files, '
                      f'{digests[new]["map_bytes"]} bytes); {seen[new]}',
                      flush=True)
            if len(routes) == 2:
                res['device_over_host'] = res['host']['median_s'] / \
                    res['device']['median_s']
            said = {(d['table_sha256'], d['map_sha256'])
                    for d in digests.values()}
            if a.cross:
                dt, dg, rt = cross_run(inputs, tmp, which, command, workflow,
                                       ROUTES)
                res['cross'] = dict(dg, seconds=dt, routes=rt)
                print(f'{key} one file per sample, not demultiplexed: '
                      f'{dt:.3f} s; tables {dg["table_sha256"][:16]}, maps '
                      f'{dg["map_sha256"][:16]} ({dg["map_files"]} files, '
                      f'{dg["map_bytes"]} bytes); {rt}', flush=True)
                said.add((dg['table_sha256'], dg['map_sha256']))
            if expect is not None:
                said |= {(d['table_sha256'], d['map_sha256'])
                         for k, d in expect[key].items() if isinstance(d, dict)}
            if len(said) > 1:
                raise SystemExit(f'{key}: different tables or maps: {said}')
            if a.json:      # (after every configuration: a run cut short keeps what it has)
                os.makedirs(os.path.dirname(os.path.abspath(a.json)),
                            exist_ok=True)
                with open(a.json, 'w') as fh:
                    json.dump(out, fh, indent=1, sort_keys=True)
                    fh.write('\n')


if __name__ == '__main__':
    main()
