#!/usr/bin/env python3
"""`woltka classify -i aln/ --rank none,free,genus --outmap maps/` and `...
--rank genus --trim-sub _ --name-as-id --outmap maps/` (doc/stratify.md,
Method II, step 1) on one sample, end to end: the read maps with taxon lists
on the device route (R1l: every block staged as a CSR chunk, counted with the
assignment codes left in HBM, the lists built and the lines formatted there,
csrc/wk_readmap_lists.hpp; only finished text crosses to the host) against
the host route (`WOLTKA_NO_DLISTMAPS=1`: the host tokenizer on all threads,
the codes copied back, `_multi_lists` in numpy and `wk_format_readmap` on
helper threads -- R3, every such call's route before), alternating in one
process after a warm-up of each.

One sample S1: the reads and hits of config 3 (`woltka_amd/synth.py::
lca_problem`, 100 k subjects under 2 M nodes) as SAM text in the page cache.
The second command reads the same records with ORF-style subject names
(`T0001234_7`: the gene's number is the record's, modulo 10) and shows the
names of names.dmp.

    python tools/e2e_readmap_lists.py --reads 12000000 --reps 3 \\
        --json profiles/readmap_lists_e2e.json

Prints per command and route the median and min-max of the wall time,
records/s and the sha256 over the tables and over the (inflated) map texts --
equal between the routes, or the tool fails.  `--package-root DIR` measures
the package of another tree (a checkout of the parent commit, built: there
`--route old` is the only route); `--expect FILE.json` then requires the
digests of that earlier result.  `--route new --reps 1 --only mixed` is the
run to put under `rocprofv3 --kernel-trace --output-format csv`; `--trace
<kernel_trace.csv> --csv profiles/readmap_lists_kernel_stats.csv` then sums
the dispatches of every kernel of the traced run; the kernels of
csrc/wk_readmap_lists.hpp and the ones they share with the other read-map
routes are marked."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import e2e_readmap_reads as E  # noqa: E402

N_SUBJECTS = E.N_SUBJECTS
COMMANDS = {'mixed': dict(ranks='none,free,genus'),
            'orf': dict(ranks='genus', trimsub='_', name_as_id=True)}
MARKED = ('readmap_lists_build_kernel', 'readmap_lists_write_kernel',
          'readmap_leaders_kernel', 'u64_tile_sum_kernel',
          'u64_tile_prefix_kernel', 'tile_scan_kernel',
          'strata_place_reads_kernel')


def write_inputs(tmp, n_reads, seed, bench, synth):
    """aln/S1.sam, orf/S1.sam, nodes.dmp and names.dmp; returns ({command:
    input directory}, nodes.dmp, names.dmp, records, bytes of SAM)."""
    rng = np.random.default_rng(seed)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=2_000_000, n_subjects=N_SUBJECTS, n_reads=n_reads,
        with_names=False))
    dirs = {'mixed': os.path.join(tmp, 'aln'), 'orf': os.path.join(tmp, 'orf')}
    for d in dirs.values():
        os.makedirs(d)
    records, size = bench.write_sam_lca(os.path.join(dirs['mixed'], 'S1.sam'),
                                        p, n_reads)
    # the same records under ORF names: `T<subject:07d>0<gene>` written with
    # nine digits, the zero then turned into the underscore
    qoff = p['qoff']
    read_of = np.repeat(np.arange(n_reads, dtype=np.int64),
                        np.diff(qoff[:n_reads + 1]))
    subj = p['subj'][:records].astype(np.int64)
    gene = np.arange(records, dtype=np.int64) % 10
    fp = os.path.join(dirs['orf'], 'S1.sam')
    size2 = bench.write_sam(fp, read_of, (subj * 100 + gene).astype(np.int64),
                            swidth=9)
    text = np.memmap(fp, dtype=np.uint8, mode='r+')
    head = int(np.flatnonzero(text[:64] == 10)[0]) + 1
    width = (size2 - head) // records
    if head + width * records != size2 or subj.max() * 100 + 9 >= 2 ** 31:
        raise SystemExit('the SAM writer left lines of several widths')
    rows = text[head:].reshape(records, width)
    at = 1 + 9 + 3 + 1 + 7          # R, read id, <tab>0<tab>, T, subject
    if not (rows[:3, at] == 48).all() or not (rows[:3, at - 8] == 84).all():
        raise SystemExit('the SAM writer put the subject elsewhere')
    rows[:, at] = 95
    text.flush()
    del rows, text
    nodes = os.path.join(tmp, 'nodes.dmp')
    bench.write_nodes_dmp(nodes, p['hier'])
    names = os.path.join(tmp, 'names.dmp')
    with open(names, 'w') as f:
        f.writelines(f'T{v:07d}\t|\ttaxon {v % 977} of {v}\t|\t\t|\t'
                     'scientific name\t|\n'
                     for v in range(p['hier'].n_nodes))
    return dirs, nodes, names, records, size


def one_run(inputs, tmp, command, new, workflow, ROUTES, digests=True):
    dirs, nodes, names = inputs[:3]
    if new:
        os.environ.pop('WOLTKA_NO_DLISTMAPS', None)
    else:
        os.environ['WOLTKA_NO_DLISTMAPS'] = '1'
    work = tempfile.mkdtemp(dir=tmp)
    out, maps = os.path.join(work, 'tables'), os.path.join(work, 'maps')
    kw = dict(COMMANDS[command], nodes_fps=[nodes])
    if kw.get('name_as_id'):
        kw['names_fps'] = [names]
    ROUTES.clear()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=dirs[command], input_fmt='sam', output_fmt=False,
                 output_fp=out, outmap_dir=maps, outmap_zip='none', **kw)
    dt = time.perf_counter() - t0
    routes = dict(ROUTES)
    if new != bool(routes.get('dreads_lists')) or \
            (new and routes.get('host_block')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    dg = None
    if digests:
        th, mh, n = hashlib.sha256(), hashlib.sha256(), 0
        files = [out] if os.path.isfile(out) else \
            [os.path.join(out, fn) for fn in sorted(os.listdir(out))]
        for fp in files:
            th.update(E.file_digest(fp)[0].encode())
        for dirpath, dirs_, fns in sorted(os.walk(maps)):
            dirs_.sort()
            for fn in sorted(fns):
                rel = os.path.relpath(os.path.join(dirpath, fn), maps)
                d, k = E.file_digest(os.path.join(dirpath, fn))
                mh.update(rel.encode() + b'\0' + d.encode())
                n += k
        dg = {'table_sha256': th.hexdigest(), 'map_sha256': mh.hexdigest(),
              'map_bytes': n}
    import shutil
    shutil.rmtree(work)
    return dt, dg, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=12_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--only', default=None, help='one command: mixed or orf')
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
        E.MARKED = MARKED
        E.trace_summary(a.trace, a.csv)
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
    commands = [c for c in COMMANDS if a.only in (None, c)]
    routes = [True, False] if a.route == 'both' else [a.route == 'new']
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        t0 = time.perf_counter()
        inputs = write_inputs(tmp, a.reads, 9, bench, synth)
        records, size = inputs[3:]
        print(f'{records} records of {a.reads} reads, {size / 1e9:.2f} GB of '
              f'SAM, written in {time.perf_counter() - t0:.0f} s', flush=True)
        out = {'reads': a.reads, 'records': records, 'subjects': N_SUBJECTS,
               'text_bytes': size, 'reps': a.reps,
               'package_root': os.path.basename(os.path.relpath(
                   os.path.abspath(a.package_root), ROOT)),
               'cpus': len(os.sched_getaffinity(0)), 'configs': {}}
        for key in commands:
            for new in routes:      # warm-up: page cache, first contexts
                one_run(inputs, tmp, key, new, workflow, ROUTES,
                        digests=False)
            print(f'{key}: warmed up', flush=True)
            times = {r: [] for r in routes}
            digests, seen = {}, {}
            for rep in range(a.reps):
                for new in routes:
                    dt, dg, rt = one_run(inputs, tmp, key, new, workflow,
                                         ROUTES, digests=rep == a.reps - 1)
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
