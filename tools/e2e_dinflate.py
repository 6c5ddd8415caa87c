#!/usr/bin/env python3
"""`woltka classify -i S1.sam.gz --rank phylum,genus,species` on a BGZF file,
end to end: the host inflater's route (`WOLTKA_NO_DINFLATE=1`: the file is
inflated by csrc/wk_inflate.cpp on the host's threads and the text crosses the
link, the route before csrc/wk_dinflate.hpp) against the device route (the
compressed members cross the link and are inflated in HBM), alternating in one
process after a warm-up of each.

Config-3-shaped SAM text (`bench.lca_problem`, 100 k subjects under 2 M
nodes, written by the generator of bench.py), deflated as BGZF -- members of
65 280 bytes of text, zlib level 6 -- by 16 worker processes; the tool says
how long that took and what it came to.  A second, smaller file carries 150
bases of SEQ / QUAL per line (bench.py's `lca_seqqual` shape): there the old
route trims the text on the host before the link and the new one cannot.

    python tools/e2e_dinflate.py --records 50000000 --reps 3 \\
        --json profiles/dinflate_e2e.json

Prints per file and route the median and min-max of the wall time, the host
CPU seconds of the call (all threads), records/s and the sha256 over the
tables (equal between the routes, or the tool fails).  `--route new --reps 1
--no-seqqual` is the run to put under `rocprofv3 --kernel-trace
--output-format csv`; `--trace <kernel_trace.csv> --csv
profiles/dinflate_kernel_stats.csv --text-bytes N` then sums the dispatches
of every kernel of the traced run and gives the inflate kernel's bytes of
text per second."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import re
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from woltka_amd.hostio import ROUTES  # noqa: E402
from woltka_amd.workflow import workflow  # noqa: E402

RANKS = 'phylum,genus,species'
PIECE = 65280
HEAD = b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00'
EOF_BLOCK = HEAD + struct.pack('<H', 27) + b'\x03\x00' + b'\0' * 8


def trace_summary(trace, out_csv, text_bytes):
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
    lines = ['kernel,dispatches,total_ms,mean_us,share_of_kernel_time,text_GB_per_s']
    for name, (n, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        rate = f'{text_bytes / ns:.3f}' if name == 'dinflate_kernel' and text_bytes else ''
        lines.append(f'{name},{n},{ns / 1e6:.3f},{ns / n / 1e3:.2f},'
                     f'{ns / total:.4f},{rate}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out_csv:
        with open(out_csv, 'w') as fh:
            fh.write(text)


def _members(args):
    path, lo, hi = args
    out = []
    with open(path, 'rb') as f:
        f.seek(lo)
        data = f.read(hi - lo)
    for i in range(0, len(data), PIECE):
        piece = data[i:i + PIECE]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        out.append(HEAD + struct.pack('<H', 18 + len(body) + 8 - 1) + body +
                   struct.pack('<II', zlib.crc32(piece), len(piece)))
    return b''.join(out)


def to_bgzf(src, dst, workers=16, span=PIECE * 256):
    """`src` as BGZF in `dst`; returns (seconds, compressed bytes)."""
    from multiprocessing import Pool
    size = os.path.getsize(src)
    t0 = time.perf_counter()
    with Pool(workers) as pool, open(dst, 'wb') as out:
        tasks = [(src, lo, min(size, lo + span)) for lo in range(0, size, span)]
        for blob in pool.imap(_members, tasks, chunksize=1):
            out.write(blob)
        out.write(EOF_BLOCK)
    return time.perf_counter() - t0, os.path.getsize(dst)


def write_inputs(tmp, name, prob, n_reads, seqqual):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    plain = os.path.join(tmp, name + '.sam')
    records, size = bench.write_sam_lca(plain, prob, n_reads, seqqual=seqqual)
    secs, comp = to_bgzf(plain, os.path.join(d, 'S1.sam.gz'))
    os.remove(plain)
    print(f'{name}: {records} records, {size / 1e9:.2f} GB of SAM -> '
          f'{comp / 1e9:.3f} GB of BGZF (level 6, 16 processes) in {secs:.1f} s',
          flush=True)
    return {'dir': d, 'records': records, 'text_bytes': size,
            'bgzf_bytes': comp, 'deflate_s': secs}


def tables_digest(out):
    h = hashlib.sha256()
    for fn in sorted(os.listdir(out)):
        h.update(fn.encode() + b'\0')
        with open(os.path.join(out, fn), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def one_run(inp, nodes, tmp, new):
    if new:
        os.environ.pop('WOLTKA_NO_DINFLATE', None)
    else:
        os.environ['WOLTKA_NO_DINFLATE'] = '1'
    out = tempfile.mkdtemp(dir=tmp)
    ROUTES.clear()
    t0, c0 = time.perf_counter(), time.process_time()
    with contextlib.redirect_stdout(io.StringIO()):
        workflow(input_fp=inp['dir'], input_fmt='sam', nodes_fps=[nodes],
                 ranks=RANKS, output_fmt=False,
                 output_fp=os.path.join(out, 'tables'))
    dt, cpu = time.perf_counter() - t0, time.process_time() - c0
    routes = dict(ROUTES)
    if new != bool(routes.get('dinflate')):
        raise SystemExit(f'the run took another route than asked: {routes}')
    return dt, cpu, tables_digest(os.path.join(out, 'tables')), routes


def measure(inp, nodes, tmp, routes, reps):
    for new in routes:          # warm-up: page cache, first contexts
        one_run(inp, nodes, tmp, new)
    times, cpus = {r: [] for r in routes}, {r: [] for r in routes}
    digests, seen = {}, {}
    for _ in range(reps):
        for new in routes:
            dt, cpu, dg, rt = one_run(inp, nodes, tmp, new)
            times[new].append(dt)
            cpus[new].append(cpu)
            digests[new], seen[new] = dg, rt
    out = {k: v for k, v in inp.items() if k != 'dir'}
    for new in routes:
        t = times[new]
        label = 'device' if new else 'host'
        out[label] = {'median_s': statistics.median(t), 'min_s': min(t),
                      'max_s': max(t), 'times_s': t,
                      'host_cpu_s': statistics.median(cpus[new]),
                      'records_per_s': inp['records'] / statistics.median(t),
                      'tables_sha256': digests[new], 'routes': seen[new]}
        print(f'  {label} inflate: median {statistics.median(t):.3f} s (min '
              f'{min(t):.3f}, max {max(t):.3f}) = '
              f'{inp["records"] / statistics.median(t) / 1e6:.1f} M records/s, '
              f'{statistics.median(cpus[new]):.2f} s of host CPU; tables '
              f'{digests[new][:16]}; {seen[new]}', flush=True)
    if len(routes) == 2:
        out['device_over_host'] = out['host']['median_s'] / out['device']['median_s']
    if len(set(digests.values())) > 1:
        raise SystemExit(f'the routes wrote different tables: {digests}')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=50_000_000)
    ap.add_argument('--seqqual-records', type=int, default=5_000_000)
    ap.add_argument('--no-seqqual', action='store_true')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--route', choices=['both', 'new', 'old'], default='both')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--trace', default=None,
                    help='summarise this rocprofv3 kernel trace (CSV) and stop')
    ap.add_argument('--csv', default=None)
    ap.add_argument('--text-bytes', type=int, default=0)
    a = ap.parse_args()
    if a.trace:
        trace_summary(a.trace, a.csv, a.text_bytes)
        return
    routes = [True, False] if a.route == 'both' else [a.route == 'new']
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        reads = max(1000, int(a.records / 4.75))
        prob = bench.lca_problem(1002, reads / 50_000_000)
        reads = min(reads, int(prob['qoff'].size - 1))
        nodes = os.path.join(tmp, 'nodes.dmp')
        bench.write_nodes_dmp(nodes, prob['hier'])
        out = {'ranks': RANKS, 'reps': a.reps,
               'cpus': len(os.sched_getaffinity(0)), 'member_text_bytes': PIECE}
        inp = write_inputs(tmp, 'config3', prob, reads, 0)
        out['config3'] = measure(inp, nodes, tmp, routes, a.reps)
        if not a.no_seqqual:
            few = min(reads, max(1000, int(a.seqqual_records / 4.75)))
            inp = write_inputs(tmp, 'config3_seqqual', prob, few, 150)
            out['config3_seqqual'] = measure(inp, nodes, tmp, routes, a.reps)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
