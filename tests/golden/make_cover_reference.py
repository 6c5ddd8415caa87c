#!/usr/bin/env python3
"""tests/golden/vectors/cover_device.json: what the REAL reference makes of
the inputs of tests/test_cover_host.py / tests/test_gpu_cover.py (build
container only; the inputs are regenerated from their seeds by the functions
of tests/test_cover_host.py, only digests are committed).

  merge   range.merge_ranges over the ~2 M rows of `cover_rows`, per key, the
          merged ranges concatenated in key order: their number and sha256
  runs    for every case of RUN_CASES the reference workflow's profile and
          <sample>.cov files: sha256 each

    python tests/golden/make_cover_reference.py      # ~2 min

The host route of this package must reproduce every digest before the file is
committed: `WOLTKA_NO_DCOVER=1 python tests/golden/make_cover_reference.py
check` runs it (on a machine with a device, like every classify call; it
needs no reference tree)."""
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import _refshim  # noqa: E402
import test_cover_host as T  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'cover_device.json')


def gen_merge():
    from woltka.range import merge_ranges
    key, beg, end = T.cover_rows()
    order = np.argsort(key, kind='stable')
    ks, bs, es = key[order], beg[order], end[order]
    cut = np.flatnonzero(np.diff(ks)) + 1
    K, B, E = [], [], []
    for lo, hi in zip([0] + cut.tolist(), cut.tolist() + [ks.size]):
        flat = np.stack([bs[lo:hi], es[lo:hi]], 1).reshape(-1).tolist()
        merged = merge_ranges(flat)
        K += [int(ks[lo])] * (len(merged) // 2)
        B += merged[0::2]
        E += merged[1::2]
    return {'seed': T.ROWS_SEED, 'rows': int(key.size), 'n_ranges': len(K),
            'sha256': T.rows_digest(K, B, E)}


def run_all(workflow):
    runs = {}
    for case in T.RUN_CASES:
        with tempfile.TemporaryDirectory() as tmp:
            indir = os.path.join(tmp, 'aln')
            T.write_inputs(case, indir)
            with contextlib.redirect_stdout(io.StringIO()):
                workflow(**T.run_kwargs(case, indir, tmp))
            runs[T.run_label(case)] = T.run_digests(tmp)
        print(T.run_label(case), flush=True)
    return runs


def main():
    if sys.argv[1:] == ['check']:
        from woltka_amd.workflow import workflow
        with open(OUT) as fh:
            gold = json.load(fh)
        got = run_all(workflow)
        bad = [k for k in gold['runs'] if got[k] != gold['runs'][k]]
        print('host route:', 'every digest reproduced' if not bad else bad)
        sys.exit(1 if bad else 0)
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    from woltka.workflow import workflow
    doc = {'merge': gen_merge(), 'runs': run_all(workflow)}
    with open(OUT, 'w') as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
