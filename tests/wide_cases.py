"""The input of the wide-table CLI case, rebuilt from a seed wherever it is
needed: tests/golden/make_wide_reference.py runs the reference on it, and
tests/test_gpu_weigh_wide_cli.py runs this package on the same bytes.

Three samples of simple-map alignments.  The first two name 1 310 000
distinct subjects between them -- more than the 1 299 456 the team layout of
the weighted histogram takes (csrc/wk_weigh_wide.hpp) --, the third names
800 000 of those again: its blocks bring no new subject, so as SAM text they
are the one-kernel tokenizer's to keep (a block with unknown subjects goes
back to the six kernels, and after two such blocks in a row the one kernel is
left out for a few blocks: the third sample is long enough to see it back).
Most reads have one hit, one in ten 2..16, and a subject-to-genus map is named
after its rank.  A sample's records are a permutation of (some of) its
subjects, so the subjects of a read are distinct.
"""
import hashlib
import os

import numpy as np

SEED = 20261019
N_SUBJECTS = 1_310_000
N_GENERA = 5003
RANK = 'genus'
SAMPLES = {'S1': (0, 800_000), 'S2': (500_000, N_SUBJECTS), 'S3': None}
N_KNOWN = 800_000         # records of S3, which names known subjects only
ARGS = ['--rank', 'none,' + RANK, '--map-as-rank', '--to-tsv', '--no-exe']


def records(sample):
    """(read number of every record, subject number of every record)."""
    rng = np.random.default_rng([SEED, sorted(SAMPLES).index(sample)])
    if SAMPLES[sample] is None:
        subj = rng.permutation(N_SUBJECTS)[:N_KNOWN]
    else:
        lo, hi = SAMPLES[sample]
        subj = lo + rng.permutation(hi - lo)
    n = subj.size
    size = np.where(rng.random(n) < 0.9, 1, rng.integers(2, 17, n))
    ends = np.cumsum(size)
    ends = ends[ends < n]
    read_of = np.zeros(n, np.int64)
    read_of[ends] = 1
    return np.cumsum(read_of), subj


def map_text(sample):
    read_of, subj = records(sample)
    return ''.join(['R%07d\tC%07d\n' % rs
                    for rs in zip(read_of.tolist(), subj.tolist())]).encode()


def sam_text(sample):
    read_of, subj = records(sample)
    return ''.join(['R%07d\t0\tC%07d\t1\t42\t50M\t*\t0\t0\t*\t*\n' % rs
                    for rs in zip(read_of.tolist(), subj.tolist())]).encode()


def genus_map_text():
    s = np.arange(N_SUBJECTS, dtype=np.int64)
    g = (s * 7919 + s // 977) % N_GENERA
    return ''.join(['C%07d\tG%04d\n' % sg
                    for sg in zip(s.tolist(), g.tolist())]).encode()


def write_inputs(root, fmt):
    """The alignment directory and the map under ``root``; returns the command
    line of `woltka classify` without --output."""
    aln = os.path.join(root, 'aln_' + fmt)
    os.makedirs(aln, exist_ok=True)
    for sample in SAMPLES:
        with open(os.path.join(aln, f'{sample}.{fmt}'), 'wb') as f:
            f.write(map_text(sample) if fmt == 'map' else sam_text(sample))
    gmap = os.path.join(root, RANK + '.map')
    if not os.path.isfile(gmap):
        with open(gmap, 'wb') as f:
            f.write(genus_map_text())
    return ['--input', aln, '--format', fmt, '--map', gmap] + ARGS


def digest(path):
    """What is kept of a table: sha256, rows, the first and the last ten."""
    with open(path, 'rb') as f:
        blob = f.read()
    lines = blob.decode().splitlines()
    return {'sha256': hashlib.sha256(blob).hexdigest(), 'rows': len(lines),
            'head': lines[:10], 'tail': lines[-10:]}


def digests(out_dir):
    return {fn: digest(os.path.join(out_dir, fn))
            for fn in sorted(os.listdir(out_dir))}
