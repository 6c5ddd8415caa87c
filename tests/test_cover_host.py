"""Subject coverage on the device (`--outcov`, csrc/wk_cover.hpp), the parts
that need no GPU: when the route is chosen, the six calls of the C ABI, and the
numpy mirror of the merge at the size the device test uses.

The rows of the `merge` fixture (tests/golden/vectors/cover_device.json, made
by tests/golden/make_cover_reference.py from the reference's
range.merge_ranges) are regenerated here from their seed."""
import hashlib
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import load_vectors        # noqa: E402

ROWS_SEED, ROWS_N, ROWS_KEYS = 20261, 2_000_000, 3000


def cover_rows(seed=ROWS_SEED, n=ROWS_N, n_keys=ROWS_KEYS):
    """(key, beg, end) int32: ~2 M rows over `n_keys` keys under a Zipf law (a
    few keys hold most rows, thousands hold one), negative `beg`,
    `beg` up to 2^31 - 2, `end == beg`, `end < beg`, rows that touch the row
    before them (`beg == end` of it) and rows that miss it by one."""
    rng = np.random.default_rng(seed)
    p = np.arange(1, n_keys + 1, dtype=np.float64) ** -2.4
    p /= p.sum()
    key = rng.choice(n_keys, size=n, p=p).astype(np.int32)
    key = np.concatenate([key, np.arange(n_keys, dtype=np.int32)])
    m = key.size
    span = np.where(key < 8, 40_000_000, 300_000)   # the deep keys are long
    beg = (rng.random(m) * span).astype(np.int64) - 1000
    far = rng.random(m) < 0.001
    beg[far] = (1 << 31) - 2 - rng.integers(0, 500, int(far.sum()))
    length = rng.integers(0, 300, m)
    kind = rng.random(m)
    length[kind < 0.05] = 0
    end = beg + length
    neg = (kind >= 0.05) & (kind < 0.08)
    end[neg] = beg[neg] - rng.integers(1, 6, int(neg.sum()))
    t = np.flatnonzero((kind >= 0.08) & (kind < 0.14))
    t = t[t > 0]
    key[t] = key[t - 1]
    beg[t] = end[t - 1] + (kind[t] >= 0.11)
    end[t] = beg[t] + rng.integers(0, 200, t.size)
    end = np.minimum(end, (1 << 31) - 1)
    beg = np.minimum(beg, (1 << 31) - 2)
    return key, beg.astype(np.int32), end.astype(np.int32)


def rows_digest(key, beg, end):
    """sha256 over the merged ranges in (key, beg) order: the three columns as
    little-endian int32, one after the other."""
    h = hashlib.sha256()
    for col in (key, beg, end):
        h.update(np.ascontiguousarray(col, dtype='<i4').tobytes())
    return h.hexdigest()


def test_rows_have_what_the_fixture_promises():
    key, beg, end = cover_rows()
    count = np.bincount(key)
    assert count.size == ROWS_KEYS and count[:3].sum() > key.size // 2
    assert (count == 1).sum() > 1000
    assert (beg < 0).any() and beg.max() == (1 << 31) - 2
    assert (end == beg).sum() > 50_000 and (end < beg).sum() > 50_000


def test_numpy_mirror_reproduces_merge_ranges_at_two_million_rows():
    from woltka_amd.ranges import merge_intervals
    gold = load_vectors('cover_device.json')['merge']
    key, beg, end = cover_rows()
    assert key.size == gold['rows']
    k, b, e = merge_intervals(key.astype(np.int64), beg.astype(np.int64),
                              end.astype(np.int64))
    assert k.size == gold['n_ranges']
    assert rows_digest(k, b, e) == gold['sha256']


def test_binding_declares_the_six_calls():
    from woltka_amd import _native
    for name in ('wk_cover_begin', 'wk_dtok_cover_append', 'wk_cover_add',
                 'wk_cover_finish', 'wk_cover_fetch', 'wk_cover_reset'):
        assert name in _native.SYMBOLS
        assert hasattr(_native.load_library(), name)


ON = dict(fmt='sam', exclude=False, demux=False, strata=False, outmap=False,
          part=None, n_jobs_ok=True)


def test_eligibility_truth_table(monkeypatch):
    from woltka_amd.classify import cover_on_device
    monkeypatch.delenv('WOLTKA_NO_DCOVER', raising=False)
    for fmt in ('sam', 'b6o', 'paf'):
        assert cover_on_device(**dict(ON, fmt=fmt))
    for fmt in ('map', None, 'biom'):
        assert not cover_on_device(**dict(ON, fmt=fmt))
    # each excluded option alone turns it off
    for name, value in (('exclude', True), ('demux', True), ('strata', True),
                        ('outmap', True), ('part', (0, 100)),
                        ('n_jobs_ok', False)):
        assert not cover_on_device(**dict(ON, **{name: value})), name
    # and so does any combination of them
    for a, b in itertools.combinations(
            ('exclude', 'demux', 'strata', 'outmap'), 2):
        assert not cover_on_device(**dict(ON, **{a: True, b: True}))
    # subjects the files before have brought: the measured guard
    from woltka_amd.classify import COVER_MAX_SUBJECTS
    assert cover_on_device(**ON, n_subjects=COVER_MAX_SUBJECTS)
    assert not cover_on_device(**ON, n_subjects=COVER_MAX_SUBJECTS + 1)
    monkeypatch.setenv('WOLTKA_NO_DCOVER', '1')
    assert not cover_on_device(**ON)


# ---- the `runs` fixtures: alignment text regenerated from its seed -----------

TAX = os.path.join(ROOT, 'tests', 'golden', 'data', 'taxonomy')
TEXT_SAMPLES, TEXT_QUERIES = 3, 38_000      # ~200 k records a format

# (format, seed, ranks, trimsub, outcov_fmt): every format with `--rank none`,
# a given rank and `free` (the three kinds of job set the packed records
# take), with and without `--trim-sub`, every coordinate style
RUN_CASES = [
    ('sam', 11, 'none', None, 'bed'), ('sam', 11, 'genus', None, 'gff'),
    ('sam', 12, 'free', '_', '1i'), ('sam', 12, 'none', '_', 'bed'),
    ('b6o', 21, 'none', None, 'gff'), ('b6o', 22, 'genus', '_', 'bed'),
    ('b6o', 21, 'free', None, '1i'),
    ('paf', 31, 'none', None, '1i'), ('paf', 31, 'genus', None, 'bed'),
    ('paf', 32, 'free', '_', 'gff'),
]


def run_label(case):
    fmt, seed, ranks, trimsub, covfmt = case
    return f'{fmt}-{seed}-{ranks}-{"trim" if trimsub else "whole"}-{covfmt}'


def genome_ids():
    with open(os.path.join(TAX, 'taxid.map')) as fh:
        return [line.split('\t')[0] for line in fh if line.strip()]


def cover_text(fmt, seed, genes=False):
    """{sample: text} of `TEXT_SAMPLES` alignment files in `fmt`: queries of
    1-4 hits on the bundled taxonomy's genomes (a few take most hits;
    ``genes``: the subjects are `<genome>_<n>`, for `--trim-sub _`), only
    lines of shapes the device "ex" parsers keep."""
    import random
    rng = random.Random(seed)
    gids = genome_ids()
    weights = [1.0 / (i + 1) ** 1.2 for i in range(len(gids))]
    ops = 'MIDNSH=X'
    out = {}
    for si in range(TEXT_SAMPLES):
        lines = ['@HD\tVN:1.0\tSO:unsorted\n'] if fmt == 'sam' else []
        hits = rng.choices(range(1, 5), [5, 3, 1, 1], k=TEXT_QUERIES)
        picks = iter(rng.choices(gids, weights, k=sum(hits)))
        for qi, k in enumerate(hits):
            q = f'S{si}r{qi:06d}'
            paired = fmt == 'sam' and rng.random() < 0.4
            for _ in range(k):
                s = next(picks)
                if genes:
                    s = f'{s}_{rng.randrange(1, 40)}'
                pos = rng.randrange(1, 2_000_000)
                ln = rng.choice((50, 100, 150, 151, 250))
                if fmt == 'sam':
                    flag = rng.choice((99, 147, 355, 403, 65, 129)) \
                        if paired else rng.choice((0, 16, 256, 272))
                    r = rng.random()
                    if r < 0.6:
                        cigar = f'{ln}M'
                    elif r < 0.63:      # no reference span: end == beg
                        cigar = f'{ln}S' if r < 0.615 else f'{ln}I'
                    else:
                        cigar = ''.join(
                            f'{rng.randrange(1, 90)}{rng.choice(ops)}'
                            for _ in range(rng.randrange(2, 7)))
                    lines.append(f'{q}\t{flag}\t{s}\t{pos}\t{rng.randrange(43)}'
                                 f'\t{cigar}\t=\t0\t0\t*\t*\n')
                elif fmt == 'b6o':
                    a, b = pos, pos + ln - 1
                    if rng.random() < 0.5:      # reverse strand
                        a, b = b, a
                    lines.append(
                        f'{q}\t{s}\t{rng.randrange(800, 1001) / 10}\t{ln}\t'
                        f'{rng.randrange(5)}\t0\t1\t{ln}\t{a}\t{b}\t'
                        f'{rng.choice(("1e-30", "2.5e-8", "0.0"))}\t'
                        f'{rng.randrange(500, 3000) / 10}\n')
                else:
                    lines.append(
                        f'{q}\t{ln}\t0\t{ln}\t{rng.choice("+-")}\t{s}\t'
                        f'3000000\t{pos}\t{pos + ln}\t{ln - rng.randrange(9)}\t'
                        f'{ln}\t{rng.randrange(61)}\n')
        out[f'S{si}'] = ''.join(lines)
    return out


def run_kwargs(case, indir, outdir):
    """Arguments of `workflow` (the reference's and this package's alike)."""
    fmt, _, ranks, trimsub, covfmt = case
    kw = dict(input_fp=indir, input_fmt=fmt, ranks=ranks,
              output_fp=os.path.join(outdir, 'profile.tsv'),
              outcov_dir=os.path.join(outdir, 'cov'), outcov_fmt=covfmt)
    if ranks != 'none':
        kw.update(map_fps=[os.path.join(TAX, 'taxid.map')],
                  nodes_fps=[os.path.join(TAX, 'nodes.dmp')])
    if trimsub:
        kw['trimsub'] = trimsub
    return kw


def write_inputs(case, indir):
    fmt, seed, _, trimsub, _ = case
    os.makedirs(indir, exist_ok=True)
    for sample, text in cover_text(fmt, seed, genes=bool(trimsub)).items():
        with open(os.path.join(indir, f'{sample}.{fmt}'), 'w') as fh:
            fh.write(text)


def run_digests(outdir):
    """sha256 of the profile and of every <sample>.cov a run wrote."""
    def sha(path):
        with open(path, 'rb') as fh:
            return hashlib.sha256(fh.read()).hexdigest()
    cov = os.path.join(outdir, 'cov')
    return {'profile': sha(os.path.join(outdir, 'profile.tsv')),
            'cov': {x[:-4]: sha(os.path.join(cov, x))
                    for x in sorted(os.listdir(cov))}}


def test_run_cases_cover_what_the_fixture_promises():
    gold = load_vectors('cover_device.json')['runs']
    assert sorted(gold) == sorted(map(run_label, RUN_CASES))
    for fmt in ('sam', 'b6o', 'paf'):
        mine = [c for c in RUN_CASES if c[0] == fmt]
        assert {c[2] for c in mine} == {'none', 'genus', 'free'}
        assert {bool(c[3]) for c in mine} == {False, True}
    assert {c[4] for c in RUN_CASES} == {'bed', 'gff', '1i'}
    text = cover_text('sam', 11)
    assert len(text) == TEXT_SAMPLES
    assert sum(t.count('\n') for t in text.values()) > 150_000
