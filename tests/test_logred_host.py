"""The host half of the equivalence the device-side reduction of the `--sizes`
log relies on (routes/fold.py): `fold_sized_rows` over distinct rows with
counts gives the dict that the fetch route of `Folding._collect_log` builds
from the raw rows."""
import numpy as np

from woltka_amd.routes.fold import fold_sized_rows


def _raw_rows(rng, n, n_groups):
    """int32[n, 4] = (feature, subject, job << 16 | divisor, group) with many
    duplicates and with rows that differ in one field only."""
    feature = rng.integers(0, 6, n)
    feature[rng.random(n) < 0.1] = 0x0FFFFFFF        # 'Unassigned'
    subject = rng.integers(0, 5, n)
    job = rng.integers(0, 8, n)
    divisor = rng.integers(1, 5, n)
    divisor[rng.random(n) < 0.02] = 4095             # (a read of very many subjects)
    group = rng.integers(0, n_groups, n)
    return np.stack((feature, subject, (job << 16) | divisor, group),
                    axis=1).astype(np.int32)


def _fetch_route(acc, rows, groups, job_base):
    """The loop of `Folding._collect_log` on its fetch route."""
    uniq, cnt = np.unique(rows, axis=0, return_counts=True)
    for (f, s, meta, g), c in zip(uniq.tolist(), cnt.tolist()):
        key = (job_base + (meta >> 16), groups[g], f, s, meta & 0xFFFF)
        acc[key] = acc.get(key, 0) + c
    return acc


def _reduced(rng, rows):
    """What the device hands over: every distinct row once with its count, in
    no particular order."""
    uniq, cnt = np.unique(rows, axis=0, return_counts=True)
    mix = rng.permutation(uniq.shape[0])
    return uniq[mix], cnt[mix].astype(np.int64)


def test_reduced_rows_fold_like_raw_rows():
    rng = np.random.default_rng(2024)
    groups = [('S1', None), ('S2', None), ('S1', 'soil'), ('S3', 'gut')]
    rows = _raw_rows(rng, 20_000, len(groups))
    assert np.unique(rows, axis=0).shape[0] < rows.shape[0] // 2
    want = _fetch_route({}, rows, groups, 0)
    got = fold_sized_rows({}, *_reduced(rng, rows), groups, 0)
    assert got == want and sum(got.values()) == rows.shape[0]


def test_job_base_and_two_folds_into_one_acc():
    """Two chunks folded one after the other (the second batch of ranks has a
    job base of 8), with keys in common."""
    rng = np.random.default_rng(7)
    groups = [('A', None), ('B', 'x')]
    first, second, third = (_raw_rows(rng, n, len(groups)) for n in (5000, 3000, 4000))
    want, got = {}, {}
    for rows, base in ((first, 0), (second, 8), (third, 8)):
        _fetch_route(want, rows, groups, base)
        fold_sized_rows(got, *_reduced(rng, rows), groups, base)
    assert got == want
    assert {k[0] for k in got} == set(range(16))
    assert sum(got.values()) == 12_000


def test_rows_reduced_per_chunk_fold_like_one_log():
    """The pile holds the rows of several reduces before one fold: a row that
    two chunks have in common arrives twice, each time with its count."""
    rng = np.random.default_rng(13)
    groups = [('A', None), ('B', None), ('C', None)]
    a, b = _raw_rows(rng, 6000, 3), _raw_rows(rng, 6000, 3)
    want = _fetch_route(_fetch_route({}, a, groups, 0), b, groups, 0)
    ra, ca = _reduced(rng, a)
    rb, cb = _reduced(rng, b)
    got = fold_sized_rows({}, np.concatenate((ra, rb)),
                          np.concatenate((ca, cb)), groups, 0)
    assert got == want
    assert fold_sized_rows({}, np.empty((0, 4), np.int32), np.empty(0, np.int64), groups) == {}
