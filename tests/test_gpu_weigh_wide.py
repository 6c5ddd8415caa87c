"""The wide layout of the weighted histogram (csrc/wk_weigh_wide.hpp): packed
records of an unsliced accumulation partitioned by slice of the subject table
(count, scan, scatter), then histogrammed bucket by bucket -- what
`wk_words_flush` takes for tables of more than 32 slices (1 299 456 subjects),
up to the packed word's 2^23.

Kernel level, through `nat.Context`.  Expected tables come from the C oracle
(classify.assign_none / assign_rank + classify.counter restated; classify.py:
32-51, 81-127, 144-171) or, for flat jobs, from an exact integer sum of
720720 / size per record.  The tree is regular (8 phyla x 64 genera x 16 384
leaves) so that every one of 2^23 subjects is a leaf of its own: a record
counted for the wrong subject changes the `none` table.  It is built once.

Knobs (include/woltka_hip_measure.h): "weigh_wide" = 1 opens an accumulation
unsliced and flushes it through the wide layout at any table size,
"weigh_wide_wgs" caps the histogram's workgroups.  Tiles: the scatter takes
8 192 words per workgroup and round, the histogram 4 096.
"""
import functools
import types

import numpy as np
import pytest

from helpers import assert_same_counts, oracle_table
from woltka_amd import _native as nat
from woltka_amd import synth

pytestmark = pytest.mark.gpu

BINS = 40608                    # kSliceBins: subjects per bucket
TEAM_MAX = 32 * BINS            # 1 299 456: the largest table of the team layout
SUBJ_MAX = 1 << 23
N_BUCKETS = -(-SUBJ_MAX // BINS)            # 207
SCATTER_TILE, BINS_TILE = 8192, 4096
L = nat.WEIGHT_L
P, Q, R = 8, 64, 16384          # phyla, genera per phylum, leaves per genus


@functools.lru_cache(maxsize=None)
def _tree():
    """Pre-order arrays of the regular tree and the node of every leaf."""
    per_genus, per_phylum = 1 + R, 1 + Q * (1 + R)
    n = 1 + P * per_phylum
    v = np.arange(n, dtype=np.int64)
    inside = (v - 1) % per_phylum                  # position inside its phylum
    phylum = 1 + (v - 1) // per_phylum * per_phylum
    in_genus = (inside - 1) % per_genus
    genus = phylum + 1 + (inside - 1) // per_genus * per_genus
    is_phylum = (v > 0) & (inside == 0)
    is_genus = (v > 0) & ~is_phylum & (in_genus == 0)
    is_leaf = (v > 0) & ~is_phylum & ~is_genus
    parent = np.where(is_phylum, 0, np.where(is_genus, phylum, genus))
    last = np.where(is_phylum, phylum + per_phylum - 1,
                    np.where(is_genus, genus + per_genus - 1, v))
    parent[0], last[0] = 0, n - 1
    rank = np.zeros(n, np.int32)
    rank[is_phylum] = synth.RANK_CODES['phylum']
    rank[is_genus] = synth.RANK_CODES['genus']
    leaves = np.flatnonzero(is_leaf).astype(np.int32)
    assert leaves.size == SUBJ_MAX
    return types.SimpleNamespace(
        parent=parent.astype(np.int32), last=last.astype(np.int32),
        rank_code=rank, leaves=leaves, rank_codes=synth.RANK_CODES)


def _jobs():
    return [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0),
            nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0),
            nat.Job(nat.MODE_RANK, 1, 0, 0, 0.0)]


def _specs(h):
    return [(nat.MODE_NONE, 0, 0, 0.0),
            (nat.MODE_RANK, h.rank_codes['genus'], 0, 0.0),
            (nat.MODE_RANK, h.rank_codes['phylum'], 0, 0.0)]


def _context():
    h = _tree()
    c = nat.Context(0)
    c.set_tree(h.parent, h.last, h.rank_code)
    c.build_rank_table(0, h.rank_codes['genus'])
    c.build_rank_table(1, h.rank_codes['phylum'])
    c.counts_reserve(1 << 21)
    c.profile_kernels(True)
    return c


@pytest.fixture(scope='module')
def wctx():
    c = _context()
    yield c
    c.close()


_TUNED = set()      # contexts whose wide knobs are not at their defaults


def _fresh(c, n_subjects, wide=0, wgs=0):
    """Empty counts, the knobs as asked, a table of n_subjects.  (The knobs are
    touched only where a test has moved them: the tests of the default route
    run as the command does.)"""
    c.counts_clear()
    if wide or wgs or c in _TUNED:
        c.tune('weigh_wide', wide)
        c.tune('weigh_wide_wgs', wgs)
        (_TUNED.add if wide or wgs else _TUNED.discard)(c)
    c.set_subjects(_tree().leaves[:n_subjects])


def _words(sidx, qoff):
    off = np.asarray(qoff, np.int64)
    size = np.diff(off)
    w = np.asarray(sidx).astype(np.uint32)
    w |= (np.arange(w.size, dtype=np.int64) -
          np.repeat(off[:-1], size)).astype(np.uint32) << np.uint32(23)
    w |= np.repeat(size, size).astype(np.uint32) << np.uint32(27)
    return w


def _single(sidx):
    """Reads of one hit each."""
    sidx = np.asarray(sidx, np.int64)
    return sidx, np.arange(sidx.size + 1, dtype=np.int64)


def _reads(rng, n_reads, lo, hi):
    """Reads of 1 hit (half of them) or 2..16 distinct subjects of [lo, hi),
    ascending inside a read."""
    k = np.where(rng.random(n_reads) < 0.5, 1, rng.integers(2, 17, n_reads))
    read_of = np.repeat(np.arange(n_reads, dtype=np.int64), k)
    s = rng.integers(lo, hi, read_of.size)
    pairs = np.unique((read_of << 32) | s)
    cnt = np.bincount(pairs >> 32, minlength=n_reads)
    qoff = np.zeros(n_reads + 1, np.int64)
    np.cumsum(cnt, out=qoff[1:])
    return pairs & 0xFFFFFFFF, qoff


def _expect(sidx, qoff, group):
    h = _tree()
    return oracle_table(h.leaves[np.asarray(sidx, np.int64)],
                        np.asarray(qoff, np.int32), _specs(h), h, group=group)


def _flush(c, sidx, qoff, group, pieces=1):
    words = _words(sidx, qoff)
    n_reads = len(qoff) - 1
    assert c.words_begin(_jobs(), group)
    cuts = np.linspace(0, n_reads, pieces + 1).astype(np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        c.words_append(words[int(qoff[a]):int(qoff[b])], int(b - a))
    return c.counts_fetch()


def _check(c, sidx, qoff, group=5, pieces=1):
    c.counts_clear()
    keys, vals = _flush(c, sidx, qoff, group, pieces)
    assert_same_counts(keys, vals, *_expect(sidx, qoff, group))
    assert c.last_kernel_ms('weigh_wide') > 0
    assert c.last_kernel_ms('weigh_wide_part') > 0
    return keys, vals


def test_first_table_the_team_layout_cannot_take(wctx):
    """33 slices.  Before the wide layout this flush ended with ValueError,
    "subject table too large for the weighted histogram"."""
    n = TEAM_MAX + 1
    rng = np.random.default_rng(1)
    _fresh(wctx, n)
    seams = np.array([0, BINS - 1, BINS, TEAM_MAX - 1, TEAM_MAX])
    s1, q1 = _single(np.concatenate([seams, rng.integers(0, n, 40), seams]))
    s2, q2 = _reads(rng, 3000, 0, n)
    sidx = np.concatenate([s1, s2])
    qoff = np.concatenate([q1, q2[1:] + q1[-1]])
    keys, vals = _check(wctx, sidx, qoff, group=5)
    job, k, grp, feat = nat.decode_keys(keys)
    assert (grp == 5).all() and set(job.tolist()) == {0, 1, 2}


def test_largest_table(wctx):
    """2^23 subjects, 207 buckets: records at the first and the last subject of
    buckets 0, 32, 33 and 206 (the last one partial) only."""
    _fresh(wctx, SUBJ_MAX)
    ends = []
    for b in (0, 32, 33, N_BUCKETS - 1):
        ends += [b * BINS, min((b + 1) * BINS, SUBJ_MAX) - 1]
    assert ends[-1] == SUBJ_MAX - 1
    sidx, qoff = _single(np.repeat(ends, 3))
    _check(wctx, sidx, qoff)
    # ... and as reads that span the buckets
    sidx = np.array(sorted(ends) * 2)
    qoff = np.array([0, len(ends), 2 * len(ends)])
    _check(wctx, sidx, qoff)


def test_last_bucket_of_one_subject(wctx):
    n = 33 * BINS + 1
    _fresh(wctx, n)
    _check(wctx, *_single([n - 1]))
    _check(wctx, *_single([n - 1, 0, n - 2, n - 1]))


def test_all_records_in_one_high_bucket(wctx):
    """Every workgroup of the histogram walks bucket 150."""
    _fresh(wctx, SUBJ_MAX)
    rng = np.random.default_rng(2)
    sidx, qoff = _reads(rng, 25000, 150 * BINS, 151 * BINS)
    assert 90_000 < sidx.size < 250_000
    _check(wctx, sidx, qoff)


def test_fewer_workgroups_than_buckets(wctx):
    """Eight workgroups, a record in each of 207 buckets: a workgroup takes
    26 buckets in turn."""
    _fresh(wctx, SUBJ_MAX, wgs=8)
    rng = np.random.default_rng(3)
    at = np.arange(N_BUCKETS) * BINS
    at += rng.integers(0, SUBJ_MAX - at[-1], N_BUCKETS)
    _check(wctx, *_single(at))
    # ... and a few thousand reads all over the table
    _check(wctx, *_reads(rng, 4000, 0, SUBJ_MAX))


@pytest.mark.parametrize('n_records', [1, SCATTER_TILE - 1, SCATTER_TILE,
                                       SCATTER_TILE + 1, BINS_TILE - 1,
                                       BINS_TILE, BINS_TILE + 1])
def test_record_counts_at_the_tiles_ends(wctx, n_records):
    """Single-hit reads, two thirds of them on three subjects of bucket 20
    (one bucket's share of the stream passes the histogram's tile) and the
    others spread over the table."""
    n = TEAM_MAX + 1
    _fresh(wctx, n)
    rng = np.random.default_rng(n_records)
    sidx = rng.integers(0, n, n_records)
    hot = rng.random(n_records) < 2 / 3
    sidx[hot] = 20 * BINS + rng.integers(0, 3, int(hot.sum()))
    _check(wctx, *_single(sidx))
    # all of them in one bucket: exactly n_records words in its range
    _check(wctx, *_single(TEAM_MAX - 1 - rng.integers(0, 100, n_records)))


def test_reads_without_covered_records(wctx):
    """Words whose size field is 0 (reads of more than 16 hits travel another
    way) add nothing: alone, and between weighted words."""
    n = TEAM_MAX + 1
    _fresh(wctx, n)
    rng = np.random.default_rng(4)
    idle = rng.integers(0, n, 5000).astype(np.uint32)       # size 0
    assert wctx.words_begin(_jobs(), 2)
    wctx.words_append(idle, 300)
    keys, vals = wctx.counts_fetch()
    assert keys.size == 0
    assert wctx.last_kernel_ms('weigh_wide') > 0
    sidx, qoff = _reads(rng, 2000, 0, n)
    words = _words(sidx, qoff)
    mixed = np.empty(words.size + idle.size, np.uint32)
    where = np.zeros(mixed.size, bool)
    where[rng.choice(mixed.size, idle.size, replace=False)] = True
    mixed[where], mixed[~where] = idle, words
    assert wctx.words_begin(_jobs(), 2)
    wctx.words_append(mixed, len(qoff) - 1 + 300)
    assert_same_counts(*wctx.counts_fetch(), *_expect(sidx, qoff, 2))


def test_wraps_carry(wctx):
    """6 000 single-hit reads on one subject of bucket 0 and on one of bucket
    100: a 32-bit bin holds 5 959 of them."""
    _fresh(wctx, SUBJ_MAX)
    a, b = 17, 100 * BINS + 40000
    sidx, qoff = _single(np.tile([a, b], 6000))
    keys, vals = _check(wctx, sidx, qoff)
    job, k, grp, feat = nat.decode_keys(keys)
    none = job == 0
    assert sorted(vals[none].tolist()) == [6000 * L, 6000 * L]
    assert 6000 * L > 1 << 32
    leaves = _tree().leaves
    assert sorted(feat[none].tolist()) == sorted([leaves[a], leaves[b]])
    # the next sample finds clean bins and carries
    keys, vals = _check(wctx, *_single([a, b]))
    assert sorted(vals[nat.decode_keys(keys)[0] == 0].tolist()) == [L, L]


def test_subject_beyond_the_table():
    """A weighted word whose index is at or beyond n_subjects: the error the
    other layouts give.  (A context of its own: the call fails.)"""
    n = TEAM_MAX + 1
    c = _context()
    try:
        _fresh(c, n)
        for bad in (n, n + BINS, SUBJ_MAX - 1):
            sidx, qoff = _single([0, 5 * BINS, bad, n - 1])
            assert c.words_begin(_jobs(), 0)
            c.words_append(_words(sidx, qoff), len(qoff) - 1)
            with pytest.raises((ValueError, RuntimeError),
                               match='feature id outside'):
                c.counts_fetch()
            c.counts_clear()
        # a word without weight may name anything
        assert c.words_begin(_jobs(), 0)
        c.words_append(np.array([SUBJ_MAX - 1, n], np.uint32), 1)
        c.words_append(_words(*_single([n - 1])), 1)
        assert_same_counts(*c.counts_fetch(), *_expect(*_single([n - 1]), 0))
    finally:
        c.close()


def test_table_grows_past_the_team_layout_under_an_open_accumulation(wctx):
    rng = np.random.default_rng(6)
    _fresh(wctx, 1_200_000)
    s1, q1 = _reads(rng, 3000, 0, 1_200_000)
    assert wctx.words_begin(_jobs(), 1)
    wctx.words_append(_words(s1, q1), len(q1) - 1)
    wctx.set_subjects(_tree().leaves[:1_310_000])
    s2, q2 = _reads(rng, 3000, 1_200_000, 1_310_000)
    wctx.words_append(_words(s2, q2), len(q2) - 1)
    assert wctx.words_pending() == (s1.size + s2.size, 6000)
    sidx = np.concatenate([s1, s2])
    qoff = np.concatenate([q1, q2[1:] + q1[-1]])
    assert_same_counts(*wctx.counts_fetch(), *_expect(sidx, qoff, 1))
    assert wctx.last_kernel_ms('weigh_wide') > 0


def test_table_grows_from_streams_to_wide(wctx):
    """Opened sliced at 300 000 subjects; past 324 864 `words_roll` flushes
    and goes on unsliced; past 1 299 456 the flush is wide."""
    rng = np.random.default_rng(7)
    _fresh(wctx, 300_000)
    parts = []
    assert wctx.words_begin(_jobs(), 1)
    for lo, hi in ((0, 300_000), (300_000, 400_000), (400_000, 1_310_000)):
        wctx.set_subjects(_tree().leaves[:hi])
        s, q = _reads(rng, 3000, lo, hi)
        wctx.words_append(_words(s, q), len(q) - 1)
        parts.append((s, q))
    assert wctx.words_pending() == (parts[1][0].size + parts[2][0].size, 6000)
    sidx = np.concatenate([s for s, _ in parts])
    qoff = [np.zeros(1, np.int64)]
    for _, q in parts:
        qoff.append(q[1:] + qoff[-1][-1])
    assert_same_counts(*wctx.counts_fetch(),
                       *_expect(sidx, np.concatenate(qoff), 1))
    assert wctx.last_kernel_ms('weigh_wide') > 0


def test_two_samples_in_a_row(wctx):
    _fresh(wctx, SUBJ_MAX)
    rng = np.random.default_rng(8)
    sidx, qoff = _reads(rng, 5000, 0, SUBJ_MAX)
    a = nat.canonical_counts(*_check(wctx, sidx, qoff, group=1))
    wctx.counts_clear()
    b = nat.canonical_counts(*_check(wctx, sidx, qoff, group=1, pieces=3))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # another sample next to the first one's counts: both stay what they are
    s2, q2 = _reads(rng, 100, 0, 1000)
    keys, vals = _flush(wctx, s2, q2, 2)
    grp = nat.decode_keys(keys)[2]
    c = nat.canonical_counts(keys[grp == 1], vals[grp == 1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert_same_counts(keys[grp == 2], vals[grp == 2], *_expect(s2, q2, 2))


@pytest.mark.parametrize('slices', [3, 9])
def test_forced_wide_equals_the_other_layouts(wctx, slices):
    """The same 200 k reads through the default layout of a table of 3
    (streams) and of 9 slices (teams), through the wide layout, and through the
    general route (wk_chunk_stage + wk_classify_staged, histogram off)."""
    n = slices * BINS - 7
    rng = np.random.default_rng(slices)
    sidx, qoff = _reads(rng, 200_000, 0, n)
    # (a Zipf head on top: most records in one bucket)
    head = _single(n - 1 - synth.zipf_draw(rng, 2000, 100_000))
    sidx = np.concatenate([sidx, head[0]])
    qoff = np.concatenate([qoff, head[1][1:] + qoff[-1]])
    tables = []
    for wide in (0, 1):
        _fresh(wctx, n, wide=wide)
        keys, vals = _flush(wctx, sidx, qoff, 3, pieces=4)
        tables.append(nat.canonical_counts(keys, vals))
        if wide:
            assert wctx.last_kernel_ms('weigh_wide') > 0
    _fresh(wctx, n)
    wctx.tune('weigh', 0)
    wctx.chunk_stage(sidx.astype(np.int32), qoff.astype(np.int32), group=3,
                     subj_is_set=True, indexed=True)
    wctx.classify_staged(_jobs())
    tables.append(nat.canonical_counts(*wctx.counts_fetch()))
    wctx.tune('weigh', 1)
    for t in tables[1:]:
        assert np.array_equal(tables[0][0], t[0])
        assert np.array_equal(tables[0][1], t[1])
    assert tables[0][0].size > 100_000
