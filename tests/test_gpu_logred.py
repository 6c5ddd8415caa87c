"""The contribution log of `--sizes` jobs reduced on the device
(csrc/wk_logred.hpp) through the ABI: `log_reduce` + `sized_fetch` against
`np.unique` over the log that `log_fetch` downloads for the same staged chunk
(sized jobs write nothing but the log, so a staged chunk is classified twice).
The new kernels are never compared with themselves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HIER = {}


def _hier():
    if not _HIER:
        from woltka_amd import synth
        rng = np.random.default_rng(77)
        p = synth.lca_problem(rng, n_nodes=3000, n_subjects=50, n_reads=10,
                              with_names=False)
        _HIER['h'] = p['hier']
    return _HIER['h']


def _context(log_cap=1 << 20):
    from woltka_amd import _native as nat
    h = _hier()
    c = nat.Context(0)
    c.set_tree(h.parent, h.last, h.rank_code)
    c.build_rank_table(0, h.rank_codes['genus'])
    c.build_rank_table(1, h.rank_codes['phylum'])
    c.counts_reserve(1 << 12)
    c.log_reserve(log_cap)
    return c


def _job(mode, slot=0, flags=0, major=0.0):
    from woltka_amd import _native as nat
    return nat.Job(mode, slot, flags | nat.F_SIZED, 0, major)


def _as_dict(rows, counts):
    keys = list(map(tuple, rows.tolist()))
    out = dict(zip(keys, counts.tolist()))
    assert len(out) == len(keys), 'a row appears twice'
    return out


def _expected(rows):
    """{row: times it occurs} of a fetched log, by numpy."""
    if not rows.shape[0]:
        return {}
    u, n = np.unique(rows, axis=0, return_counts=True)
    return _as_dict(u, n)


def _qoff(sizes):
    q = np.zeros(len(sizes) + 1, dtype=np.int32)
    np.cumsum(sizes, out=q[1:])
    return q


def _fetch_then_reduce(c, jobs):
    """The staged chunk classified twice: log_fetch + numpy, then log_reduce +
    sized_fetch; every assertion the two must meet.  Returns the expected
    dict."""
    s0 = c.stats()
    c.classify_staged(jobs)
    s1 = c.stats()
    want = _expected(c.log_fetch().copy())
    c.classify_staged(jobs)
    s2 = c.stats()
    assert s1['n_reads'] > s0['n_reads']
    for k in s2:        # one more pass over the same chunk
        assert s2[k] - s1[k] == s1[k] - s0[k], k
    held = c.sized_pending()
    n_in, n_distinct = c.log_reduce()
    assert c.sized_pending() == (held[0] + n_distinct, held[1])     # (no flush of words is counted)
    rows, counts = c.sized_fetch()
    got = _as_dict(rows, counts)            # (asserts that no row appears twice)
    assert got == want
    assert (counts > 0).all()
    assert int(counts.sum()) == n_in == sum(want.values())
    assert n_distinct == len(want) == rows.shape[0]
    assert c.counts_fetch()[0].size == 0    # (sized jobs count nothing)
    assert c.stats() == s2                  # (the reduction is not a pass over reads)
    assert c.sized_pending()[0] == 0
    return want


def test_empty_log():
    """Every read is unassigned (its subject is outside the tree, the job asks
    for a genus) and the job lacks F_UNASSIGNED: nothing is logged."""
    from woltka_amd import _native as nat
    n_nodes = _hier().n_nodes
    with _context() as c:
        jobs = [_job(nat.MODE_RANK, 0)]
        subj = (n_nodes + np.arange(500)).astype(np.int32)
        c.chunk_stage(subj, _qoff([1] * 500), group=2)
        c.classify_staged(jobs)
        assert c.log_fetch().shape[0] == 0
        c.classify_staged(jobs)
        held = c.sized_pending()
        assert c.log_reduce() == (0, 0)
        assert c.sized_pending() == held == (0, 0)
        assert c.sized_fetch()[0].shape == (0, 4)


def test_one_row():
    from woltka_amd import _native as nat
    with _context() as c:
        c.chunk_stage(np.array([5], np.int32), _qoff([1]), group=4)
        want = _fetch_then_reduce(c, [_job(nat.MODE_NONE)])
        assert list(want.values()) == [1]


def test_one_row_300001_times():
    """The hot-row path: the LDS front of every workgroup, the flush of all
    workgroups into one global slot, a row count that is no multiple of 64 or
    of the workgroup size."""
    from woltka_amd import _native as nat
    n = 300_001
    with _context() as c:
        c.chunk_stage(np.full(n, 9, np.int32), _qoff([1] * n), group=1)
        want = _fetch_then_reduce(c, [_job(nat.MODE_NONE)])
        assert list(want.values()) == [n]


def test_all_rows_distinct():
    """200 000 distinct rows: far more than the LDS fronts of a workgroup hold,
    the global table at its planned load, appends from nearly every wave of
    the emit kernel."""
    from woltka_amd import _native as nat
    n = 200_000
    rng = np.random.default_rng(3)
    with _context() as c:
        subj = (_hier().n_nodes + rng.permutation(n)).astype(np.int32)
        c.chunk_stage(subj, _qoff([1] * n), group=0)
        want = _fetch_then_reduce(c, [_job(nat.MODE_NONE)])
        assert len(want) == n and set(want.values()) == {1}


def _fields(row):
    f, s, meta, g = row
    return (f, s, meta >> 16, meta & 0xFFFF, g)     # feature, subject, job, divisor, group


def _has_pair_differing_only_in(rows, field):
    seen = {}
    for r in rows:
        x = _fields(r)
        seen.setdefault(x[:field] + x[field + 1:], set()).add(x[field])
    return any(len(v) > 1 for v in seen.values())


def test_rows_that_differ_in_one_field():
    """Pairs of rows equal in all but the divisor, the group, the job or the
    subject: all 128 bits decide."""
    from woltka_amd import _native as nat
    rng = np.random.default_rng(11)
    with _context() as c:
        genus = c.get_rank_table(0)
        # three nodes of one genus and some of others
        ids, n_of = np.unique(genus[genus >= 0], return_counts=True)
        g0 = int(ids[np.argmax(n_of)])
        same = np.flatnonzero(genus == g0)[:3].tolist()
        assert len(same) == 3
        others = np.flatnonzero((genus >= 0) & (genus != g0))[:25].tolist()
        a, a2, a3 = same
        pool = same + others
        reads = [[a], [a, a2], [a, a2, others[0]], [a2], [a3, a], [others[0]],
                 [others[1], others[2]], [a, a2, a3, others[3], others[4]]]
        for _ in range(120):
            k = int(rng.integers(1, 5))
            reads.append(rng.choice(pool, k, replace=False).tolist())
        # the same reads under two groups; a few reads belong to no group
        half = len(reads)
        groups = [3] * half + [5] * half
        reads = reads + reads
        for i in rng.choice(np.arange(8, half), 9, replace=False).tolist():
            groups[i + half * (i % 2)] = -1     # (none of the hand-made reads)
        subj = np.array([s for r in reads for s in r], np.int32)
        c.chunk_stage(subj, _qoff([len(r) for r in reads]),
                      group=np.array(groups, np.int32))
        jobs = [_job(nat.MODE_NONE),
                _job(nat.MODE_RANK, 0, nat.F_UNIQ | nat.F_UNASSIGNED),
                _job(nat.MODE_RANK, 0, major=0.8)]
        want = _fetch_then_reduce(c, jobs)
        for field, name in ((3, 'divisor'), (4, 'group'), (2, 'job'), (1, 'subject')):
            assert _has_pair_differing_only_in(want, field), name
        assert all(g in (3, 5) for *_, g in want)


def test_skew():
    """One row 70 000 times, most rows once, three jobs."""
    from woltka_amd import _native as nat
    rng = np.random.default_rng(5)
    with _context() as c:
        genus, phylum = c.get_rank_table(0), c.get_rank_table(1)
        nodes = np.flatnonzero((genus >= 0) & (phylum >= 0))
        hot = int(nodes[7])
        once = _hier().n_nodes + np.arange(20_000)
        few = rng.choice(nodes, 3_000)
        subj = np.concatenate((np.full(70_000, hot), once, few))
        subj = subj[rng.permutation(subj.size)].astype(np.int32)
        c.chunk_stage(subj, _qoff([1] * subj.size), group=6)
        jobs = [_job(nat.MODE_NONE),
                _job(nat.MODE_RANK, 0, nat.F_UNASSIGNED),
                _job(nat.MODE_RANK, 1, nat.F_UNASSIGNED)]
        want = _fetch_then_reduce(c, jobs)
        n = np.array(list(want.values()))
        assert n.max() >= 70_000 and (n == 1).sum() * 2 > n.size
        assert 150_000 < n.sum() < 300_000


def test_overflow():
    """A log that overflowed: the error of `log_fetch`, the pile untouched;
    after a larger reservation the re-run is exact."""
    from woltka_amd import _native as nat
    rng = np.random.default_rng(8)
    with _context(log_cap=1000) as c:
        subj = rng.integers(0, 700, 5000).astype(np.int32)
        c.chunk_stage(subj, _qoff([1] * subj.size), group=2)
        jobs = [_job(nat.MODE_NONE)]
        c.classify_staged(jobs)
        held = c.sized_pending()
        with pytest.raises(OverflowError):
            c.log_reduce()
        assert c.sized_pending() == held == (0, 0)
        c.log_reserve(8000)
        want = _fetch_then_reduce(c, jobs)
        assert sum(want.values()) == 5000


def test_two_reduces_one_fetch():
    """Two chunks under different groups before one fetch: the second append
    lands behind the first, across a growth of the pile's buffers (the first
    chunk leaves a pile of a few rows)."""
    from woltka_amd import _native as nat
    rng = np.random.default_rng(9)
    with _context() as c:
        jobs = [_job(nat.MODE_NONE)]
        chunks = [(rng.integers(0, 5, 40).astype(np.int32), 1),
                  (rng.integers(0, 30_000, 90_000).astype(np.int32), 2)]
        want = {}
        for subj, group in chunks:
            c.chunk_stage(subj, _qoff([1] * subj.size), group=group)
            c.classify_staged(jobs)
            want.update(_expected(c.log_fetch().copy()))
            c.classify_staged(jobs)
            before = c.sized_pending()[0]
            n_in, n_distinct = c.log_reduce()
            assert n_in == subj.size
            assert c.sized_pending()[0] == before + n_distinct
        assert {g for *_, g in want} == {1, 2}
        rows, counts = c.sized_fetch()
        assert _as_dict(rows, counts) == want
        assert int(counts.sum()) == 90_040 and (counts > 0).all()
        assert c.sized_pending() == (0, 0)
