"""`--sizes` on the words route, host half: the vectorised fold of the device's
(row, count) pile equals a plain loop over the rows, and the gates that keep
the other inputs on the general route.  No device work."""
import numpy as np
import pytest


def _loop(acc, rows, counts, groups, job_base=0):
    """What `Folding._collect_log` does per distinct row."""
    for (f, s, meta, g), c in zip(rows.tolist(), counts.tolist()):
        key = (job_base + (meta >> 16), groups[g], f, s, meta & 0xFFFF)
        acc[key] = acc.get(key, 0) + c
    return acc


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_fold_equals_a_loop_over_the_rows(seed):
    from woltka_amd.routes.fold import fold_sized_rows
    rng = np.random.default_rng(seed)
    groups = [('S%d' % i, None) for i in range(4)] + [('S9', 'x'), ('S9', 'y')]
    n = 5000
    rows = np.stack([
        rng.integers(0, 40, n),                         # feature
        rng.integers(0, 25, n),                         # subject
        (rng.integers(0, 3, n) << 16) | rng.integers(1, 17, n),
        rng.integers(0, len(groups), n)], axis=1).astype(np.int32)
    # (keys repeat: 40 * 25 * 48 * 6 cells would hold them, yet rows are copied)
    rows[n // 2:] = rows[rng.integers(0, n // 2, n - n // 2)]
    counts = rng.integers(1, 1 << 40, n).astype(np.int64)
    want = _loop({}, rows, counts, groups)
    got = fold_sized_rows({}, rows, counts, groups)
    assert got == want
    assert all(type(v) is int for v in got.values())
    assert all(type(x) is int for k in got for x in (k[0], k[2], k[3], k[4]))
    # into a dict that holds keys already, in two pieces, with a job base
    half = n // 3
    want2 = _loop(_loop({}, rows[:half], counts[:half], groups, 8),
                  rows[half:], counts[half:], groups, 8)
    got2 = fold_sized_rows({}, rows[:half], counts[:half], groups, 8)
    assert fold_sized_rows(got2, rows[half:], counts[half:], groups, 8) == want2
    assert min(k[0] for k in got2) >= 8


def test_fold_of_nothing_and_of_extreme_fields():
    from woltka_amd import _native as nat
    from woltka_amd.routes.fold import fold_sized_rows
    acc = {'kept': 1}
    assert fold_sized_rows(acc, np.empty((0, 4), np.int32),
                           np.empty(0, np.int64), []) == {'kept': 1}
    groups = [None] * 3
    groups[2] = ('S', None)
    rows = np.array([[nat.FEATURE_UNASSIGNED, nat.MAX_FEATURE, (7 << 16) | 16, 2],
                     [0, 0, 1, 2],
                     [nat.FEATURE_UNASSIGNED, nat.MAX_FEATURE, (7 << 16) | 16, 2]],
                    dtype=np.int32)
    got = fold_sized_rows({}, rows, np.array([5, 7, 11], np.int64), groups)
    assert got == {(7, ('S', None), nat.FEATURE_UNASSIGNED, nat.MAX_FEATURE, 16): 16,
                   (0, ('S', None), 0, 0, 1): 7}


def test_gates(monkeypatch):
    """`sized_on_device`: plain classification of a whole file, unless
    WOLTKA_NO_DSIZES is set; `words_eligible` takes sized plain jobs only when
    told so, and never sized jobs that look at whole reads."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.words import WordsRoute
    monkeypatch.delenv('WOLTKA_NO_DSIZES', raising=False)
    monkeypatch.delenv('WOLTKA_NO_WORDS', raising=False)
    assert WordsRoute.sized_on_device(True, None)
    assert not WordsRoute.sized_on_device(False, None)
    assert not WordsRoute.sized_on_device(True, (0, 2))

    class E(WordsRoute):
        _replay = None
        _tok_identity = True
        use_tree = True
        sizes = {'a': 1}

    def engine(*jobs):
        e = E()
        e.jobs = [nat.Job(m, 0, f | nat.F_SIZED, 0, major) for m, f, major in jobs]
        return e
    plain = engine((nat.MODE_NONE, 0, 0.0), (nat.MODE_RANK, 0, 0.0))
    assert not plain.words_eligible()
    assert plain.words_eligible(sized=True)
    assert plain.words_eligible(identity=False, sized=True)
    for whole in ((nat.MODE_FREE, 0, 0.0), (nat.MODE_RANK, nat.F_UNIQ, 0.0),
                  (nat.MODE_RANK, nat.F_ABOVE, 0.0), (nat.MODE_RANK, 0, 0.8),
                  (nat.MODE_NONE, nat.F_UNIQ, 0.0)):
        assert not engine(whole).words_eligible(sized=True)
        assert not engine((nat.MODE_NONE, 0, 0.0), whole).words_eligible(sized=True)
    monkeypatch.setenv('WOLTKA_NO_DSIZES', '1')
    assert not WordsRoute.sized_on_device(True, None)
