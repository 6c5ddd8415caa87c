"""bench.py's host side: the threaded generator of the headline's problem
returns the arrays of the synth functions it stands for, and `--dump-outputs`
turns a count table of several equal passes into the rows of one."""
import types

import numpy as np
import pytest


@pytest.mark.parametrize('threads', [1, 3])
def test_lca_problem_equals_synth(threads):
    import bench
    from woltka_amd import synth
    scale = 0.002
    got = bench.lca_problem(7, scale, threads=threads)
    want = synth.as_sets(synth.lca_problem(
        np.random.default_rng(7), n_nodes=2_000_000, n_subjects=100_000,
        n_reads=int(50_000_000 * scale), with_names=False))
    assert got.keys() == want.keys()
    for key in ('subj', 'qoff', 'subjects'):
        assert got[key].dtype == want[key].dtype, key
        assert np.array_equal(got[key], want[key]), key
    assert got['n_ids'] == want['n_ids']
    for key in ('parent', 'last', 'rank_code'):
        assert np.array_equal(getattr(got['hier'], key),
                              getattr(want['hier'], key)), key


def _key(job, k, group, feature):
    from woltka_amd import _native as nat
    return (job << 61) | (k << (nat.KEY_FEATURE_BITS + nat.KEY_GROUP_BITS)) | \
        (group << nat.KEY_FEATURE_BITS) | feature


def test_dump_outputs_one_pass(tmp_path):
    import bench
    from woltka_amd import _native as nat
    L = nat.WEIGHT_L
    # one pass: job 0 feature 5 = 1 + 1/3 (two cells), feature 2 = 1/2 in
    # units of 1 / L; job 1 feature 9 = 4; job 2: nothing
    cells = [((0, 1, 0, 5), 1), ((0, 3, 0, 5), 1), ((0, 0, 0, 2), L // 2),
             ((1, 1, 0, 9), 4)]
    keys = np.array([_key(*c) for c, _ in cells], dtype=np.uint64)
    vals = np.array([n for _, n in cells], dtype=np.int64)
    for passes in (1, 7):
        ctx = types.SimpleNamespace(
            counts_fetch=lambda: (keys[::-1].copy(), vals[::-1] * passes))
        wl = types.SimpleNamespace(ctx=ctx, passes_run=passes,
                                   ranks=('phylum', 'genus', 'species'),
                                   jobs=[None] * 3)
        out = tmp_path / str(passes)
        bench.dump_outputs(wl, str(out))
        p = np.load(out / 'phylum.npy')
        assert p.dtype == np.float64
        assert p.tolist() == [[0.0, 2.0, 0.5], [0.0, 5.0, 1 + 1 / 3]]
        assert np.load(out / 'genus.npy').tolist() == [[0.0, 9.0, 4.0]]
        assert np.load(out / 'species.npy').shape == (0, 3)
    wl.passes_run = 2
    with pytest.raises(RuntimeError, match='equal passes'):
        bench.dump_outputs(wl, str(tmp_path / 'x'))
