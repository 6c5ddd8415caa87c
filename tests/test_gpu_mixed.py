"""Mixed rank sets on the packed-record route (wk_words_begin_mixed, mode 4 of
wk_words_*): whole-read jobs (`--rank free`, a rank under --uniq / --above /
--major above one half) next to plain ones (`--rank none`, a plain rank) — the
call the reference's documentation recommends, `--rank none,free,phylum,...`.
The sample's records are kept once, in read order; the flush counts every
whole-read job with the per-read stream (csrc/wk_free.hpp) and the plain jobs
with the weighted histogram (csrc/wk_weigh.hpp), each under its index in the
set.  Held against the general evaluator (wk_chunk_stage + wk_classify_staged),
the C oracle, and — through `workflow` — the reference's own tables
(tests/golden/vectors/mixed_device.json)."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

from helpers import assert_same_counts, load_vectors, oracle_table

import mixed_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANKS = ('phylum', 'genus', 'species')      # rank slots 0, 1, 2


def _words(sidx, off):
    """subject | position in the read << 23 | read size << 27"""
    size = np.diff(off)
    pos = np.arange(sidx.size) - np.repeat(off[:-1], size)
    return (sidx.astype(np.uint32) | (pos.astype(np.uint32) << np.uint32(23)) |
            (np.repeat(size, size).astype(np.uint32) << np.uint32(27)))


def _problem(seed, n_nodes, n_subjects, n_reads, offtree_frac=0.0):
    """The reads, and the subject table in two forms: every subject of the
    problem (``subjects``), the records as indices into it (``sidx``)."""
    from woltka_amd import synth
    rng = np.random.default_rng(seed)
    p = synth.as_sets(synth.lca_problem(
        rng, n_nodes=n_nodes, n_subjects=n_subjects, n_reads=n_reads,
        with_names=False, offtree_frac=offtree_frac))
    p['off'] = p['qoff'].astype(np.int64)
    assert int(np.diff(p['off']).max()) <= 16
    return p


def _context(nat, h, table=1 << 18):
    c = nat.Context(0)
    c.set_tree(h.parent, h.last, h.rank_code)
    for slot, rank in enumerate(RANKS):
        c.build_rank_table(slot, h.rank_codes[rank])
    c.counts_reserve(table)
    return c


def _specs(nat, jobs, h):
    codes = [h.rank_codes[r] for r in RANKS]
    return [(j.mode, codes[j.rank_slot] if j.mode == nat.MODE_RANK else 0,
             j.flags, j.major) for j in jobs]


def _general(nat, c, jobs, sidx, qoff, group):
    c.chunk_stage(sidx.astype(np.int32), qoff, group=group, subj_is_set=True,
                  indexed=True)
    c.classify_staged(jobs)


def _is_plain(nat, job):
    return job.mode == nat.MODE_NONE or (
        job.mode == nat.MODE_RANK and job.major <= 0 and
        not job.flags & (nat.F_UNIQ | nat.F_ABOVE))


@pytest.fixture(scope='module')
def small():
    """30 000 nodes, 2 000 subjects, 200 000 reads, every subject in the tree
    (and, as the generator makes them, below a node of every rank)."""
    p = _problem(21, 30000, 2000, 200_000)
    # (subject indices in the order of first appearance, as a tokenizer hands
    # them out: the table grows while the file is read)
    u, first, inv = np.unique(p['subj'], return_index=True, return_inverse=True)
    order = np.argsort(first)
    place = np.empty(u.size, np.int64)
    place[order] = np.arange(u.size)
    p['feats'], p['sidx'] = u[order].astype(np.int32), place[inv]
    assert np.array_equal(p['feats'][p['sidx']], p['subj'])
    p['words'] = _words(p['sidx'], p['off'])
    return p


def _mixed_sets(nat):
    none = nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)
    free = nat.Job(nat.MODE_FREE, 0, 0, 0, 0.0)
    phylum = nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)
    genus = nat.Job(nat.MODE_RANK, 1, 0, 0, 0.0)
    return [
        [none, free],
        [free, genus, none],
        [none, free, phylum, genus],
        [none, nat.Job(nat.MODE_RANK, 1, nat.F_ABOVE, 0, 0.0), free],
        [none, nat.Job(nat.MODE_RANK, 1, 0, 0, 0.8)],
    ]


@pytest.mark.parametrize('which', range(5))
def test_mixed_sets_are_taken(ctx, small, which):
    """wk_words_begin refuses the set, wk_words_begin_mixed takes it; the
    subject table grows between the two halves; the table equals the general
    evaluator's and the oracle's bit for bit, under the job indices of the
    set; reads and records are counted once; a begin under another group
    flushes the first."""
    from woltka_amd import _native as nat
    p = small
    h, off, words, feats, sidx = p['hier'], p['off'], p['words'], p['feats'], p['sidx']
    n_reads = off.size - 1
    half = n_reads // 2
    jobs = _mixed_sets(nat)[which]
    with _context(nat, h) as c:
        # (the first 2 000 reads name about two thirds of the subjects, the
        # first half all of them: the table grows under accumulated records)
        at = 0
        for upto in (2000, half, n_reads):
            seen = int(sidx[:int(off[upto])].max()) + 1
            assert (seen < feats.size) == (upto == 2000)
            c.set_subjects(feats[:seen])
            assert not at or c.words_pending() == (int(off[at]), at)
            if not at:
                assert not c.words_begin(jobs, 4)
            assert c.words_begin(jobs, 4, mixed=True)
            c.words_append(words[int(off[at]):int(off[upto])], upto - at)
            at = upto
        assert c.words_pending() == (words.size, n_reads)
        a = nat.canonical_counts(*c.counts_fetch())
        st = c.stats()
        assert st['n_reads'] == n_reads and st['n_records'] == words.size
        job, k, grp, feat = nat.decode_keys(a[0])
        assert (grp == 4).all()
        assert sorted(np.unique(job).tolist()) == list(range(len(jobs)))
        for j, jb in enumerate(jobs):   # every read adds L in all to a plain job
            if _is_plain(nat, jb):
                assert int(a[1][job == j].sum()) == n_reads * nat.WEIGHT_L, j
        c.counts_clear()
        c.reset_stats()
        _general(nat, c, jobs, sidx, p['qoff'], 4)
        b = nat.canonical_counts(*c.counts_fetch())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert_same_counts(*a, *oracle_table(p['subj'], p['qoff'],
                                             _specs(nat, jobs, h), h, group=4))
        # a second group behind the first, all at once this time
        cut = 3000
        c.counts_clear()
        c.reset_stats()
        assert c.words_begin(jobs, 4, mixed=True)
        c.words_append(words, n_reads)
        assert c.words_begin(jobs, 5, mixed=True)
        assert c.words_pending() == (0, 0)
        st = c.stats()
        assert st['n_reads'] == n_reads and st['n_records'] == words.size
        c.words_append(words[:int(off[cut])], cut)
        a2 = nat.canonical_counts(*c.counts_fetch())
        c.counts_clear()
        _general(nat, c, jobs, sidx, p['qoff'], 4)
        _general(nat, c, jobs, sidx[:int(off[cut])], p['qoff'][:cut + 1], 5)
        b2 = nat.canonical_counts(*c.counts_fetch())
        assert np.array_equal(a2[0], b2[0]) and np.array_equal(a2[1], b2[1])
        assert set(nat.decode_keys(a2[0])[2].tolist()) == {4, 5}


@pytest.mark.parametrize('wide', [0, 1])
def test_mixed_over_more_than_one_slice(ctx, wide):
    """41 000 subjects: one slice of the histogram holds 40 608.  The team
    layout over the one unsliced stream, and the wide layout
    (csrc/wk_weigh_wide.hpp), both reading the records in read order."""
    from woltka_amd import _native as nat
    p = _problem(22, 120_000, 41_000, 150_000)
    h, off = p['hier'], p['off']
    subjects = np.asarray(p['subjects'], dtype=np.int32)
    assert subjects.size == 41_000
    sidx = np.searchsorted(subjects, p['subj'])
    assert np.array_equal(subjects[sidx], p['subj'])
    assert int(sidx.max()) >= 40_608        # (records in the second slice)
    words = _words(sidx, off)
    jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0),
            nat.Job(nat.MODE_FREE, 0, 0, 0, 0.0),
            nat.Job(nat.MODE_RANK, 1, 0, 0, 0.0)]
    with _context(nat, h, 1 << 20) as c:
        c.tune('weigh_wide', wide)
        c.profile_kernels(True)
        c.set_subjects(subjects)
        assert c.words_begin(jobs, 1, mixed=True)
        c.words_append(words, off.size - 1)
        a = nat.canonical_counts(*c.counts_fetch())
        if wide:
            assert c.last_kernel_ms('weigh_wide') > 0
        assert c.last_kernel_ms('weigh_merge') > 0
        c.counts_clear()
        _general(nat, c, jobs, sidx, p['qoff'], 1)
        b = nat.canonical_counts(*c.counts_fetch())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        job = nat.decode_keys(a[0])[0]
        for j in (0, 2):
            assert int(a[1][job == j].sum()) == (off.size - 1) * nat.WEIGHT_L


def test_mixed_refusals(ctx, small):
    """Every refusal of wk_words_begin is one of the mixed entry; all-plain and
    all-whole-read sets give through it what they give through
    wk_words_begin; subjects outside the tree are taken by `none,free` and
    refused — after what is there has been flushed — next to a plain rank."""
    from woltka_amd import _native as nat
    p = small
    h, off, words, feats, sidx = p['hier'], p['off'], p['words'], p['feats'], p['sidx']
    n_reads = off.size - 1
    none = nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)
    free = nat.Job(nat.MODE_FREE, 0, 0, 0, 0.0)
    genus = nat.Job(nat.MODE_RANK, 1, 0, 0, 0.0)
    with _context(nat, h) as c:
        c.set_subjects(feats)
        for bad in ([nat.Job(nat.MODE_NONE, 0, nat.F_SIZED, 0, 0.0), free],
                    [none, nat.Job(nat.MODE_FREE, 0, nat.F_SIZED, 0, 0.0)],
                    [nat.Job(nat.MODE_NONE, 0, nat.F_UNIQ, 0, 0.0), free],
                    [none, free, nat.Job(nat.MODE_RANK, 1, 0, 0, 0.5)],
                    [free, nat.Job(nat.MODE_RANK, 1, 0, 0, 0.3)],
                    [nat.Job(nat.MODE_RANK, 1, 0, 0, 0.5)],
                    [nat.Job(nat.MODE_RANK, 1, nat.F_UNIQ | nat.F_SIZED, 0, 0.0)]):
            assert not c.words_begin(bad, 0, mixed=True), bad
        with pytest.raises(ValueError):         # more than WK_MAX_JOBS jobs
            c.words_begin([none, free] * 4 + [genus], 0, mixed=True)
        # the sets of one kind: the same tables through either entry
        for jobs in ([none, genus, nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)],
                     [free, nat.Job(nat.MODE_RANK, 1, nat.F_UNIQ, 0, 0.0)],
                     [free], [nat.Job(nat.MODE_RANK, 2, 0, 0, 0.8)]):
            got = []
            for mixed in (False, True):
                c.counts_clear()
                assert c.words_begin(jobs, 2, mixed=mixed)
                c.words_append(words, n_reads)
                got.append(nat.canonical_counts(*c.counts_fetch()))
            assert np.array_equal(got[0][0], got[1][0])
            assert np.array_equal(got[0][1], got[1][1])
            assert got[0][0].size > 3
    with nat.Context(0) as c:                   # no tree
        c.set_subjects(feats)
        c.counts_reserve(1 << 16)
        assert not c.words_begin([none, free], 0, mixed=True)
    # subjects outside the tree (1 % of the records)
    q = _problem(25, 30000, 2000, 60_000, offtree_frac=0.01)
    h, off = q['hier'], q['off']
    feats, sidx = np.unique(q['subj'], return_inverse=True)
    feats = feats.astype(np.int32)
    n_in = int(np.searchsorted(feats, h.n_nodes))
    assert 0 < n_in < feats.size
    words = _words(sidx, off)
    n_reads = off.size - 1
    with _context(nat, h) as c:
        c.set_subjects(feats)
        jobs = [none, free]
        assert c.words_begin(jobs, 3, mixed=True)
        c.words_append(words, n_reads)
        a = nat.canonical_counts(*c.counts_fetch())
        assert_same_counts(*a, *oracle_table(q['subj'], q['qoff'],
                                             _specs(nat, jobs, h), h, group=3))
        # a stranger is its own result under --subok: not for the stream
        assert not c.words_begin(
            [none, nat.Job(nat.MODE_FREE, 0, nat.F_SUBOK, 0, 0.0)], 3,
            mixed=True)
        # the reads before the first stranger, then the strangers join the table
        first = int(np.flatnonzero(sidx >= n_in)[0])
        lead = int(np.searchsorted(off, first, side='right')) - 1
        assert lead > 10 and int(sidx[:int(off[lead])].max()) < n_in
        jobs = [none, free, genus]
        c.counts_clear()
        c.reset_stats()
        c.set_subjects(feats[:n_in])
        assert c.words_begin(jobs, 3, mixed=True)
        c.words_append(words[:int(off[lead])], lead)
        c.set_subjects(feats)
        assert not c.words_begin(jobs, 3, mixed=True)
        assert c.words_pending() == (0, 0)
        with pytest.raises(RuntimeError):
            c.words_append(words[:10], 1)
        a = nat.canonical_counts(*c.counts_fetch())
        st = c.stats()
        assert st['n_reads'] == lead and st['n_records'] == int(off[lead])
        c.counts_clear()
        _general(nat, c, jobs, sidx[:int(off[lead])], q['qoff'][:lead + 1], 3)
        b = nat.canonical_counts(*c.counts_fetch())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[0].size >= 3


# ---- through `workflow`: the reference's tables ------------------------------

def _routes():
    from woltka_amd.hostio import ROUTES
    return dict(ROUTES)


def _delta(before):
    after = _routes()
    return {k: after.get(k, 0) - before.get(k, 0)
            for k in ('mixed', 'dtok', 'host_block', 'text_ahead')}


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run_call(call, root, log=None):
    """One `workflow` call of a case: its result as run_case gives it, and the
    routes its blocks took."""
    from woltka_amd import classify, workflow
    from sizes_cases import run_case
    os.makedirs(root, exist_ok=True)
    before = _routes()
    env = dict(WOLTKA_NO_MIXED=None)
    env.update(call.get('env', {}))
    block = classify.Engine.DTOK_BLOCK
    with _env(**env), contextlib.ExitStack() as stack:
        classify.Engine.DTOK_BLOCK = call.get('block', block)
        stack.callback(setattr, classify.Engine, 'DTOK_BLOCK', block)
        if log is None:
            got = run_case(workflow.workflow, call, root)
        else:
            from sizes_cases import write_case
            args = write_case(call, root)
            args['output_fp'] = os.path.join(root, 'out')
            with contextlib.redirect_stdout(log):
                workflow.workflow(**args)
            got = {'tables': {
                fn: open(os.path.join(root, 'out', fn)).read()
                for fn in sorted(os.listdir(os.path.join(root, 'out')))}}
    return got, _delta(before)


CALLS = [(case['name'], i) for case in mixed_cases.cases()
         for i in range(len(case['calls']))]


@pytest.mark.parametrize('name,i', CALLS, ids=[f'{n}-{i}' for n, i in CALLS])
def test_mixed_cli_cases(tmp_path, name, i):
    """The reference's tables (or error) byte for byte, and the route the
    case promises."""
    want = load_vectors('mixed_device.json')[name][i]
    case = next(c for c in mixed_cases.cases() if c['name'] == name)
    call = case['calls'][i]
    got, d = _run_call(call, str(tmp_path / 'run'))
    assert got == want
    route = call['route']
    if route == 'as-plain':
        # what the plain ranks of the set take on this hierarchy today
        plain = dict(call, kwargs=dict(call['kwargs'], ranks=call['plain_ranks']))
        _, dp = _run_call(plain, str(tmp_path / 'plain'))
        assert (d['dtok'] > 0) == (dp['dtok'] > 0)
        assert (d['host_block'] > 0) == (dp['host_block'] > 0)
        assert (d['mixed'] > 0) == (dp['dtok'] > 0)
    elif route == 'device':
        assert d['mixed'] > 0 and d['dtok'] > 0 and d['host_block'] == 0, d
    elif route == 'both':
        assert d['mixed'] > 0 and d['host_block'] > 0, d
    else:
        assert route == 'host' and d['mixed'] == 0, d


@pytest.mark.parametrize('name', ['sop8', 'blocks'])
@pytest.mark.parametrize('dtok', [True, False])
def test_mixed_equals_old_route(tmp_path, name, dtok):
    """The same call with and without WOLTKA_NO_MIXED=1 — through the device
    tokenizer, and with the host tokenizer's words (`_run_words`) — writes the
    same tables and the same log."""
    case = next(c for c in mixed_cases.cases() if c['name'] == name)
    call = case['calls'][0]
    res = []
    for tag, no_mixed in (('new', None), ('old', '1')):
        log = io.StringIO()
        with _env(WOLTKA_NO_DTOK=None if dtok else '1'):
            call_ = dict(call, env=dict(call.get('env', {}),
                                        WOLTKA_NO_MIXED=no_mixed))
            got, d = _run_call(call_, str(tmp_path / tag), log=log)
        assert (d['mixed'] > 0) == (no_mixed is None), (tag, d)
        assert 'Number of sequences classified' in log.getvalue()
        # (the log names the input directory)
        res.append((got, log.getvalue().replace(str(tmp_path / tag), '.')))
    assert res[0] == res[1]
    assert res[0][0] == load_vectors('mixed_device.json')[name][0]


def test_mixed_keeps_the_reader_started_ahead(tmp_path, monkeypatch):
    """`sop8` with the reader started before the hierarchy (routes.device_text
    TEXT_AHEAD_MIN patched to 0): a mixed set keeps it."""
    from woltka_amd.routes import device_text
    monkeypatch.setattr(device_text, 'TEXT_AHEAD_MIN', 0)
    case = next(c for c in mixed_cases.cases() if c['name'] == 'sop8')
    got, d = _run_call(case['calls'][0], str(tmp_path / 'run'))
    assert got == load_vectors('mixed_device.json')['sop8'][0]
    assert d['text_ahead'] == 1 and d['mixed'] > 0
