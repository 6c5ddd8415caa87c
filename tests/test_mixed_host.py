"""Mixed rank sets on the packed-record route, host half: which job sets
`Engine.words_eligible(mixed=...)` takes, and that the committed fixture has
exactly the cases of tests/mixed_cases.py.  No device work."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _engine_class():
    from woltka_amd.routes.words import WordsRoute

    class E(WordsRoute):
        _replay = None
        _tok_identity = True
        use_tree = True
        sizes = None
    return E


def _engine(*jobs, **attrs):
    """A stub engine over jobs given as (mode, flags, major)."""
    from woltka_amd import _native as nat
    e = _engine_class()()
    e.jobs = [nat.Job(m, 0, f, 0, major) for m, f, major in jobs]
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


@pytest.fixture
def clean_env(monkeypatch):
    for name in ('WOLTKA_NO_MIXED', 'WOLTKA_NO_WORDS', 'WOLTKA_NO_DSIZES'):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_mixed_gate(clean_env):
    """Mixed unsized sets are taken only with ``mixed=True``; every refusal of
    the two kinds stays one; WOLTKA_NO_MIXED is honoured."""
    from woltka_amd import _native as nat
    none = (nat.MODE_NONE, 0, 0.0)
    rank = (nat.MODE_RANK, 0, 0.0)
    wholes = [(nat.MODE_FREE, 0, 0.0), (nat.MODE_RANK, nat.F_UNIQ, 0.0),
              (nat.MODE_RANK, nat.F_ABOVE, 0.0), (nat.MODE_RANK, 0, 0.8),
              (nat.MODE_FREE, nat.F_UNASSIGNED | nat.F_SUBOK, 0.0)]
    for whole in wholes:
        for jobs in ((none, whole), (whole, rank, none), (none, whole, rank, rank),
                     (none, whole, wholes[0])):
            assert not _engine(*jobs).words_eligible()
            assert not _engine(*jobs).words_eligible(identity=False)
            assert _engine(*jobs).words_eligible(mixed=True) is True
            assert _engine(*jobs).words_eligible(identity=False, mixed=True)
            assert _engine(*jobs).words_mixed()
            # no tree, ids that are no subject indices, a replay, `--sizes`
            assert not _engine(*jobs, use_tree=False).words_eligible(mixed=True)
            assert not _engine(*jobs, _tok_identity=False).words_eligible(mixed=True)
            assert not _engine(*jobs, _replay=object()).words_eligible(mixed=True)
            assert not _engine(*jobs, sizes={'a': 1}).words_eligible(mixed=True)
    free = wholes[0]
    refused = [
        ((nat.MODE_NONE, nat.F_SIZED, 0.0), free),           # a sized job,
        (none, (nat.MODE_FREE, nat.F_SIZED, 0.0)),           # of either kind
        ((nat.MODE_RANK, nat.F_SIZED, 0.0), free, none),
        ((nat.MODE_NONE, nat.F_UNIQ, 0.0), free),            # `none` under --uniq
        (none, free, (nat.MODE_RANK, 0, 0.5)),               # 0 < major <= 0.5
        (free, (nat.MODE_RANK, 0, 0.3)),
        (none, free, (nat.MODE_RANK, nat.F_UNASSIGNED, 0.01)),
        (none, free, (7, 0, 0.0)),                           # no mode of either kind
        (none, free) * 4 + (rank,),                          # more than MAX_JOBS
    ]
    assert len(refused[-1]) == nat.MAX_JOBS + 1
    for jobs in refused:
        assert not _engine(*jobs).words_eligible(mixed=True), jobs
        assert not _engine(*jobs, sizes={'a': 1}).words_eligible(
            sized=True, mixed=True), jobs
    # exactly MAX_JOBS jobs are taken
    assert _engine(*((none, free) * 4)).words_eligible(mixed=True)
    clean_env.setenv('WOLTKA_NO_MIXED', '1')
    assert not _engine(none, free).words_eligible(mixed=True)
    assert not _engine(free, rank, none).words_eligible(identity=False, mixed=True)
    # (the sets of one kind do not care)
    assert _engine(none, rank).words_eligible(mixed=True)
    assert _engine(free, wholes[1]).words_eligible(mixed=True)
    clean_env.delenv('WOLTKA_NO_MIXED')
    clean_env.setenv('WOLTKA_NO_WORDS', '1')
    assert not _engine(none, free).words_eligible(mixed=True)


def test_default_argument_keeps_todays_answers(clean_env):
    """The sets of tests/test_sizes_host.py::test_gates, and the unsized sets of
    one kind: the same answer with and without ``mixed=True`` unless the set
    is mixed, and the default never takes a mixed set."""
    from woltka_amd import _native as nat
    S = nat.F_SIZED
    sized = {'a': 1}
    plain = _engine((nat.MODE_NONE, S, 0.0), (nat.MODE_RANK, S, 0.0), sizes=sized)
    assert not plain.words_eligible()
    assert plain.words_eligible(sized=True)
    assert plain.words_eligible(identity=False, sized=True)
    assert plain.words_eligible(sized=True, mixed=True)
    for m, f, major in ((nat.MODE_FREE, 0, 0.0), (nat.MODE_RANK, nat.F_UNIQ, 0.0),
                        (nat.MODE_RANK, nat.F_ABOVE, 0.0), (nat.MODE_RANK, 0, 0.8),
                        (nat.MODE_NONE, nat.F_UNIQ, 0.0)):
        whole = (m, f | S, major)
        for mixed in (False, True):
            assert not _engine(whole, sizes=sized).words_eligible(
                sized=True, mixed=mixed)
            assert not _engine((nat.MODE_NONE, S, 0.0), whole, sizes=sized
                               ).words_eligible(sized=True, mixed=mixed)
    none, rank, free = (nat.MODE_NONE, 0, 0.0), (nat.MODE_RANK, 0, 0.0), \
        (nat.MODE_FREE, 0, 0.0)
    for jobs, want in (((none,), True), ((none, rank, rank), True),
                       ((free,), True), ((free, (nat.MODE_RANK, 0, 0.8)), True),
                       (((nat.MODE_RANK, 0, 0.5),), False),
                       (((nat.MODE_NONE, nat.F_UNIQ, 0.0),), False),
                       ((none, free), False)):
        assert bool(_engine(*jobs).words_eligible()) is want, jobs
        if not _engine(*jobs).words_mixed():
            assert bool(_engine(*jobs).words_eligible(mixed=True)) is want, jobs
    # without a tree the plain sets are still taken, the whole-read ones not
    assert _engine(none, use_tree=False).words_eligible(mixed=True)
    assert not _engine(free, use_tree=False).words_eligible(mixed=True)


def test_begin_helper_picks_the_entry(clean_env):
    """`_words_begin`: the mixed entry for a mixed set, and only for it."""
    from woltka_amd import _native as nat
    from woltka_amd.hostio import ROUTES
    calls = []

    class Ctx:
        def words_begin(self, jobs, group, mixed=False):
            calls.append((len(jobs), group, mixed))
            return True
    none, rank, free = (nat.MODE_NONE, 0, 0.0), (nat.MODE_RANK, 0, 0.0), \
        (nat.MODE_FREE, 0, 0.0)
    before = ROUTES['mixed']
    for jobs, want in (((none, free), True), ((none, rank), False),
                       ((free,), False), ((free, rank, none), True)):
        e = _engine(*jobs, ctx=Ctx())
        assert e._words_begin(3)
        assert calls[-1] == (len(jobs), 3, want)
        e._count_mixed()
    assert ROUTES['mixed'] == before + 2
    clean_env.setenv('WOLTKA_NO_MIXED', '1')
    e = _engine(none, free, ctx=Ctx())
    e._words_begin(0)
    e._count_mixed()
    assert calls[-1] == (2, 0, False) and ROUTES['mixed'] == before + 2


def test_fixture_has_the_cases():
    import mixed_cases
    with open(os.path.join(HERE, 'golden', 'vectors', 'mixed_device.json')) as f:
        gold = json.load(f)
    cases = mixed_cases.cases()
    assert sorted(gold) == sorted(c['name'] for c in cases)
    assert sorted(gold) == sorted([
        'sop8', 'free-first', 'two-whole', 'major', 'unassigned-subok',
        'blocks', 'b6o', 'paf', 'map', 'gz', 'trimsub', 'lineage', 'no-class',
        'stranger', 'wide-read', 'uniq'])
    for case in cases:
        assert len(gold[case['name']]) == len(case['calls'])
        for call, res in zip(case['calls'], gold[case['name']]):
            assert call['route'] in ('device', 'both', 'host', 'as-plain')
            assert set(res) in ({'tables'}, {'error'})
            if 'tables' in res:
                ranks = call['kwargs']['ranks'].split(',')
                assert sorted(res['tables']) == sorted(f'{r}.tsv' for r in ranks)
    assert len(mixed_cases.full()) == 103
