"""The cases of tests/cli_routes_cases.py without a GPU: the generated inputs
are the ones the reference saw, every admissible pair of option levels stands
in a case, every file has the size and the runs promised, the caps on errors
and on cases without a device route hold, every ROUTES key has its cases --
and `expected_route`, the table of DESIGN.md section 3 as data, says what the
gates of `classify.py`, `routes/words.py` and `workflow.classify` say for
every case (`gates_route`: the gates called as `workflow.classify` calls
them, on a stand-in for the engine)."""
import hashlib

import pytest

import cli_routes_cases as T
from helpers import load_vectors

CASES = T.cases()
GOLD = load_vectors('cli_routes.json')


@pytest.fixture(scope='module')
def files():
    """{case name: (`case_files`)}: made once."""
    return {c['name']: T.case_files(c) for c in CASES}


def test_inputs_are_the_recorded_ones(files):
    assert sorted(GOLD) == sorted(c['name'] for c in CASES)
    for case in CASES:
        got = {k: hashlib.sha256(v).hexdigest()
               for k, v in files[case['name']][0].items()}
        assert got == GOLD[case['name']]['inputs'], T.label(case)


def test_every_admissible_pair_is_covered():
    want = T.all_pairs()
    # (recomputed here from the factors and the constraints alone)
    bad = {frozenset((a, b)) for a, b, _ in T.CONSTRAINTS}
    n = 0
    for i, f in enumerate(T.NAMES):
        for g in T.NAMES[i + 1:]:
            for x in T.FACTORS[f]:
                for y in T.FACTORS[g]:
                    if frozenset(((f, x), (g, y))) in bad:
                        assert ((f, x), (g, y)) not in want
                        continue
                    n += 1
                    assert any(c[f] == x and c[g] == y for c in CASES), \
                        (f, x, g, y)
    assert n == len(want)
    for case in CASES:
        assert T.admissible({f: case[f] for f in T.NAMES}), T.label(case)
    for a, b, reason in T.CONSTRAINTS:
        assert a[1] in T.FACTORS[a[0]] and b[1] in T.FACTORS[b[0]] and reason


def test_files_have_the_size_and_the_runs(files):
    for case in CASES:
        _, texts, _ = files[case['name']]
        assert len(texts) == (1 if case['input'] in T.DEMUX else 3)
        for fp, text in texts.items():
            assert len(text) >= 3 * T.BLOCK, (T.label(case), fp, len(text))
            assert T.run_share(text) >= T.MIN_RUN_SHARE, (T.label(case), fp)
        if case['stratify']:
            strata = [k for k in files[case['name']][0]
                      if k.startswith('strata/')]
            assert len(strata) == 3, T.label(case)


def test_caps():
    errors = [c for c in CASES if 'error' in GOLD[c['name']]]
    assert len(errors) <= 0.10 * len(CASES), list(map(T.label, errors))
    nowhere = [c for c in CASES if T.expected_route(c) is None]
    assert len(nowhere) <= 0.40 * len(CASES), len(nowhere)
    for key in T.ROUTE_KEYS:
        have = [c for c in CASES if T.expected_route(c) is not None and
                key in T.expected_route(c) | T.expected_also(c)]
        many = [c for c in have if c['blocks'] == 'many']
        assert len(have) >= 6, (key, len(have))
        assert len(many) >= 2, (key, len(many))
        assert any(c['zip'] == '.gz' for c in have), key


def test_table_keys_are_routes_keys():
    keys = {k for row, _ in T.TABLE for k in row.split('+')}
    assert keys == set(T.ROUTE_KEYS)
    for _, cond in T.TABLE:
        for f, levels in cond.items():
            assert set(levels) <= set(T.FACTORS[f]), (f, levels)


# ---- the gates --------------------------------------------------------------
def _engine(kw):
    """The smallest stand-in for `classify.Engine` the gates can be asked
    on: the jobs of the command as `Engine.__init__` numbers them."""
    from woltka_amd import _native as nat
    from woltka_amd.routes.words import WordsRoute

    class E(WordsRoute):
        pass
    flags = 0
    if kw.get('uniq'):
        flags |= nat.F_UNIQ
    if kw.get('above'):
        flags |= nat.F_ABOVE
    if kw.get('unassigned'):
        flags |= nat.F_UNASSIGNED
    if kw.get('sizes'):
        flags |= nat.F_SIZED
    e = E()
    e.jobs = []
    for rank in kw['ranks'].split(','):
        if rank == 'none':
            e.jobs.append(nat.Job(nat.MODE_NONE, 0, flags, 0, 0.0))
        elif rank == 'free':
            e.jobs.append(nat.Job(nat.MODE_FREE, 0, flags, 0, 0.0))
        else:
            e.jobs.append(nat.Job(nat.MODE_RANK, 0, flags, 0,
                                  (kw.get('major') or 0) / 100))
    e.sizes = {'x': 1} if kw.get('sizes') else None
    e._replay = None
    e.use_tree = True
    e._tok_identity = True
    return e


def gates_route(case, kw):
    """What `workflow.classify` and `Engine.native_chunks` decide for a file
    of the case, every gate called with the case's options: the ROUTES keys
    that count its blocks (one of them: a key that stands for a family),
    or None -- the host tokenizer."""
    from woltka_amd import classify as C
    fmt = case['fmt']
    ordinal = bool(kw.get('coords_fp'))
    demux = bool(kw.get('demux'))
    strata = bool(kw.get('strata_dir'))
    outmap, cover = case['outmap'], case['outcov']
    exclude, trimsub = bool(kw.get('exclude')), bool(kw.get('trimsub'))
    sizes = bool(kw.get('sizes'))
    own_text = case['zip'] in ('', '.gz')
    e = _engine(kw)
    n_jobs = len(e.jobs)
    # workflow.classify
    native = not (fmt == 'map' and (ordinal or cover))
    if not native:
        return None
    native_strata = strata and not demux
    native_demux = demux and not strata and not outmap and not cover
    want_names = bool((demux and not native_demux) or outmap or
                      (strata and not native_strata))
    dreads = native_strata and C.strata_reads_on_device(
        fmt, strata=True, demux=demux, coords=ordinal, sizes=sizes,
        outmap=outmap, outcov=cover, part=None, n_jobs=n_jobs, replay=False,
        own_text=own_text)
    dstrata = bool(native_strata and ordinal and fmt in ('sam', 'b6o', 'paf')
                   and not exclude and not cover and not outmap and own_text)
    on_device_map = dstrata or dreads       # (`load_strata(device=...)`)
    want_strings = bool((demux and not native_demux) or
                        (strata and not native_strata) or
                        (ordinal and outmap))
    plain = not (ordinal or cover or want_names or native_strata or demux or
                 outmap)
    sized = e.sized_on_device(plain, None)
    words = plain and not trimsub and e.words_eligible(sized=sized,
                                                       mixed=True)
    words_dev = plain and (trimsub or exclude) and e.words_eligible(
        identity=False, sized=sized, mixed=True)
    dcover = cover and not ordinal and C.cover_on_device(
        fmt, exclude=exclude, demux=demux, strata=strata, outmap=outmap,
        part=None, n_jobs_ok=e.words_eligible(identity=not trimsub),
        n_subjects=0)
    dmaps = outmap and not (ordinal or cover or demux or strata or trimsub
                            or want_strings) and e.device_maps_eligible()
    dreadmaps = outmap and not dmaps and not want_strings and \
        e.read_maps_on_device(fmt, demux=demux, strata=strata,
                              coords=ordinal, outcov=cover, part=None,
                              own_text=own_text)
    ddemux = C.demux_on_device(native_demux, fmt, coords=ordinal,
                               sizes=sizes, n_jobs=n_jobs, replay=False)
    dhdemux = ordinal and C.demux_hits_on_device(
        native_demux, fmt, sizes=sizes, exclude=exclude, n_jobs=n_jobs,
        replay=False)
    # Engine.native_chunks
    want_groups, want_samples = native_strata, native_demux
    dhdemux = bool(dhdemux and want_samples and ordinal and not cover and
                   not want_names and not want_groups and not exclude)
    device_ex = bool(ordinal and not cover and not want_names and
                     (not want_groups or on_device_map) and
                     (not want_samples or dhdemux))
    dcover = bool(dcover and cover and not ordinal)
    ddemux = bool(ddemux and want_samples and not ordinal and not cover)
    dreads = bool(dreads and want_groups and on_device_map and not ordinal
                  and not cover and not want_names and not want_samples)
    dreadmaps = bool(dreadmaps and not (words or words_dev or dmaps) and
                     not ordinal and not cover and not want_groups and
                     not want_samples)
    if not ((words or words_dev or device_ex or dmaps or dcover or ddemux
             or dreads or dreadmaps) and
            (fmt in ('sam', 'b6o', 'paf') or not ordinal) and
            (not exclude or ((words or words_dev or ddemux or dreads or
                              dreadmaps) and not dmaps)) and own_text):
        return None
    # Engine._device_chunks: who takes the blocks
    if device_ex:
        return {'dhits_demux'} if dhdemux else \
            {'dhits_strata'} if want_groups else {'dhits'}
    if ddemux:
        return {'ddemux'}
    if dreads:
        return {'dreads_strata'}
    if dreadmaps:
        return {'dreads_maps'}
    if dcover:
        return {'dcover'}
    if dmaps and not words:
        return {'dtok_maps'}
    return {'dtok'}


def test_every_gate_is_what_its_docstring_says(files):
    """Each gate alone, asked with the case's options whether or not
    `workflow.classify` would ask it: `cli_routes_cases.GATES`."""
    from woltka_amd import classify as C
    wrong = []
    for case in CASES:
        kw = T.kwargs_of(case, files[case['name']][2])
        e = _engine(kw)
        fmt, n_jobs = case['fmt'], len(e.jobs)
        ordinal = case['system'] in T.COORDS
        demux, strata = case['input'] in T.DEMUX, case['stratify']
        own_text = case['zip'] in ('', '.gz')
        native_demux = demux and not strata and not case['outmap'] and \
            not case['outcov']
        got = {
            'cover_on_device': C.cover_on_device(
                fmt, exclude=case['exclude'], demux=demux, strata=strata,
                outmap=case['outmap'], part=None,
                n_jobs_ok=e.words_eligible(identity=not case['trimsub']),
                n_subjects=0),
            'demux_on_device': C.demux_on_device(
                native_demux, fmt, coords=ordinal, sizes=case['sizes'],
                n_jobs=n_jobs, replay=False),
            'demux_hits_on_device': C.demux_hits_on_device(
                native_demux, fmt, sizes=case['sizes'],
                exclude=case['exclude'], n_jobs=n_jobs, replay=False),
            'strata_reads_on_device': C.strata_reads_on_device(
                fmt, strata=strata, demux=demux, coords=ordinal,
                sizes=case['sizes'], outmap=case['outmap'],
                outcov=case['outcov'], part=None, n_jobs=n_jobs,
                replay=False, own_text=own_text),
            'read_maps_on_device': e.read_maps_on_device(
                fmt, demux=demux, strata=strata, coords=ordinal,
                outcov=case['outcov'], part=None, own_text=own_text),
            'device_maps_eligible': e.device_maps_eligible(),
            'words_eligible': not case['sizes'] and
            e.words_eligible(mixed=True),
            'sized_words': bool(case['sizes']) and
            e.words_eligible(sized=True, mixed=True),
        }
        assert set(got) == set(T.GATES)
        for gate, said in got.items():
            if bool(said) != T.gate_says(gate, case):
                wrong.append((gate, T.label(case), bool(said)))
    assert not wrong, wrong
    # every gate says yes and says no somewhere, and each of its conditions
    # is the only one that fails in some case
    for gate, cond in T.GATES.items():
        assert any(T.gate_says(gate, c) for c in CASES), gate
        for f in cond:
            assert any(T.isolates(c, cond, f) for c in CASES), (gate, f)


def test_expected_route_is_what_the_gates_say(files):
    wrong = []
    for case in CASES:
        kw = T.kwargs_of(case, files[case['name']][2])
        want, got = T.expected_route(case), gates_route(case, kw)
        if want != got:
            wrong.append((T.label(case), want, got))
        also = T.expected_also(case)
        e = _engine(kw)
        assert ('mixed' in also) == bool(want == {'dtok'} and e._mixed_on()),\
            T.label(case)
        assert ('sized_flush' in also) == bool(want == {'dtok'} and e.sizes),\
            T.label(case)
    assert not wrong, wrong
