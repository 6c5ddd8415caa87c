"""Cases of tests/golden/vectors/cli_routes.json: the options of `woltka
classify` met two at a time over every device route, on inputs of several
tokenizer blocks.  Everything is rebuilt from `SEED` -- by
tests/golden/make_cli_routes_reference.py (which runs the reference on the
cases), by tests/test_cli_routes_host.py and by tests/test_gpu_cli_routes.py;
only what the reference made of the cases is committed.  This module imports
neither the package nor the reference.

Factors and levels: `FACTORS`.  No level is dropped; what the reference cannot
run, or what has no meaning, is a pair of `CONSTRAINTS` (each with its
reason).  Where a level needs files the bundled data has only for one system,
the level keeps its meaning and changes its files:

* under `--coords` the features are genes, so the ranks are those of the
  bundled gene -> UniRef -> GO process maps (`uniref`, `process`) and
  `--sizes` is `.` (the genes' lengths from the coordinates); with
  `--trim-sub _` the genes become their genomes again and the ranks and
  sizes are the taxonomy's, as in plain classification;
* plain `--trim-sub` puts `_1` / `_2` behind the subjects in the text.

Selection (`cases()`): for every ROUTES key of `TABLE` six cases are seeded
with the options that lead to it (two of them with 8192-byte blocks, one of
these two `.gz`), their other factors filled by the greedy pairwise step; then
the greedy step goes on until every admissible pair of levels of two factors
stands in a case; then, per row of the table and per option the row names,
a neighbour: a case that meets the row but for that option (`_neighbours`).

Input text (`case_files`): the text of every alignment file (before
compression) is `MIN_BYTES` at least, made
of batches of `make_golden._random_alignment` (plain) or of reads placed over
and next to genes as `make_golden.gen_cli_coords` places them (`--coords`);
runs of 1-6 lines per query; every batch brings a subject the file has not
met yet.  A multiplexed file changes its sample with every
batch, so samples are met late and again.

Expected route (`expected_route`): the table of DESIGN.md section 3 as data.
It does not call the gates; tests/test_cli_routes_host.py holds it against
them."""
import gzip
import hashlib
import lzma
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
DATA = os.path.join(GOLDEN, 'data')
TAX = os.path.join(DATA, 'taxonomy')
FUN = os.path.join(DATA, 'function')

SEED = 20261
BLOCK = 1 << 13             # Engine.DTOK_BLOCK of the many-blocks cases
MIN_BYTES = 3 * BLOCK + 512     # of every alignment file
MIN_RUN_SHARE = 0.30        # of the lines: in runs of two or more equal QNAMEs
VERBATIM = 512              # longer read maps / coverage files: `digest`
GENES = 6                   # genes of a genome that reads are placed over
EXT = {'sam': 'sam', 'b6o': 'b6', 'paf': 'paf', 'map': 'map'}

FACTORS = {
    'fmt': ('sam', 'b6o', 'paf', 'map'),
    # a directory of 3 files / with samples='S2,S1' / one multiplexed file
    # (demux=True) / the same with a whitelist file
    'input': ('dir', 'dir-samples', 'mux', 'mux-list'),
    'zip': ('', '.gz', '.bz2'),
    # plain classification / --coords / --coords with a random overlap
    # threshold and chunk size
    'system': ('plain', 'coords', 'coords-th'),
    'jobs': ('none', 'one', 'three', 'whole', 'none-uniq', 'mixed'),
    'outmap': (False, True),
    'outcov': (False, True),
    'stratify': (False, True),
    'sizes': (False, True),
    'trimsub': (False, True),
    'exclude': (False, True),
    'unassigned': (False, True),
    'name_as_id': (False, True),
    'blocks': ('one', 'many'),
}
NAMES = tuple(FACTORS)

CONSTRAINTS = (
    (('fmt', 'map'), ('system', 'coords'),
     'a simple map has no coordinates to match genes with'),
    (('fmt', 'map'), ('system', 'coords-th'),
     'a simple map has no coordinates to match genes with'),
    (('fmt', 'map'), ('outcov', True),
     'a simple map has no ranges to cover subjects with'),
    (('system', 'coords'), ('outcov', True),
     'coverage is of subjects; the coord-match yields genes and no ranges '
     '(the reference fails inside parse_ranges, this package says so)'),
    (('system', 'coords-th'), ('outcov', True),
     'coverage is of subjects; the coord-match yields genes and no ranges '
     '(the reference fails inside parse_ranges, this package says so)'),
)

# ---- the table of DESIGN.md section 3, as data ------------------------------
# (key, what must hold: factor -> admitted levels) -- the first row whose
# conditions all hold names the route; 'words' / 'whole-only' / 'plain-only'
# are the job sets of `JOB_KINDS`.  A file must be text the package reads block
# by block: plain or `.gz`, never `.bz2` (`BLOCKWISE`).
BLOCKWISE = ('', '.gz')
COORDS = ('coords', 'coords-th')
DEMUX = ('mux', 'mux-list')
DIR = ('dir', 'dir-samples')
TEXT3 = ('sam', 'b6o', 'paf')

JOB_KINDS = {
    # the jobs of the weighted histogram: none, <rank>
    'plain-only': ('none', 'one', 'three'),
    # no job can return a list: free, a rank under --uniq / --above /
    # --major, none under --uniq
    'no-list': ('whole', 'none-uniq'),
    # what `Engine.words_eligible` takes: plain jobs, whole-read jobs, ...
    'words': ('none', 'one', 'three', 'whole'),
    # ... and both kinds in one set where the caller declares it
    'words-mixed': ('none', 'one', 'three', 'whole', 'mixed'),
}

TABLE = (
    # R2d: --coords under --demux, with or without --sizes / --trim-sub
    ('dhits_demux', {'system': COORDS, 'input': DEMUX, 'fmt': TEXT3,
                     'exclude': (False,), 'stratify': (False,),
                     'outmap': (False,), 'outcov': (False,)}),
    # R2 with a strata map: the join runs on the device too
    ('dhits_strata', {'system': COORDS, 'input': DIR, 'fmt': TEXT3,
                      'stratify': (True,), 'exclude': (False,),
                      'outmap': (False,), 'outcov': (False,)}),
    # R2: --coords, with or without --sizes / --trim-sub
    ('dhits', {'system': COORDS, 'input': DIR, 'fmt': TEXT3,
               'stratify': (False,), 'exclude': (False,),
               'outmap': (False,), 'outcov': (False,)}),
    # R1d
    ('ddemux', {'system': ('plain',), 'input': DEMUX, 'stratify': (False,),
                'outmap': (False,), 'outcov': (False,), 'sizes': (False,)}),
    # R1t
    ('dreads_strata', {'system': ('plain',), 'input': DIR,
                       'stratify': (True,), 'sizes': (False,),
                       'outmap': (False,), 'outcov': (False,)}),
    # R1c (R1s is "not with --outcov": no `--sizes` here)
    ('dcover', {'system': ('plain',), 'input': DIR, 'outcov': (True,),
                'fmt': TEXT3, 'exclude': (False,), 'stratify': (False,),
                'outmap': (False,), 'jobs': JOB_KINDS['words'],
                'sizes': (False,)}),
    # R1 with read maps of plain jobs
    ('dtok_maps', {'system': ('plain',), 'input': DIR, 'outmap': (True,),
                   'jobs': JOB_KINDS['plain-only'], 'trimsub': (False,),
                   'exclude': (False,), 'stratify': (False,),
                   'outcov': (False,), 'sizes': (False,)}),
    # R1m
    ('dreads_maps', {'system': ('plain',), 'input': DIR, 'outmap': (True,),
                     'jobs': JOB_KINDS['no-list'], 'stratify': (False,),
                     'outcov': (False,), 'sizes': (False,)}),
    # R1s
    ('dtok+sized_flush', {'system': ('plain',), 'input': DIR,
                          'sizes': (True,), 'jobs': JOB_KINDS['plain-only'],
                          'outmap': (False,), 'outcov': (False,),
                          'stratify': (False,)}),
    # R1, a mixed set
    ('dtok+mixed', {'system': ('plain',), 'input': DIR, 'jobs': ('mixed',),
                    'sizes': (False,), 'outmap': (False,),
                    'outcov': (False,), 'stratify': (False,)}),
    # R1
    ('dtok', {'system': ('plain',), 'input': DIR,
              'jobs': JOB_KINDS['words'], 'sizes': (False,),
              'outmap': (False,), 'outcov': (False,), 'stratify': (False,)}),
)
ROUTE_KEYS = ('dtok', 'dtok_maps', 'dreads_maps', 'dcover', 'ddemux', 'dhits',
              'dhits_strata', 'dhits_demux', 'dreads_strata', 'mixed',
              'sized_flush')
# (the keys that count blocks of the device text route: 'mixed' and
# 'sized_flush' count on the host tokenizer's packed words too)
BLOCK_KEYS = ROUTE_KEYS[:-2]


def _row_of(case):
    if case['zip'] not in BLOCKWISE:
        return None
    for key, cond in TABLE:
        if all(case[f] in levels for f, levels in cond.items()):
            return key
    return None


def expected_route(case):
    """The ROUTES keys of which one must count for the case (its factor
    levels), or None: no device text route.  The key that counts the blocks."""
    row = _row_of(case)
    return None if row is None else {row.split('+')[0]}


def expected_also(case):
    """The ROUTES keys that must count next to `expected_route`'s: 'mixed'
    for a mixed set, 'sized_flush' for `--sizes` on the packed records."""
    row = _row_of(case)
    return set((row or '').split('+')[1:])


# ---- the gates' docstrings, as data -----------------------------------------
# gate -> what must hold of the case for the gate to say yes when it is asked
# with the case's options (factor -> admitted levels); `NATIVE_DEMUX` is what
# `workflow.classify` hands over as ``native_demux``.  The table above is
# what these make together with `Engine.native_chunks`; a gate is also held
# to its own line here, because `native_chunks` checks some conditions once
# more and would hide a gate that has lost one.
NATIVE_DEMUX = {'input': DEMUX, 'stratify': (False,), 'outmap': (False,),
                'outcov': (False,)}
GATES = {
    'cover_on_device': {
        'fmt': TEXT3, 'exclude': (False,), 'input': DIR, 'stratify': (False,),
        'outmap': (False,), 'jobs': JOB_KINDS['words'], 'sizes': (False,)},
    'demux_on_device': dict(NATIVE_DEMUX, system=('plain',), sizes=(False,)),
    'demux_hits_on_device': dict(NATIVE_DEMUX, fmt=TEXT3, exclude=(False,)),
    'strata_reads_on_device': {
        'stratify': (True,), 'input': DIR, 'system': ('plain',),
        'sizes': (False,), 'outmap': (False,), 'outcov': (False,),
        'zip': BLOCKWISE},
    'read_maps_on_device': {
        'input': DIR, 'stratify': (False,), 'system': ('plain',),
        'outcov': (False,), 'sizes': (False,), 'zip': BLOCKWISE,
        'jobs': JOB_KINDS['no-list']},
    'device_maps_eligible': {
        'sizes': (False,), 'jobs': JOB_KINDS['plain-only']},
    # (`words_eligible(mixed=True)`, without `--sizes`; with: `sized_words`)
    'words_eligible': {'sizes': (False,), 'jobs': JOB_KINDS['words-mixed']},
    'sized_words': {'sizes': (True,), 'jobs': JOB_KINDS['plain-only']},
}


def isolates(case, cond, f):
    """Does the case meet ``cond`` but for the factor ``f``?"""
    return case[f] not in cond[f] and all(
        case[g] in lv for g, lv in cond.items() if g != f)


def gate_says(gate, case):
    """Must ``gate`` say yes for the case, by its docstring?"""
    return all(case[f] in levels for f, levels in GATES[gate].items())


def n_files(case):
    """Alignment files the command reads (`samples='S2,S1'` leaves S3
    out)."""
    return {'dir': 3, 'dir-samples': 2}.get(case['input'], 1)


# ---- pairwise selection -----------------------------------------------------
def _forbidden():
    out = set()
    for a, b, _ in CONSTRAINTS:
        out.add((a, b))
        out.add((b, a))
    return out


def admissible(case):
    """Does the (partial) case hold no pair of `CONSTRAINTS`?"""
    bad = _forbidden()
    items = list(case.items())
    return not any((items[i], items[j]) in bad
                   for i in range(len(items))
                   for j in range(i + 1, len(items)))


def all_pairs():
    """Every admissible pair of levels of two different factors:
    {((factor, level), (factor, level))}, the factors in `NAMES`' order."""
    bad = _forbidden()
    out = set()
    for i, f in enumerate(NAMES):
        for g in NAMES[i + 1:]:
            for x in FACTORS[f]:
                for y in FACTORS[g]:
                    if ((f, x), (g, y)) not in bad:
                        out.add(((f, x), (g, y)))
    return out


def pairs_of(case):
    return {((f, case[f]), (g, case[g]))
            for i, f in enumerate(NAMES) for g in NAMES[i + 1:]}


def _fill(fixed, todo, rng):
    """One case: ``fixed`` (factor -> level) and, factor by factor in a
    random order, the level that covers most pairs of ``todo`` with what
    stands already (ties: at random)."""
    case = dict(fixed)
    order = [f for f in NAMES if f not in case]
    rng.shuffle(order)
    for f in order:
        best, best_n = [], -1
        for x in FACTORS[f]:
            trial = dict(case)
            trial[f] = x
            if not admissible(trial):
                continue
            n = sum(((min((f, x), (g, y), key=lambda p: NAMES.index(p[0])),
                      max((f, x), (g, y), key=lambda p: NAMES.index(p[0])))
                     in todo) for g, y in case.items())
            if n > best_n:
                best, best_n = [x], n
            elif n == best_n:
                best.append(x)
        case[f] = rng.choice(best)
    return {f: case[f] for f in NAMES}


def _seeds():
    """Per ROUTES key of the table six partial cases that lead to it: the
    row's conditions where they leave no choice, two of the six with
    8192-byte blocks, one of these `.gz`."""
    rng = random.Random(SEED)
    out = []
    for key in ROUTE_KEYS:
        rows = [(k, c) for k, c in TABLE if key in k.split('+')]
        for i in range(6):
            _, cond = rows[i % len(rows)]
            fixed = {f: rng.choice(levels) for f, levels in cond.items()}
            fixed['zip'] = '.gz' if i == 0 else rng.choice(BLOCKWISE)
            fixed['blocks'] = 'many' if i < 2 else 'one'
            out.append((key, fixed))
    return out


def _neighbours():
    """Per row of the table and per option it names (the system and the
    kind of input apart): a partial case that meets the row but for that one
    option -- where a gate that has lost a condition shows.  Plain or `.gz`
    text, so that nothing but the option decides."""
    rng = random.Random(SEED + 2)
    out = []
    for _, cond in TABLE:
        for f, levels in cond.items():
            others = [x for x in FACTORS[f] if x not in levels]
            if f in ('system', 'input') or not others:
                continue
            fixed = {g: rng.choice(lv) for g, lv in cond.items()}
            fixed[f] = rng.choice(others)
            fixed['zip'] = rng.choice(BLOCKWISE)
            if admissible(fixed):
                out.append(fixed)
    return out


_CASES = None


def cases():
    """[{'name', 'seed', every factor}]: the seeded cases of every route,
    greedy cases until all pairs are covered, then the routes' neighbours."""
    global _CASES
    if _CASES is not None:
        return [dict(c) for c in _CASES]
    rng = random.Random(SEED + 1)
    todo = all_pairs()
    out = []

    def add(case):
        # (a row above the seeded one may claim the case: try again)
        case = dict(case, seed=SEED + 100 + len(out))
        case['name'] = f'{len(out):03d}'
        out.append(case)
        todo.difference_update(pairs_of(case))

    for key, fixed in _seeds():
        for _ in range(50):
            case = _fill(fixed, todo, rng)
            got = (_row_of(case) or '').split('+')
            if key in got:
                break
        else:
            raise AssertionError(f'no case for {key}: {fixed}')
        add(case)
    while todo:
        first = min(todo, key=repr)      # (any order, but always the same one)
        best = None
        for _ in range(12):
            case = _fill(dict(first), todo, rng)
            n = len(pairs_of(case) & todo)
            if best is None or n > best[0]:
                best = (n, case)
        add(best[1])
    for fixed in _neighbours():
        add(_fill(fixed, todo, rng))
    # ... and the gates' own neighbours, where no case is one yet
    nrng = random.Random(SEED + 3)
    for gate, cond in GATES.items():
        for f in cond:
            if any(isolates(c, cond, f) for c in out):
                continue
            fixed = {g: nrng.choice(lv) for g, lv in cond.items()}
            fixed[f] = nrng.choice([x for x in FACTORS[f]
                                    if x not in cond[f]])
            fixed.setdefault('zip', nrng.choice(BLOCKWISE))
            assert admissible(fixed), (gate, f)
            add(_fill(fixed, todo, rng))
    _CASES = out
    return [dict(c) for c in out]


def label(case):
    """The case's factor levels, for ids and failure messages."""
    bits = [case['name'], case['fmt'] + case['zip'], case['input'],
            case['system'], case['jobs']]
    bits += [f for f in ('outmap', 'outcov', 'stratify', 'sizes', 'trimsub',
                         'exclude', 'unassigned', 'name_as_id') if case[f]]
    bits.append(case['blocks'])
    return '-'.join(bits)


# ---- input text -------------------------------------------------------------
def _make_golden():
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden
    return make_golden


_GENOMES, _GENES = None, None


def genomes():
    """The genomes of the bundled `taxid.map` that have an ancestor at each
    of phylum, genus and species, in file order (a subject without one makes
    the weighted histogram hand its block to the host: another test's
    business, tests/mixed_cases.py)."""
    global _GENOMES
    if _GENOMES is None:
        from sizes_cases import RANKS3, genome_ranks
        _GENOMES = [g for g, have in genome_ranks().items()
                    if set(RANKS3) <= have]
    return _GENOMES


def genes():
    """{genome: [(begin, end)]} of the bundled coordinates."""
    global _GENES
    if _GENES is None:
        _GENES = {}
        with lzma.open(os.path.join(FUN, 'coords.txt.xz'), 'rt') as f:
            for line in f:
                if line.startswith('>'):
                    cur = _GENES.setdefault(line[1:].strip(), [])
                else:
                    x = line.split('\t')
                    a, b = int(x[1]), int(x[2])
                    cur.append((min(a, b), max(a, b)))
    return _GENES


def _placed_alignment(rng, fmt, subjects, n_queries, prefix):
    """Reads placed over / next to the first `GENES` genes of ``subjects``
    (so the tables stay small), as `make_golden.gen_cli_coords` places
    them: 1-3 hits per query."""
    G = genes()
    lines = []
    for qi in range(n_queries):
        q = f'{prefix}r{qi:04d}'
        paired = fmt == 'sam' and rng.random() < 0.5
        for _ in range(rng.choice([1, 1, 2, 3])):
            s = rng.choice(subjects)
            gs, ge = rng.choice(G[s][:GENES])
            ln = rng.choice([75, 100, 150])
            pos = max(1, gs + rng.randint(-ln, ge - gs))
            if fmt == 'sam':
                flag = rng.choice([99, 147]) if paired else \
                    rng.choice([0, 16, 256])
                cig = rng.choice([f'{ln}M', f'{ln - 10}M2D10M',
                                  f'5S{ln - 5}M'])
                lines.append(f'{q}\t{flag}\t{s}\t{pos}\t255\t{cig}\t='
                             f'\t0\t0\t*\t*\n')
            elif fmt == 'b6o':
                a, b = pos, pos + ln - 1
                if rng.random() < 0.5:
                    a, b = b, a
                lines.append(f'{q}\t{s}\t99.0\t{ln}\t0\t0\t1\t{ln}\t'
                             f'{a}\t{b}\t1e-9\t200\n')
            else:
                lines.append(f'{q}\t{ln}\t0\t{ln}\t+\t{s}\t9999999\t'
                             f'{pos - 1}\t{pos - 1 + ln}\t{ln}\t{ln}\t60\n')
    return ''.join(lines)


def _alignment(rng, case, subjects, samples, suffix):
    """Text of one alignment file of MIN_BYTES at least: batches of 60
    queries, every batch under the next of ``samples`` (read ids
    `<sample>_...`; [None]: no prefix) and with one more of ``subjects``
    than the batch before, so that subjects are met late."""
    fmt = case['fmt']
    coords = case['system'] in COORDS
    mg = _make_golden()
    parts, size, k = [], 0, 0
    if fmt == 'sam':
        parts.append('@HD\tVN:1.0\tSO:unsorted\n')
    while size < MIN_BYTES:
        smp = samples[k % len(samples)]
        prefix = (f'{smp}_' if smp else '') + f'k{k}'
        if coords:
            body = _placed_alignment(rng, fmt, subjects[:2 + k], 60, prefix)
        else:
            body = mg._random_alignment(rng, fmt, subjects[:4 + k], 60,
                                        prefix, suffix)
            if fmt == 'sam':            # (its header line: once per file)
                body = body.split('\n', 1)[1]
        parts.append(body)
        size += len(body)
        k += 1
    return ''.join(parts)


def read_ids(text, fmt):
    """The query ids of the text's lines as the reference's parsers name
    them (SAM: `/1`, `/2` by the flag; unmapped records have none)."""
    out = []
    for line in text.split('\n'):
        if not line or line[0] in '@#':
            continue
        x = line.split('\t')
        q = x[0]
        if fmt == 'sam':
            flag = int(x[1])
            if flag & 4:
                continue
            q += '/1' if flag & 64 else '/2' if flag & 128 else ''
        out.append(q)
    return out


def run_share(text):
    """Share of the alignment lines that stand in a run of two or more
    equal QNAMEs."""
    names = [x.split('\t', 1)[0] for x in text.split('\n')
             if x and x[0] not in '@#']
    n, i = 0, 0
    while i < len(names):
        j = i
        while j < len(names) and names[j] == names[i]:
            j += 1
        if j - i > 1:
            n += j - i
        i = j
    return n / len(names)


def _zipped(text, ext):
    import bz2
    data = text.encode()
    if ext == '.gz':
        return gzip.compress(data, mtime=0)
    if ext == '.bz2':
        return bz2.compress(data)
    return data


def case_files(case):
    """({relative path: bytes}, {alignment path: its text}, details) of the
    case: alignment files under `aln/` (or `mux.<ext>`), the whitelist
    `ids.txt`, the strata maps under `strata/`; details = what `kwargs_of`
    needs of the draw (excluded subjects, overlap, chunk, the whole-read
    flavour, the strata maps' compression)."""
    rng = random.Random(case['seed'])
    fmt, coords = case['fmt'], case['system'] in COORDS
    if coords:
        G = genes()
        pool = [g for g in G if len(G[g]) > 50]
        subjects = rng.sample(pool, rng.randint(3, 4))
    else:
        subjects = rng.sample(genomes(), rng.randint(8, 12))
    suffix = rng.choice(['_1', '_2']) if case['trimsub'] and not coords else ''
    det = {
        'exclude': [x + suffix for x in rng.sample(subjects[:3],
                                                   1 if coords else 2)],
        'overlap': rng.choice([50, 80, 100]),
        'chunk': rng.choice([50, None]),
        'whole': rng.choice(['free', 'uniq', 'above', 'major']),
        'strata_zip': rng.choice(['', '.gz']),
    }
    texts = {}
    if case['input'] in DEMUX:
        name = f'mux.{EXT[fmt]}{case["zip"]}'
        texts[name] = _alignment(rng, case, subjects, ['A', 'B', 'C'], suffix)
        samples = ['A', 'B', 'C']
    else:
        for smp in ('S1', 'S2', 'S3'):
            texts[f'aln/{smp}.{EXT[fmt]}{case["zip"]}'] = _alignment(
                rng, case, subjects, [None], suffix)
        samples = ['S1', 'S2', 'S3']
    files = {k: _zipped(v, case['zip']) for k, v in texts.items()}
    if case['input'] == 'mux-list':
        files['ids.txt'] = b'A\nC\n'
    if case['stratify']:
        # per sample: read -> stratum for about 80 % of its reads
        for smp in samples:
            rows = []
            for fp, text in texts.items():
                for q in dict.fromkeys(read_ids(text, fmt)):
                    if case['input'] in DEMUX:
                        left, _, q = q.partition('_')
                        if left != smp:
                            continue
                    elif not fp.startswith(f'aln/{smp}.'):
                        continue
                    if rng.random() < 0.8:
                        rows.append(f'{q}\t{rng.choice("XY")}\n')
            files[f'strata/{smp}.txt{det["strata_zip"]}'] = _zipped(
                ''.join(rows), det['strata_zip'])
    return files, texts, det


def kwargs_of(case, det):
    """The keyword arguments of `workflow.workflow` but for the output paths;
    `$TAX/`, `$FUN/` and the case's own relative paths are for `real`."""
    coords = case['system'] in COORDS
    kw = {'output_fmt': False, 'input_fmt': case['fmt']}
    if case['input'] in DEMUX:
        kw['input_fp'] = f'mux.{EXT[case["fmt"]]}{case["zip"]}'
        kw['demux'] = True
        if case['input'] == 'mux-list':
            kw['samples'] = 'ids.txt'
    else:
        kw['input_fp'] = 'aln'
        if case['input'] == 'dir-samples':
            kw['samples'] = 'S2,S1'
    taxonomy = not coords or case['trimsub']
    if taxonomy:
        kw.update(nodes_fps=['$TAX/nodes.dmp'], map_fps=['$TAX/taxid.map'],
                  names_fps=['$TAX/names.dmp'])
        one, three = 'genus', 'phylum,genus,species'
    else:
        kw.update(map_fps=['$FUN/uniref/uniref.map.xz',
                           '$FUN/go/process.tsv.xz'],
                  map_rank=None, names_fps=['$FUN/go/name.txt.xz'])
        one, three = 'process', 'none,uniref,process'
    jobs = case['jobs']
    if jobs == 'none':
        kw['ranks'] = 'none'
    elif jobs == 'one':
        kw['ranks'] = one
    elif jobs == 'three':
        kw['ranks'] = three
    elif jobs == 'none-uniq':
        kw.update(ranks='none', uniq=True)
    elif jobs == 'mixed':
        kw['ranks'] = f'none,free,{one}'
    elif det['whole'] == 'free':
        kw['ranks'] = 'free'
    else:
        kw['ranks'] = one
        kw.update({'uniq': dict(uniq=True), 'above': dict(above=True),
                   'major': dict(major=60)}[det['whole']])
    if coords:
        kw['coords_fp'] = '$FUN/coords.txt.xz'
        if case['system'] == 'coords-th':
            kw['overlap'] = det['overlap']
            if det['chunk']:
                kw['chunk'] = det['chunk']
    if case['sizes']:
        kw['sizes'] = '$TAX/length.map' if taxonomy else '.'
        kw['scale'] = '1M'
    if case['trimsub']:
        kw['trimsub'] = '_'
    if case['exclude']:
        kw['exclude'] = ','.join(det['exclude'])
    if case['unassigned']:
        kw['unassigned'] = True
    if case['name_as_id']:
        kw['name_as_id'] = True
    if case['stratify']:
        kw['strata_dir'] = 'strata'
    return kw


def digest(data):
    return {'sha256': hashlib.sha256(data).hexdigest(), 'bytes': len(data),
            'lines': data.count(b'\n')}


def kept(data):
    """A read map / coverage file in the fixture: its text, or above
    `VERBATIM` bytes its `digest`."""
    return data.decode() if len(data) <= VERBATIM else digest(data)


def run_case(workflow, case, root):
    """Write the case under ``root`` and run ``workflow`` on it:
    {'inputs': {path: sha256}, and 'tables' / 'maps' / 'cov' (name ->
    `kept`) or 'error': [type name, message]}."""
    import contextlib
    import io
    files, _, det = case_files(case)
    for rel, data in files.items():
        fp = os.path.join(root, rel)
        os.makedirs(os.path.dirname(fp), exist_ok=True)
        with open(fp, 'wb') as f:
            f.write(data)

    def real(v):
        if isinstance(v, list):
            return [real(x) for x in v]
        if isinstance(v, str) and v.startswith('$TAX/'):
            return os.path.join(TAX, v[5:])
        if isinstance(v, str) and v.startswith('$FUN/'):
            return os.path.join(FUN, v[5:])
        if isinstance(v, str) and (v in files or v in ('aln', 'strata')):
            return os.path.join(root, v)
        return v
    args = {k: real(v) for k, v in kwargs_of(case, det).items()}
    out = args['output_fp'] = os.path.join(root, 'out')
    maps = cov = None
    if case['outmap']:
        maps = args['outmap_dir'] = os.path.join(root, 'maps')
    if case['outcov']:
        cov = args['outcov_dir'] = os.path.join(root, 'cov')
    res = {'inputs': {k: hashlib.sha256(v).hexdigest()
                      for k, v in sorted(files.items())}}
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            workflow(**args)
    except Exception as e:      # noqa: a combination the reference refuses
        res['error'] = [type(e).__name__, str(e)]
        return res
    if os.path.isdir(out):
        res['tables'] = {fn: open(os.path.join(out, fn), newline='').read()
                         for fn in sorted(os.listdir(out))}
    else:
        with open(out, newline='') as f:
            res['tables'] = {'out': f.read()}
    if maps:
        res['maps'] = {}
        for dirpath, _, fns in os.walk(maps):
            for fn in fns:
                fp = os.path.join(dirpath, fn)
                assert fn.endswith('.txt.gz'), fn
                with gzip.open(fp, 'rb') as f:
                    rel = os.path.relpath(fp, maps)[:-3]
                    res['maps'][rel] = kept(f.read())
    if cov:
        res['cov'] = {}
        for fn in sorted(os.listdir(cov) if os.path.isdir(cov) else []):
            with open(os.path.join(cov, fn), 'rb') as f:
                res['cov'][fn] = kept(f.read())
    return res
