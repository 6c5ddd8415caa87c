"""Plain classification with `--stratify` on the device text route
(csrc/wk_strata_reads.hpp: strata_place_reads_kernel behind the plain
flavour's scan) through its own door -- `Context.dtok_stage_reads_strata`,
`chunk_groups` -- and through whole commands.

Per read: the label of every probe of the maps of tests/strata_cases.py
against tests/golden/vectors/strata_device.json (the join is blind to the
flavour of the scan: what the reference says of a read id stands there), and
the placement of blocks of every shape against a model written here.
Commands: the cases of tests/strata_plain_cases.py against
tests/golden/vectors/strata_plain_device.json
(tests/golden/make_strata_plain_reference.py), with the route each takes.
tests/test_strata_plain_host.py pins the same fixture without a device."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import strata_cases as T                # noqa: E402
import strata_plain_cases as P          # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD_MAPS = load_vectors('strata_device.json')
GOLD = load_vectors('strata_plain_device.json')
MAPS = T.map_cases()
KEPT = list(T.kept_maps())
CASES = {c['name']: c for c in P.cases()}
TILE = 256                  # lines of a workgroup of the placement (kDtokThreads)


class Device:
    """One context and one tokenizer for the whole module: every block is
    scanned over the one before, every map loaded over the one before."""

    def __init__(self):
        from woltka_amd import _native as nat
        self.nat = nat
        self.ctx = nat.Context(0)
        self.tok = nat.Tokenizer(2)
        self.ctx.counts_reserve(1 << 18)
        self.ctx.dtok_format('sam')
        self.subjects = []      # names of the tokenizer's subjects
        self.jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0)]

    def load(self, text):
        """The map's labels (as str) with label i in group i, or None."""
        got = self.ctx.strata_load(np.frombuffer(text, dtype=np.uint8))
        if got is None:
            return None
        labels, slots = got
        self.ctx.strata_groups(slots, np.arange(len(labels), dtype=np.int32))
        return [x.decode() for x in labels]

    def stage(self, text, n_lines):
        """One block of SAM lines scanned for the plain flavour and staged.
        Returns (qoff, subjects' names per record, groups)."""
        ctx = self.ctx
        text = np.frombuffer(text, dtype=np.uint8)
        status, got_lines = ctx.dtok_scan(self.tok, text, 0, text.size)
        assert status == 0 and got_lines == n_lines
        self.subjects.extend(self.tok.new_subjects())
        status, n_reads, n_records = ctx.dtok_stage_reads_strata()
        assert status == 0
        subj, qoff = ctx.chunk_download()
        assert qoff.size == n_reads + 1 and subj.size == n_records
        group = ctx.chunk_groups(n_reads)
        assert group.size == n_reads
        return qoff, subj, group

    def cells(self):
        """{(group, subject name): Fraction} of the staged chunk under
        `--rank none`."""
        ctx = self.ctx
        ctx.set_subjects(np.arange(len(self.subjects), dtype=np.int32))
        ctx.counts_clear()
        ctx.classify_staged(self.jobs)
        keys, vals = ctx.counts_fetch()
        cells = self.nat.counts_to_fractions(keys, vals)
        assert all(j == 0 for j, _, _ in cells)
        return {(g, self.subjects[f]): v for (_, g, f), v in cells.items()}

    def close(self):
        self.tok.close()
        self.ctx.close()


@pytest.fixture(scope='module')
def dev():
    d = Device()
    yield d
    d.close()


# ---- a. the join, per read --------------------------------------------------------
@pytest.mark.parametrize('name', KEPT)
def test_every_read_gets_the_reference_label(dev, name):
    labels = dev.load(MAPS[name])
    assert labels == T.gold_map(GOLD_MAPS, name)[1]
    plist = T.case_probes(name, MAPS[name])
    want_map, _ = T.gold_map(GOLD_MAPS, name)
    want = [want_map.get(T.probe_key(p)) for p in plist]
    qoff, subj, group = dev.stage(T.probe_sam(plist), len(plist))
    # (a line per probe, a subject per line: the reads are the probes, in
    # order but for the mates of a pair, which are one run -- /1 before /2)
    assert qoff.tolist() == list(range(len(plist) + 1))
    assert [int(dev.subjects[s][1:]) for s in subj.tolist()] == \
        list(range(len(plist)))
    got = [labels[g] if g >= 0 else None for g in group.tolist()]
    assert got == want
    assert sum(g < 0 for g in group.tolist()) == \
        sum(T.probe_key(p) not in want_map for p in plist)
    assert all(-1 <= g < max(len(labels), 1) for g in group.tolist())


def test_a_smaller_map_over_a_larger_one(dev):
    big = T.case_probes('labels-65536', MAPS['labels-65536'])[:200]
    want_map, _ = T.gold_map(GOLD_MAPS, 'labels-65536')
    labels = dev.load(MAPS['labels-65536'])
    _, _, group = dev.stage(T.probe_sam(big), len(big))
    got = [labels[g] if g >= 0 else None for g in group.tolist()]
    assert got == [want_map.get(T.probe_key(p)) for p in big]
    assert 40 < sum(g >= 0 for g in group.tolist()) < 160
    # the keys of the first map are gone, its label slots carry no group
    labels = dev.load(MAPS['clean'])
    _, _, group = dev.stage(T.probe_sam(big), len(big))
    assert group.tolist() == [-1] * len(big)
    plist = T.case_probes('clean', MAPS['clean'])
    want_map, _ = T.gold_map(GOLD_MAPS, 'clean')
    _, _, group = dev.stage(T.probe_sam(plist), len(plist))
    assert [labels[g] if g >= 0 else None for g in group.tolist()] == \
        [want_map.get(T.probe_key(p)) for p in plist]


def test_the_stage_wants_a_map_with_groups_and_no_demultiplexing(dev):
    ctx = dev.ctx
    text = np.frombuffer(T.probe_sam([('a', 0)]), dtype=np.uint8)
    ctx.strata_clear()
    assert ctx.dtok_scan(dev.tok, text, 0, text.size) == (0, 1)
    dev.subjects.extend(dev.tok.new_subjects())
    with pytest.raises(RuntimeError, match='no strata map with groups'):
        ctx.dtok_stage_reads_strata()
    got = ctx.strata_load(np.frombuffer(MAPS['clean'], dtype=np.uint8))
    with pytest.raises(RuntimeError, match='no strata map with groups'):
        ctx.dtok_stage_reads_strata()
    ctx.strata_groups(got[1], np.arange(len(got[0]), dtype=np.int32))
    ctx.demux_begin(True)
    try:
        with pytest.raises(RuntimeError, match='wk_demux_begin'):
            ctx.dtok_stage_reads_strata()
    finally:
        ctx.demux_begin(False)
    assert ctx.dtok_stage_reads_strata() == (0, 1, 1)
    assert ctx.chunk_groups(1).tolist() == [-1]
    # (the block has been staged: there is none left)
    with pytest.raises(RuntimeError, match='no block scanned'):
        ctx.dtok_stage_reads_strata()


# ---- b. the placement ---------------------------------------------------------------
LABELS = ['L0', 'L1', 'L2', 'L3', 'L4']
POOL = [f'Q{i:03d}' for i in range(64)]


def _model(lines, held):
    """What the parser makes of ``lines`` [(QNAME, mate, subject)]: runs of
    equal QNAMEs, in a run one read per mate in the order 0, /1, /2, a read's
    subjects each once in the order of their first lines.  Returns [(group or
    -1, subjects)] with ``held`` {read id: label}."""
    reads, i = [], 0
    while i < len(lines):
        j = i
        while j < len(lines) and lines[j][0] == lines[i][0]:
            j += 1
        for mate in (0, 1, 2):
            subs = list(dict.fromkeys(s for _, m, s in lines[i:j]
                                      if m == mate))
            if subs:
                label = held.get(T.probe_key((lines[i][0], mate)))
                reads.append((LABELS.index(label) if label else -1, subs))
        i = j
    return reads


def _sam(lines):
    return ''.join(f'{q}\t{T.FLAG[m]}\t{s}\t{1 + i}\t42\t50M\t*\t0\t0\t*\t*\n'
                   for i, (q, m, s) in enumerate(lines)).encode()


def _single(n):
    """``n`` reads of one line; every third is in the map."""
    lines = [(f'r{i}', 0, POOL[(i * 7) % len(POOL)]) for i in range(n)]
    return lines, {f'r{i}': LABELS[i % 5] for i in range(0, n, 3)}


def _shapes():
    lines, held = [], {}

    def read(q, subs, mate=0, label=None):
        lines.extend((q, mate, s) for s in subs)
        if label:
            held[T.probe_key((q, mate))] = label
    # reads of 1, 2, 16 and 17 subjects, in the map and not
    for k, n in enumerate((1, 2, 16, 17, 1, 2, 16, 17)):
        read(f'k{k}', POOL[k:k + n], label=LABELS[k % 5] if k < 4 else None)
    # a subject again inside a read: once
    read('twice', [POOL[3], POOL[4], POOL[3], POOL[5], POOL[4]], label='L1')
    # mates 0 / 1 / 2 in one run, their lines mixed, every subset in the map
    for bits in range(8):
        q = f'm{bits}'
        for mate, s in ((1, POOL[10]), (0, POOL[11]), (2, POOL[12]),
                        (1, POOL[13]), (0, POOL[10]), (2, POOL[12])):
            lines.append((q, mate, s))
        for mate in range(3):
            if bits >> mate & 1:
                held[T.probe_key((q, mate))] = LABELS[(bits + mate) % 5]
    # a run of one mate alone, of two
    read('solo', POOL[20:23], mate=2, label='L4')
    read('duo', POOL[20:22], mate=1, label='L0')
    read('duo', POOL[30:33], mate=2)
    # single lines up to 16 lines in front of the tile's end, then a run of
    # 40 lines across it
    fill = TILE - 16 - len(lines)
    assert fill > 0
    for i in range(fill):
        read(f'f{i}', [POOL[i % 64]], label=LABELS[i % 5] if i % 2 else None)
    assert len(lines) == TILE - 16
    read('across', POOL[:40], label='L2')
    for i in range(30):
        read(f'g{i}', [POOL[(3 * i) % 64]], label='L3' if i % 4 == 0 else None)
    return lines, held


BLOCKS = {f'single-{n}': (lambda n=n: _single(n))
          for n in (1, 255, 256, 257, 65537)}
BLOCKS['shapes'] = _shapes


@pytest.mark.parametrize('name', list(BLOCKS))
def test_blocks_are_placed_like_the_model(dev, name):
    lines, held = BLOCKS[name]()
    text = ''.join(f'{k}\t{v}\n' for k, v in held.items()).encode()
    # (every label once in front, so that label i is LABELS[i])
    text = ''.join(f'none{i}\t{x}\n'
                   for i, x in enumerate(LABELS)).encode() + text
    assert dev.load(text) == LABELS
    want = _model(lines, held)
    qoff, subj, group = dev.stage(_sam(lines), len(lines))
    sizes = [len(subs) for _, subs in want]
    assert qoff.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert [dev.subjects[s] for s in subj.tolist()] == \
        [s for _, subs in want for s in subs]
    assert group.tolist() == [g for g, _ in want]
    # ... and counted: 1 / k per subject of a read that has a group
    cells = {}
    for g, subs in want:
        if g >= 0:
            for s in subs:
                cells[g, s] = cells.get((g, s), 0) + Fraction(1, len(subs))
    assert dev.cells() == cells
    if name == 'shapes':
        # (`_shapes` puts the read of 40 lines 16 lines in front of a tile's end)
        assert max(sizes) == 40 and {1, 2, 16, 17} <= set(sizes)


def test_a_read_of_more_subjects_than_a_key_can_say_is_the_hosts(dev):
    assert dev.load(b'wide\tL0\n') == ['L0']
    lines = [('a', 0, 'W0000')] + [('wide', 0, s)
                                   for s in P.wide_subjects()] + \
        [('b', 0, 'W0001')]
    text = np.frombuffer(_sam(lines), dtype=np.uint8)
    assert dev.ctx.dtok_scan(dev.tok, text, 0, text.size) == (0, len(lines))
    dev.subjects.extend(dev.tok.new_subjects())
    assert dev.ctx.dtok_stage_reads_strata()[0] != 0
    with pytest.raises(RuntimeError, match='no chunk staged'):
        dev.ctx.chunk_groups(1)


# ---- c. commands ------------------------------------------------------------------
def _command(case, root, monkeypatch, **more):
    """The case through workflow.workflow; returns (tables or error, routes,
    blocks the device scanned and kept)."""
    from woltka_amd import _native as nat
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    if case['block']:
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', case['block'])
    scan, kept = nat.Context.dtok_scan, []

    def counted(self, *a, **kw):
        status, n_lines = scan(self, *a, **kw)
        kept.append(status == 0 and n_lines > 0)
        return status, n_lines
    monkeypatch.setattr(nat.Context, 'dtok_scan', counted)
    ROUTES.clear()
    got = P.run_case(workflow, case, str(root), **more)
    return got, dict(ROUTES), sum(kept)


@pytest.fixture
def clean_env(monkeypatch):
    for name in ('WOLTKA_NO_DSTRATA', 'WOLTKA_NO_DTOK'):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize('name', list(CASES))
def test_commands_match_the_reference(tmp_path, clean_env, name):
    case = CASES[name]
    got, routes, blocks = _command(case, tmp_path, clean_env)
    assert got == GOLD[name]
    if case['route'] == 'device':
        assert blocks >= (6 if case['block'] else 2)
        assert routes.get('dreads_strata', 0) == blocks and \
            routes.get('dstrata', 0) == 2 and \
            not routes.get('host_block'), routes
    elif case['route'] == 'mixed':
        assert routes.get('dreads_strata', 0) > 0 and \
            routes.get('host_block', 0) > 0 and \
            routes.get('dstrata', 0) == 2, routes
    elif case['route'] == 'host':
        assert not routes.get('dstrata') and \
            not routes.get('dreads_strata'), routes
    else:
        assert 'error' in got


@pytest.mark.parametrize('name', ['fmt-sam', 'fmt-map', 'sam-mixed', 'mates',
                                  'exclude', 'trimsub', 'gz'])
def test_the_switch_keeps_the_host_route_and_the_bytes(tmp_path, clean_env,
                                                       name):
    clean_env.setenv('WOLTKA_NO_DSTRATA', '1')
    got, routes, _ = _command(CASES[name], tmp_path, clean_env)
    assert got == GOLD[name]
    assert 'dreads_strata' not in routes and 'dstrata' not in routes, routes


def _muxed(case, root):
    """Both samples of the case in one file, the read ids behind their
    sample's name."""
    rows = []
    for s in ('S1', 'S2'):
        for row in case['files'][f'aln/{s}.sam'].decode().splitlines():
            if row[0] != '@':
                rows.append(f'{s}_{row}')
    path = os.path.join(root, 'mux.sam')
    os.makedirs(root, exist_ok=True)
    with open(path, 'w') as f:
        f.write('\n'.join(rows) + '\n')
    return path


@pytest.mark.parametrize('what', ['sizes', 'outmap', 'outcov', 'demux'])
def test_other_stratified_calls_keep_todays_route(tmp_path, clean_env, what):
    case = CASES['fmt-sam']
    results = []
    for k, switch in enumerate((False, True)):
        root = str(tmp_path / f'run{k}')
        # (per-base counts: scaled, or every cell rounds to nothing)
        more = {'sizes': dict(sizes=os.path.join(P.SC.TAX, 'length.map'),
                              scale='1M', digits=3),
                'outmap': dict(outmap_dir=os.path.join(root, 'maps')),
                'outcov': dict(outcov_dir=os.path.join(root, 'cov')),
                'demux': dict(input_fp=_muxed(case, root))}[what]
        if switch:
            clean_env.setenv('WOLTKA_NO_DSTRATA', '1')
        got, routes, _ = _command(case, root, clean_env, **more)
        assert 'tables' in got, got
        assert not routes.get('dreads_strata'), routes
        results.append(got)
    assert results[0] == results[1]
    assert all(t.count('\n') > 5 for t in results[0]['tables'].values())
