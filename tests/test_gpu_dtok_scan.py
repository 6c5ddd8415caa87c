"""The line phases of the one-kernel SAM tokenizer (csrc/wk_dtok_fused.hpp):
newline masks with a wave-uniform interior path, the first three tabs of a
line from one 32-bit mask, and position and size of a record inside its read.

Compared as tests/test_gpu_dtok_spans.py compares: the same block goes through
`dtok_scan_emit` by the one kernel and by the six kernels (wk_dtok.hpp, the
in-tree reference): status, lines, reads, records and cells are equal, exactly.
The record words themselves do not leave the library (the C ABI has no call
for them), so two jobs stand for their multiset: the per-subject job's cells
are the sum of 1/size per subject, the rank job's the same per taxon, and
`reads` counts the records of position 0.  Every kept block is also held
against `_model`, the plain parser's grouping written out in Python (runs of
equal QNAME over mapped lines, a set of subjects per mate), which also checks
on the CPU that each text has the shape its case is named for: the largest
read is 16 or 17, a line is short or not.

Geometry.  Single window: blocks of 256 KB at the default launch are 64 spans
of 4 KB, one window of 8 KB each.  The `lanes` texts are made of 32-byte lines
and every span's first line starts a read, so a span's owned lines are
numbered from that line: line i of a span sits at lane i % 64 of wave i // 64
of the records loop, 128 lines to a span and up to 96 more of its last run
behind it -- the smallest shape in which a run crosses a wave inside a
window.  There the span's end t1 (window offset 5 120) lies in the second
wave's last round, the 33 chunks that never take the interior path; `tabs_t1`
is the shape in which a full round straddles it: 1.5 MB at
`dtok_fused_per_cu` = 1 are 256 spans of 6 144 bytes, still one window each,
and t1 at window offset 7 168 lies inside the third wave's second round
(offsets 6 176-7 200).  Several windows and carry: the 16 MB,
`dtok_fused_per_cu` = 1 shape of the spans test (spans of 64 KB, windows of
20 KB).

Flags.  The flag word of a block does not leave the library either: the ABI
reports a status and the counts of blocks kept and handed back.  So a
handed-back case asserts the hand-back and that the six kernels leave the
block to the host tokenizer (status 1: they raise the same flag), and its
text is that of a kept case plus the one line or read that is out of bounds
(`tabs` for `two_tabs` and `no_flag`, `lanes` for `lanes_17`): nothing but
that line can be the reason.

Cases (kept = the one kernel keeps the block):
  tabs, tabs_open      kept    QNAMEs of 2-44 bytes x RNAMEs of 8, 16 and 29
                               bytes x FLAGs of 1, 3 and 6 digits: the third
                               tab at every byte from 13 to 82 of its line (30,
                               31, 32, 33 among them), the first and second
                               beyond byte 32 too; lines of 15-31 bytes one
                               behind the other (the next line's tabs inside
                               a line's 32 bytes); a line start at every
                               offset mod 16; a length that is no multiple of
                               16; with and without a last newline
  tabs_t1              kept    the same sweep in the shape whose span end lies
                               inside a full round of a wave's chunks
  two_tabs, no_flag    back    one line of exactly two tabs / an empty FLAG
                               among the above (kDtokShortLine)
  lanes                kept    runs at lanes 63 and 0; of 120 and 200 lines
                               with six subjects; both mates and mate-less
                               lines interleaved, different counts per mate;
                               unmapped lines inside a run; reads of exactly
                               16 subjects, across a wave and with duplicates
  lanes_17             back    the same and a read of 17 subjects across a
                               wave (kDtokBigRead)
  windows              kept    16 MB: a run carried over 27 KB of unmapped
                               lines with first lines on both sides; 64 KB of
                               24-byte lines in runs of 40 (850 owned lines a
                               window, a run across line 512)
`test_file_through_three_routes`: the `tabs` shapes as a file, blocks of
256 KB, through the one kernel, the six kernels (WOLTKA_NO_FUSED=1) and the
host tokenizer (WOLTKA_NO_DTOK=1): same tables, same log.
`test_dropped_runs_through_three_routes`: `--exclude` on a file of 32-byte
lines with runs of 70 lines that name the excluded subject first, in the
middle, last or not at all.  The reader cuts the blocks, so the test does not
know a line's lane; a run of more than 64 owned lines holds lanes 63 and 0
next to each other wherever it begins, and 2 240 bytes are less than a span
looks ahead, so the blocks are kept."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dtok_limits as D  # noqa: E402
import test_gpu_dtok_exit as X  # noqa: E402  (its helpers, as they are)
import test_gpu_dtok_spans as S  # noqa: E402

TAIL = X.TAIL
SMALL = 1 << 18             # 64 spans of 4 KB at the default launch
MAX_K = 16                  # WK_WEIGHT_MAX_K
T1_SPAN = 6144              # (256 spans: t1 inside a full round, see above)


def _long16(name):
    return name + '_subject'                 # 16 bytes


def _long29(name):
    return name + '.a_subject_of_some_len'   # 29 bytes


def _model(text):
    """(lines, reads, records, largest read, short lines) of a SAM text as the
    plain parser groups it."""
    rows = text.split('\n')
    if rows[-1] == '':
        rows.pop()
    reads = records = largest = short = 0
    last_q, sets = None, {}

    def close():
        nonlocal reads, records, largest
        for subjects in sets.values():
            reads += 1
            records += len(subjects)
            largest = max(largest, len(subjects))
        sets.clear()
    for row in rows:
        f = row.split('\t', 3)
        if len(f) < 4 or not f[1].isdigit():
            short += 1
            continue
        if f[2] == '*':
            continue
        if f[0] != last_q:
            close()
            last_q = f[0]
        sets.setdefault((int(f[1]) >> 6) & 3, set()).add(f[2])
    close()
    return len(rows), reads, records, largest, short


class _Filler:
    """Reads of 1-3 lines, QNAMEs of 2-14 bytes, around the cases' shapes."""

    def __init__(self, rng, names):
        self.rng, self.names = rng, names
        self.out, self.n, self.q = [], 0, 0

    def add(self, s):
        self.out.append(s)
        self.n += len(s)

    def qname(self, width=None):
        self.q += 1
        q = 'q' + 'x' * (self.q % 7) + str(self.q)
        return q if width is None else ('y' * width + q)[-width:]

    def plain(self, nbytes):
        stop = self.n + nbytes
        while self.n < stop:
            q = self.qname()
            for _ in range(self.rng.choice([1, 1, 1, 2, 3])):
                self.add(f'{q}\t0\t{self.rng.choice(self.names)}\t{TAIL}\n')

    def text(self):
        return ''.join(self.out)


def _tabs_text(rng, names, bad=None, size=SMALL):
    """The sweep of the module's docstring between plain reads, `size` bytes
    (up to 600 fewer)."""
    t = _Filler(rng, names)
    t.plain(9000)
    thirds, starts = set(), set()
    for qlen in range(2, 45):
        for kind in (str, _long16, _long29):
            for flag in ('0', '163', '000064'):
                q, s = t.qname(qlen), kind(rng.choice(names))
                assert len(q) == qlen
                thirds.add(qlen + len(flag) + len(s) + 2)
                starts.add(t.n % 16)
                t.add(f'{q}\t{flag}\t{s}\t{TAIL}\n')
        t.plain(rng.choice([0, 0, 90]))
    assert thirds >= set(range(13, 83)), sorted(thirds)
    t.plain(5000)
    for rep in range(6):
        for n in range(15, 32):     # (q + 13 bytes, then a byte of a fourth field)
            q = t.qname(n - 13 - (n > 20))
            starts.add(t.n % 16)
            line = f'{q}\t0\t{rng.choice(names)}\t' + ('x' if n > 20 else '') + '\n'
            assert len(line) == n
            t.add(line)
    assert starts == set(range(16)), sorted(starts)
    t.plain(3000)
    if bad == 'two_tabs':
        t.add(f'{t.qname()}\t0\t{names[3]}\n')
    elif bad == 'no_flag':
        t.add(f'{t.qname()}\t\t{names[3]}\t{TAIL}\n')
    t.plain(size - 600 - t.n)
    while t.n % 16 in (0, 1):       # (no multiple of 16, with or without the last newline)
        t.add(f'{t.qname(3 + t.n % 5)}\t0\t{names[0]}\t{TAIL}\n')
    return t.text()


def _line32(q, flag, s):
    """A line of exactly 32 bytes (QNAME and subject of 8)."""
    head = f'{q}\t{flag}\t{s}\t'
    assert len(q) == 8 and len(s) in (1, 8, 10) and len(head) <= 31
    return head + 'x' * (31 - len(head)) + '\n'


def _lanes_text(rng, names, big):
    """8 192 lines of 32 bytes: 64 spans of 128 lines, a shape per span at known
    lanes (see the module's docstring), single reads between them."""
    lines, q = [], [0]

    def qname():
        q[0] += 1
        return f'r{q[0]:07d}'

    def single():
        lines.append(_line32(qname(), 0, rng.choice(names)))

    def to(span, i):
        assert len(lines) <= span * 128 + i, (span, i, len(lines))
        while len(lines) < span * 128 + i:
            single()

    def run(subjects, flags=(0,), unmapped=()):
        # (`flags`: one per line, or what a line's is drawn from)
        name = qname()
        for k, s in enumerate(subjects):
            if k in unmapped:
                lines.append(_line32(name, 4, '*'))
            flag = flags[k] if len(flags) == len(subjects) else rng.choice(flags)
            lines.append(_line32(name, flag, s))

    to(2, 63)                                   # lanes 63 and 0
    run(rng.sample(names, 2))
    to(4, 10)                                   # 120 lines over three waves
    run([rng.choice(names[:6]) for _ in range(120)])
    to(7, 5)                                    # 200 lines, past the span's end
    run([rng.choice(names[10:16]) for _ in range(200)])
    to(11, 50)                                  # mates interleaved, across a wave
    run([rng.choice(names[:9]) for _ in range(30)], flags=(0, 0, 65, 129, 129, 129))
    to(14, 120)                                 # ... and across the span's end
    run([rng.choice(names[:12]) for _ in range(40)], flags=(0, 65, 65, 65, 129))
    to(18, 56)                                  # unmapped lines inside a run
    run([rng.choice(names[:5]) for _ in range(16)], unmapped=(1, 7, 8, 9, 15))
    to(21, 56)                                  # exactly 16 subjects across a wave
    run(rng.sample(names, MAX_K))
    to(24, 20)                                  # ... and with duplicates
    pool = rng.sample(names, MAX_K)
    run(pool + [rng.choice(pool) for _ in range(14)])
    to(27, 60)                                  # 16 per mate
    run([s for pair in zip(rng.sample(names, MAX_K), rng.sample(names, MAX_K)) for s in pair], flags=(65, 129) * MAX_K)
    if big:
        to(30, 55)
        run(rng.sample(names, MAX_K + 1))
    to(64, 0)
    for span in (2, 4, 7, 11, 14, 18, 21, 24, 27, 30):   # (their first line starts a read: line i at lane i % 64)
        assert lines[span * 128][:8] != lines[span * 128 - 1][:8]
    return ''.join(lines)


def _windows_text(rng, names):
    t = S._Text(rng, names)
    t.plain_to(40 * S.SPAN + 30000)
    q = t.run(3)
    t.unmapped(27 << 10, q)
    t.run(4, q)
    t.plain_to(90 * S.SPAN + 2000)
    n = 0
    while n < 64 << 10:
        q = f'd{n:010d}'                        # 11 bytes: lines of 24
        pool = rng.sample(names, 5)
        ln = ''.join(f'{q}\t0\t{rng.choice(pool)}\t\n' for _ in range(40))
        assert len(ln) == 40 * 24
        t.add(ln)
        n += len(ln)
    t.plain_to(S.BLOCK - 256)
    return t.text()


#        case: (text, kept by the one kernel, dtok_fused_per_cu)
CASES = {
    'tabs': (lambda r, n: _tabs_text(r, n), True, 3),
    'tabs_open': (lambda r, n: _tabs_text(r, n)[:-1], True, 3),
    'tabs_t1': (lambda r, n: _tabs_text(r, n, size=T1_SPAN * 256), True, 1),
    'two_tabs': (lambda r, n: _tabs_text(r, n, 'two_tabs'), False, 3),
    'no_flag': (lambda r, n: _tabs_text(r, n, 'no_flag'), False, 3),
    'lanes': (lambda r, n: _lanes_text(r, n, False), True, 3),
    'lanes_17': (lambda r, n: _lanes_text(r, n, True), False, 3),
    'windows': (lambda r, n: _windows_text(r, n), True, 1),
}
SHORT = ('two_tabs', 'no_flag')


def _names():
    """The subjects of test_gpu_dtok_exit._totals_context's tree, each under
    three names: 8, 16 and 29 bytes."""
    from woltka_amd import synth
    tp = synth.as_sets(synth.lca_problem(
        np.random.default_rng(1), n_nodes=5000, n_subjects=500, n_reads=4000))
    return tp, [f'T{s:07d}' for s in np.unique(tp['subj']).tolist()]


@pytest.fixture
def device():
    """A context of its own for every case: after two blocks in a row that the
    one kernel hands back, a context leaves it out for the blocks that follow.
    (A COPY of test_gpu_dtok_exit._totals_context, which cannot take
    parameters without changing that file: the same tree and rank table, but
    every subject under three names and a per-subject job next to the rank
    job.  Keep the two in step.)"""
    from woltka_amd import _native as nat
    tp, names = _names()
    th = tp['hier']
    with nat.Context(0) as ctx:
        ctx.set_tree(th.parent, th.last, th.rank_code)
        ctx.build_rank_table(0, th.rank_codes['genus'])
        ctx.counts_reserve(1 << 18)
        ctx.dtok_format('sam')
        jobs = [nat.Job(nat.MODE_NONE, 0, 0, 0, 0.0),
                nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)]
        tok = nat.Tokenizer(2)
        every = [k(s) for s in names for k in (str, _long16, _long29)]
        text = np.frombuffer(''.join(
            f'p{i}\t0\t{s}\t*\n' for i, s in enumerate(every)).encode(),
            np.uint8)
        status, n_lines = ctx.dtok_scan(tok, text, 0, text.size)
        assert status == 0 and n_lines == len(every)
        ctx.set_subjects(np.asarray([int(x[1:8]) for x in tok.new_subjects()],
                                    dtype=np.int32))
        assert ctx.words_begin(jobs, 0)
        assert ctx.dtok_emit()[0] == 0
        ctx.words_flush()
        ctx.counts_clear()
        try:
            yield ctx, nat, jobs, tok, names
        finally:
            ctx.tune('dtok_fused', 1)
            ctx.tune('dtok_fused_per_cu', 3)
            tok.close()


def _text(case):
    _, names = _names()
    return CASES[case][0](random.Random(f'scan:{case}'), names)


@pytest.mark.parametrize('case', sorted(CASES))
def test_block_through_both_kernels(device, case):
    """Status, lines, reads, records and cells of one block through the one
    kernel and through the six, whether the one kernel kept it, and (kept
    blocks) the counts of `_model`."""
    ctx, nat, jobs, tok, names = device
    text = _text(case)
    kept, per_cu = CASES[case][1:]
    lines, reads, records, largest, short = _model(text)
    if per_cu == 3:
        assert 4096 * 63 < len(text) <= SMALL            # (64 spans of 4 KB)
    elif case == 'tabs_t1':
        assert (T1_SPAN - 16) * 256 < len(text) <= T1_SPAN * 256
    else:
        assert S.SPAN * 255 < len(text) <= S.BLOCK       # (256 of 64 KB)
    assert short == (1 if case in SHORT else 0), (case, short)
    assert largest == (MAX_K + 1 if case == 'lanes_17' else MAX_K) or \
        not case.startswith('lanes'), (case, largest)
    assert largest <= MAX_K or case == 'lanes_17', (case, largest)
    if case.startswith('tabs'):
        assert len(text) % 16 != 0 and text.endswith('\n') == (case != 'tabs_open')
    raw = np.frombuffer(text.encode(), np.uint8)
    ok, begin, stop, _ = nat.Tokenizer.sam_span(raw, True, False, 'sam')
    assert ok and begin == 0 and stop == raw.size
    ctx.tune('dtok_fused_per_cu', per_cu)
    got = {}
    for fused in (0, 1):
        ctx.tune('dtok_fused', fused)
        assert ctx.words_begin(jobs, 0)
        before = ctx.dtok_fused_counts()
        status, n_lines, n_reads = ctx.dtok_scan_emit(tok, raw, begin, stop)
        if status == 0 and n_reads is None:     # (scanned only: the second call)
            st, n_reads, _ = ctx.dtok_emit()
            assert st == 0, (case, fused)
        n_records = ctx.words_pending()[0]
        ctx.words_flush()
        after = ctx.dtok_fused_counts()
        cells = nat.canonical_counts(*ctx.counts_fetch())
        ctx.counts_clear()
        got[fused] = (status, n_lines if status == 0 else None,
                      n_reads if status == 0 else None, n_records, cells,
                      (after[0] - before[0], after[1] - before[1]))
    print('scan', case, got[1][:4], got[1][5], 'model',
          (lines, reads, records, largest, short))
    assert got[0][5] == (0, 0), case
    assert got[0][:4] == got[1][:4], case
    assert np.array_equal(got[0][4][0], got[1][4][0]) and \
        np.array_equal(got[0][4][1], got[1][4][1]), case
    assert got[1][5] == ((1, 0) if kept else (0, 1)), case
    if kept:
        assert got[1][:4] == (0, lines, reads, records), case
    else:       # (the six kernels leave such a block to the host tokenizer)
        assert got[1][0] == 1, case


def test_file_through_three_routes(tmp_path, monkeypatch):
    """The `tabs` shapes as a file in blocks of 256 KB (the names of 16 and 29
    bytes are subjects of their own here): three routes, equal tables and
    logs, no block handed back behind the first."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', SMALL)
    monkeypatch.setattr(device_text, 'TRIM', False)
    rng = random.Random('scan:file')
    subjects = [f'g{i:07d}' for i in range(60)]
    every = [k(s) for s in subjects for k in (str, _long16, _long29)]
    body = _tabs_text(rng, subjects) + _tabs_text(rng, subjects) + _tabs_text(rng, subjects)[:-1]
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(D.HEADER + D._prologue(every) + body)
    per_file = X._spy_counts(monkeypatch)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    tables, routes = X._three_routes(tmp_path, monkeypatch, **kw)
    print('routes', routes, per_file)
    assert routes['dtok_fused'] > 0, routes
    assert routes.get('dtok_fused_back', 0) == 0, routes
    assert routes.get('host_block', 0) == 0, routes


def test_dropped_runs_through_three_routes(tmp_path, monkeypatch):
    """`--exclude`: runs of 70 lines of 32 bytes dropped whole, across a wave
    of the records loop (see the module's docstring); three routes, equal
    tables and logs."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', SMALL)
    monkeypatch.setattr(device_text, 'TRIM', False)
    rng = random.Random('scan:exclude')
    subjects = D.tax_subjects()
    ex, rest = subjects[0], subjects[1:]
    out, q, dropped = [], 0, 0
    while len(out) < 24000:                 # (768 KB)
        q += 1
        name = f'r{q:07d}'
        if q % 9:
            out.append(_line32(name, 0, rng.choice(rest)))
            continue
        pool = rng.sample(rest, 5)
        run = [rng.choice(pool) for _ in range(70)]
        where = (0, 35, 69, None)[(q // 9) % 4]
        if where is not None:
            run[where] = ex
            dropped += 1
        flags = (0,) if q % 2 else (65, 129)
        out.extend(_line32(name, rng.choice(flags), s) for s in run)
    assert dropped > 100
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(D.HEADER + D._prologue(subjects) +
                                  ''.join(out))
    tax = os.path.join(ROOT, 'tests', 'golden', 'data', 'taxonomy')
    kw = dict(input_fp=str(indir), input_fmt='sam', exclude=ex,
              nodes_fps=[os.path.join(tax, 'nodes.dmp')],
              map_fps=[os.path.join(tax, 'taxid.map')],
              ranks='none,phylum,genus')
    tables, routes = X._three_routes(tmp_path, monkeypatch, **kw)
    print('routes exclude', routes)
    assert routes['dtok_fused'] > 0, routes
    assert routes.get('dtok_fused_back', 0) == 0, routes
    assert routes.get('host_block', 0) == 0, routes
    assert not any(f'{ex}\t'.encode() in t for t in tables.values())
