"""Position and size of a record from bit planes in the one-kernel SAM
tokenizer (csrc/wk_dtok_fused.hpp, csrc/wk_dtok_planes.hpp).

A window's owned lines are bits of 64-bit words -- run starts in one plane,
the first lines of a read (run, mate) per mate in the others, made by wave
ballots in the duplicate walk -- and a record's position and size are
population counts between the head and the end of its run.  What can go wrong
is a matter of where a line's bit lies: a head in another word than the line,
a run that ends at a word's last or first bit, 64q and 64q + 1 owned lines,
words numbered from a negative first line (carried runs), the second and
third trip of 512 lines.  (The arithmetic alone: tests/test_dtok_planes_host.py,
on the CPU.)

Compared as tests/test_gpu_dtok_scan.py compares, on its helpers: the same
block through `dtok_scan_emit` by the one kernel and by the six kernels --
status, lines, reads, records and cells (a per-subject job and a rank job: the
multiset of the record words) equal, exactly -- and kept blocks against
`_model`, the plain parser's grouping in Python.  `_owned` is the kernel's
ownership rule for these texts written out in Python: it checks on the CPU
that a text has the shape its case claims.

Geometry of the `words` cases: that of `lanes` there -- 256 KB at the default
launch, 64 spans of 128 lines of 32 bytes, a shape per span, every such span's
first line starts a read: owned line i of the span is bit i % 64 of word
i // 64.  Every read has at most 16 subjects per mate, but in `words_17`.
  words      kept   span 2: a run of 150 mapped lines, six subjects, first
                    lines in words 0, 1 and 2 (the last two with their head two
                    and one words below); span 5: runs that start at bits 63
                    and 0; span 8: a run that ends at bit 63, one that ends at
                    bit 0 of word 2, behind the span's end: 129 owned lines
                    (span 5 has exactly 128); span 11: unmapped lines inside a
                    run at bits 62, 63, 0 and 1; span 14: mate-less lines and
                    mates 1 and 2 interleaved, 16 subjects each and 48 first
                    lines, subjects shared between the mates, duplicates of
                    one mate's subject under the others
  words_17   back   the same with a 17th subject for mate 1 in span 14
                    (kDtokBigRead): the six kernels leave the block to the
                    host tokenizer
`carry_*` and `trips`: the 16 MB, `dtok_fused_per_cu` = 1 shape of the spans
test (spans of 64 KB, windows of 20 KB).
  carry_N    kept   N = 1, 63, 64, 65, 256 mapped lines of a run of both mates,
                    27 KB of unmapped lines, the run goes on: the first owned
                    line is -N, the words are numbered from there; first lines
                    on both sides of the stretch and under both mates
  trips      kept   64 KB of 24-byte lines in runs of 40 (850 owned lines a
                    window: a run across line 512, runs in words 8-13); every
                    run has first lines at its lines 0, 1, 20 and 39, so on
                    both sides of wherever line 512 falls in it
`test_dropped_runs_through_three_routes`: `--exclude`, as the test of that name
in test_gpu_dtok_scan.py, in a 16 MB block at `dtok_fused_per_cu` = 1: runs of
140 lines of 32 bytes (more than two words wherever they begin) whose first
lines are all in the run's first 20 lines, the excluded subject named at line
100 (another word than the head and the first lines), in the last line, in
the part of a carried run behind its stretch of unmapped lines, or not at all."""
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
import test_gpu_dtok_exit as X  # noqa: E402  (their helpers, as they are)
import test_gpu_dtok_scan as T  # noqa: E402
import test_gpu_dtok_spans as S  # noqa: E402
from test_gpu_dtok_scan import device  # noqa: E402,F401  (the fixture)

MAX_K = T.MAX_K
PER_SPAN = 128              # lines of 32 bytes in a span of 4 KB
MATE_FLAG = (0, 65, 129)    # mate-less, first, second
CARRIED = (1, 63, 64, 65, 256)


def _fields(line):
    q, flag, s = line.split('\t', 3)[:3]
    return q, (int(flag) >> 6) & 3, s


def _owned(lines, span):
    """The lines span `span` owns in a text of 32-byte lines whose span begins
    with a read: from its first line to the first run start at or behind its
    end.  Per line (starts a run, first line of its (run, mate) that names its
    subject, mate), None for an unmapped line."""
    k = span * PER_SPAN
    assert _fields(lines[k])[0] != _fields(lines[k - 1])[0], span
    out, seen, last_q = [], set(), None
    while k < len(lines):
        q, mate, s = _fields(lines[k])
        if s == '*':
            out.append(None)
        else:
            start = q != last_q
            if start and k >= (span + 1) * PER_SPAN:
                break
            if start:
                seen, last_q = set(), q
            out.append((start, (mate, s) not in seen, mate))
            seen.add((mate, s))
        k += 1
    return out


def _heads(own):
    """Per first line of `own`: (its index, the index of its run's head)."""
    res, head = [], 0
    for i, ln in enumerate(own):
        if ln and ln[0]:
            head = i
        if ln and ln[1]:
            res.append((i, head))
    return res


def _words_text(rng, names, big):
    lines, q = [], [0]

    def qname():
        q[0] += 1
        return f'r{q[0]:07d}'

    def single():
        lines.append(T._line32(qname(), 0, rng.choice(names)))

    def to(span, i):
        assert len(lines) <= span * PER_SPAN + i, (span, i, len(lines))
        while len(lines) < span * PER_SPAN + i:
            single()

    def run(rows):
        """rows: (flag, subject) per line, subject None = an unmapped line."""
        name = qname()
        for flag, s in rows:
            lines.append(T._line32(name, 4, '*') if s is None else T._line32(name, flag, s))

    # span 2: 150 mapped lines, six subjects, first lines in all three words
    to(2, 0)
    p = rng.sample(names, 6)
    subj = [p[0], p[1]] + [rng.choice(p[:2]) for _ in range(68)] + \
        [p[2]] + [rng.choice(p[:3]) for _ in range(4)] + [p[3]] + \
        [rng.choice(p[:4]) for _ in range(59)] + [p[4]] + \
        [rng.choice(p[:5]) for _ in range(4)] + [p[5]] + \
        [rng.choice(p) for _ in range(9)]
    assert len(subj) == 150
    run([(0, s) for s in subj])
    # span 5: run starts at bits 63 and 0
    to(5, 63)
    run([(0, rng.choice(names))])
    run([(0, s) for s in rng.sample(names, 3)] + [(0, rng.choice(names))])
    # span 8: a run that ends at bit 63; one that ends at bit 0 of word 2 (129 owned lines)
    to(8, 30)
    p = rng.sample(names, 8)                      # (the runs' last lines are first lines)
    run([(0, p[k % 7] if k % 5 == 0 else rng.choice(p[:3])) for k in range(33)] + [(0, p[7])])
    to(8, 100)
    run([(0, p[k % 7] if k % 4 == 0 else rng.choice(p[:3])) for k in range(28)] + [(0, p[7])])
    # span 11: unmapped lines inside a run, on both sides of a word boundary
    to(11, 50)
    p = rng.sample(names, 10)
    rows = [(0, p[k % 8] if k % 3 == 0 else rng.choice(p[:4])) for k in range(30)]
    for k in (12, 13, 14, 15):
        rows[k] = (4, None)
    rows[11], rows[16] = (0, p[8]), (0, p[9])     # (first lines next to them)
    run(rows)
    # span 14: three kinds of mate interleaved, 16 subjects each, 48 first lines
    to(14, 40)
    pool = rng.sample(names, 32)
    per_mate = (pool[:16], pool[8:24], pool[16:32])    # (half of a mate's subjects are the next one's too)
    rows = [(MATE_FLAG[m], per_mate[m][j]) for j in range(MAX_K) for m in range(3)]
    for _ in range(30):                                # duplicates, under every mate
        m = rng.randrange(3)
        rows.append((MATE_FLAG[m], rng.choice(per_mate[m])))
    if big:
        rows.insert(60, (MATE_FLAG[1], pool[30]))      # (mate 1 has pool[8:24])
    run(rows)
    to(64, 0)
    return ''.join(lines)


def _check_words(text, big):
    """The shapes the `words` cases claim, from the ownership rule."""
    lines = text.splitlines()
    assert len(lines) == 64 * PER_SPAN and all(len(x) == 31 for x in lines)
    own = _owned(lines, 2)
    firsts = _heads(own)
    assert len(own) == 150 and all(own) and not any(x[0] for x in own[1:])
    assert {i // 64 for i, _ in firsts if i < 150} == {0, 1, 2}
    assert {i // 64 - h // 64 for i, h in firsts if i < 150} == {0, 1, 2}
    own = _owned(lines, 5)
    assert len(own) == 128 and own[63][0] and own[64][0] and not own[65][0]
    assert own[65][1] and own[66][1]
    own = _owned(lines, 8)
    assert len(own) == 129 and own[30][0] and own[64][0] and \
        not any(x[0] for x in own[31:64]) and own[100][0] and \
        not any(x[0] for x in own[101:129])
    assert (63, 30) in _heads(own) and (128, 100) in _heads(own)
    own = _owned(lines, 11)
    assert own[50][0] and [own[i] is None for i in range(61, 67)] == \
        [False, True, True, True, True, False]
    assert own[61][1] and own[66][1] and not own[66][0]
    own = _owned(lines, 14)
    run = [x for x in own[40:40 + 78 + big]]
    assert own[40][0] and not any(x[0] for x in run[1:]) and own[40 + 78 + big][0]
    per = [sum(1 for x in run if x[1] and x[2] == m) for m in range(3)]
    assert per == [16, 16 + big, 16], per
    assert any(not x[1] for x in run[48:])
    return max(per)


def _carry_rows(rng, names, n):
    """A run of n mapped lines in front of a stretch of unmapped lines and 12
    behind it, both mates on both sides, first lines on both sides."""
    p = rng.sample(names, 12)
    front = [(MATE_FLAG[1 + k % 2], p[k % 6] if k < 12 else rng.choice(p[:6])) for k in range(n)]
    back = [(MATE_FLAG[1 + k % 2], p[6 + k // 2] if k % 4 < 2 else rng.choice(p[:9])) for k in range(12)]
    return front, back


def _carry_text(rng, names, n):
    t = S._Text(rng, names)
    for span in (40, 120, 200):
        t.plain_to(span * S.SPAN + 30000)
        q = t.qname()
        front, back = _carry_rows(rng, names, n)
        t.add(''.join(f'{q}\t{f}\t{s}\t{T.TAIL}\n' for f, s in front))
        t.unmapped(27 << 10, q)
        t.add(''.join(f'{q}\t{f}\t{s}\t{T.TAIL}\n' for f, s in back))
    t.plain_to(S.BLOCK - 256)
    return t.text()


def _trips_text(rng, names):
    t = S._Text(rng, names)
    t.plain_to(90 * S.SPAN + 2000)
    n = 0
    while n < 64 << 10:
        q = f'd{n:010d}'                        # 11 bytes: lines of 24
        p = rng.sample(names, 4)
        subj = [p[0], p[1]] + [rng.choice(p[:2]) for _ in range(18)] + [p[2]] + \
            [rng.choice(p[:3]) for _ in range(18)] + [p[3]]
        ln = ''.join(f'{q}\t0\t{s}\t\n' for s in subj)
        assert len(ln) == 40 * 24
        t.add(ln)
        n += len(ln)
    t.plain_to(S.BLOCK - 256)
    return t.text()


#        case: (text, kept by the one kernel, dtok_fused_per_cu)
CASES = {
    'words': (lambda r, n: _words_text(r, n, False), True, 3),
    'words_17': (lambda r, n: _words_text(r, n, True), False, 3),
    'trips': (lambda r, n: _trips_text(r, n), True, 1),
}
CASES.update({f'carry_{c}': (lambda r, n, c=c: _carry_text(r, n, c), True, 1)
              for c in CARRIED})


@pytest.mark.parametrize('case', sorted(CASES))
def test_block_through_both_kernels(device, case):  # noqa: F811
    """Status, lines, reads, records and cells of one block through the one
    kernel and through the six, whether the one kernel kept it, and (kept
    blocks) the counts of the model."""
    ctx, nat, jobs, tok, names = device
    make, kept, per_cu = CASES[case]
    text = make(random.Random(f'planes:{case}'), names)
    lines, reads, records, largest, short = T._model(text)
    assert short == 0
    if case.startswith('words'):
        assert len(text) == T.SMALL
        assert _check_words(text, case == 'words_17') == largest
        assert largest == MAX_K + (case == 'words_17')
    else:
        assert S.SPAN * 255 < len(text) <= S.BLOCK       # (256 spans of 64 KB)
        assert largest <= MAX_K
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
    print('planes', case, got[1][:4], got[1][5], 'model',
          (lines, reads, records, largest))
    assert got[0][5] == (0, 0), case
    assert got[0][:4] == got[1][:4], case
    assert np.array_equal(got[0][4][0], got[1][4][0]) and \
        np.array_equal(got[0][4][1], got[1][4][1]), case
    assert got[1][5] == ((1, 0) if kept else (0, 1)), case
    if kept:
        assert got[1][:4] == (0, lines, reads, records), case
    else:       # (the six kernels leave such a block to the host tokenizer)
        assert got[1][0] == 1, case


def test_dropped_runs_through_three_routes(tmp_path, monkeypatch):
    """`--exclude` where the line that names the excluded subject, the run's
    head and its first lines lie in different words of the planes (see the
    module's docstring); three routes, equal tables and logs."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', S.BLOCK)
    monkeypatch.setattr(device_text, 'TRIM', False)
    X._per_cu(monkeypatch, 1)
    rng = random.Random('planes:exclude')
    subjects = D.tax_subjects()
    ex, rest = subjects[0], subjects[1:]
    out, q, dropped, carried = [D.HEADER], 0, 0, 0
    size = len(D.HEADER)
    # (The sample's blocks are 1, 4 and 16 MB and a rest, the first scanned the two-call way, as in the spans test:
    # the runs stay inside the 16 MB block, from 5.5 to 20.5 MB -- the spans of the others are single windows, which
    # look 3 KB ahead and no further.)
    while size < (23 << 20 | 1 << 19):
        q += 1
        name = f'r{q:07d}'
        if q % 9 or not (5 << 20 | 1 << 19) < size < 20 << 20:
            out.append(T._line32(name, 0, rng.choice(rest)))
            size += 32
            continue
        pool = rng.sample(rest, 5)
        flags = (0,) if q % 2 else (65, 129)
        run = [(f, s) for s in pool for f in flags] + [(rng.choice(flags), pool[0])] * 10
        run += [(rng.choice(flags), rng.choice(pool[:2])) for _ in range(140 - len(run))]
        where = (100, 139, None, 'carried')[(q // 9) % 4]
        if where == 'carried' and (q // 9) % 400 != 3:
            where = None                       # (a stretch of 27 KB each: a few of them)
        rows = [T._line32(name, f, s) for f, s in run]
        if where == 'carried':
            rows[70:70] = [T._line32(name, 4, '*')] * (27 << 5)
            rows[-30] = T._line32(name, run[-30][0], ex)
            carried += 1
            dropped += 1
        elif where is not None:
            rows[where] = T._line32(name, run[where][0], ex)
            dropped += 1
        out.extend(rows)
        size += 32 * len(rows)
    assert dropped > 1000 and carried >= 5, (dropped, carried)
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(D.HEADER + D._prologue(subjects))
    (indir / 'S2.sam').write_text(''.join(out))
    per_file = X._spy_counts(monkeypatch)
    tax = os.path.join(ROOT, 'tests', 'golden', 'data', 'taxonomy')
    kw = dict(input_fp=str(indir), input_fmt='sam', exclude=ex,
              nodes_fps=[os.path.join(tax, 'nodes.dmp')],
              map_fps=[os.path.join(tax, 'taxid.map')],
              ranks='none,phylum,genus')
    tables, routes = X._three_routes(tmp_path, monkeypatch, **kw)
    fused, back = [x - y for x, y in zip(per_file[2], per_file[1])]
    print('routes exclude', routes, per_file)
    assert routes['dtok_fused'] > 0 and fused > 0, (routes, per_file)
    assert back == 0, (routes, per_file)
    assert routes.get('host_block', 0) == 0, routes
    assert not any(f'{ex}\t'.encode() in t for t in tables.values())
