"""The exit path of the one-kernel SAM tokenizer (csrc/wk_dtok_fused.hpp): one
flush for all slices' record buffers (`flush_all`), the block's totals as one
packed add behind the DtokState, the block's records as the cursors' advance
over the ring buffer in front of the block.

The same files go through three routes -- the one kernel, the six kernels
(WOLTKA_NO_FUSED=1) and the host tokenizer (WOLTKA_NO_DTOK=1, which the
reference fixtures pin elsewhere) -- and must give the same tables and the same
log; where a case is meant to be kept by the one kernel, ROUTES says it was.

Geometry of the cases that fill a record buffer before a workgroup's last
tile: `dtok_fused_per_cu` = 1 (256 workgroups) and blocks of 16 MB read
untrimmed, so that the 41-byte lines reach the kernel as they are: four rounds
of 16 KB tiles, about 1 600 records per workgroup against kFzCap = 1024 -- the
buffers leave once mid-kernel and once at the exit."""
import os
import random
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dtok_limits as D  # noqa: E402
import test_gpu_dtok as T  # noqa: E402  (its `_run` and `_fused_sam`, as they are)

TAIL = '1\t42\t50M\t*\t0\t0\t*\t*'


def _per_cu(monkeypatch, per_cu):
    from woltka_amd import _native as nat
    init = nat.Context.__init__

    def init_tuned(self, *a, **k):
        init(self, *a, **k)
        self.tune('dtok_fused_per_cu', per_cu)
    monkeypatch.setattr(nat.Context, '__init__', init_tuned)


def _spy_counts(monkeypatch):
    """(blocks kept, blocks handed back) so far, noted at the end of each file."""
    from woltka_amd import _native as nat
    per_file = [(0, 0)]
    counts = nat.Context.dtok_fused_counts

    def spy(self):
        res = counts(self)
        per_file.append(tuple(res))
        return res
    monkeypatch.setattr(nat.Context, 'dtok_fused_counts', spy)
    return per_file


def _three_routes(tmp_path, monkeypatch, **kw):
    """The tables and logs of the three routes are equal; returns the tables
    and the one-kernel run's ROUTES."""
    from woltka_amd.hostio import ROUTES
    ROUTES.clear()
    a, log_a = T._run(tmp_path, 'fused', False, **kw)
    routes_a = dict(ROUTES)
    monkeypatch.setenv('WOLTKA_NO_FUSED', '1')
    ROUTES.clear()
    b, log_b = T._run(tmp_path, 'six', False, **kw)
    assert ROUTES['dtok_fused'] == 0 and ROUTES['dtok'] > 0, dict(ROUTES)
    monkeypatch.delenv('WOLTKA_NO_FUSED')
    h, log_h = T._run(tmp_path, 'host', True, **kw)
    assert a == b == h
    assert log_a == log_b == log_h
    return a, routes_a


@pytest.mark.parametrize('n_subjects,skip', [(90, None), (2 * D.SLICE - 200, None),
                                             (150_000, 2)],
                         ids=['1slice', '2slices', '4slices_one_empty'])
def test_buffers_that_fill_before_the_last_tile(tmp_path, monkeypatch,
                                                n_subjects, skip):
    """One, two and four slices of subjects (kSliceBins = 40 608 a slice); with
    four, no read of the second sample names a subject of slice `skip`: a slice
    that receives no record at all.  The first sample names every subject
    (dtok_limits._slices), so that the second sample's blocks are kept."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 24)
    monkeypatch.setattr(device_text, 'TRIM', False)
    _per_cu(monkeypatch, 1)
    rng = random.Random(f'exit:{n_subjects}')
    pool = [s for s in range(n_subjects)
            if skip is None or s // D.SLICE != skip]
    indir = tmp_path / 'in'
    indir.mkdir()
    first = D._slices(rng, n_subjects, None)
    (indir / 'S1.sam').write_text(first)
    # The reader's blocks of a sample are 1, 4 and 16 MB and a rest (`ramp`)
    # until a sample has reached the full block; from then on (a first sample
    # of two blocks: more than 1 MB) 16 MB from the start.  A sample's first
    # block is scanned the two-call way: the 16 MB block that goes through the
    # one kernel is the third, or the second.
    warm = len(first) > 1 << 20
    out, size, q = [D.HEADER], 0, 0
    while size < (35 if warm else 23) << 20:
        for _ in range(rng.choice([1, 1, 1, 2, 3])):
            out.append(f'q{q:07d}\t0\tg{rng.choice(pool):06d}\t{TAIL}\n')
            size += 41
        q += 1
    (indir / 'S2.sam').write_text(''.join(out))
    per_file = _spy_counts(monkeypatch)
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    tables, routes = _three_routes(tmp_path, monkeypatch, **kw)
    # (the second sample of the one-kernel run: every block behind its first
    # one was kept, none was handed back)
    s2 = [x - y for x, y in zip(per_file[2], per_file[1])]
    print('routes', n_subjects, routes, per_file)
    assert s2 == [2 if warm else 3, 0], (routes, per_file)
    assert routes['dtok_fused'] > 0, routes


def _totals_context(ctx, nat):
    """A small tree, a rank job and a tokenizer that knows every subject."""
    from woltka_amd import synth
    tp = synth.as_sets(synth.lca_problem(
        np.random.default_rng(1), n_nodes=5000, n_subjects=500, n_reads=4000))
    th = tp['hier']
    ctx.set_tree(th.parent, th.last, th.rank_code)
    ctx.build_rank_table(0, th.rank_codes['genus'])
    ctx.counts_reserve(1 << 18)
    ctx.dtok_format('sam')
    job = [nat.Job(nat.MODE_RANK, 0, 0, 0, 0.0)]
    names = [f'T{s:07d}' for s in np.unique(tp['subj']).tolist()]
    tok = nat.Tokenizer(2)
    text = np.frombuffer(''.join(
        f'p{i}\t0\t{s}\t*\n' for i, s in enumerate(names)).encode(), np.uint8)
    status, n_lines = ctx.dtok_scan(tok, text, 0, text.size)
    assert status == 0 and n_lines == len(names)
    ctx.set_subjects(np.asarray([int(x[1:]) for x in tok.new_subjects()],
                                dtype=np.int32))
    assert ctx.words_begin(job, 0)
    assert ctx.dtok_emit()[0] == 0
    ctx.words_flush()
    ctx.counts_clear()
    return job, tok, names


def _block_texts(names):
    rng = random.Random('totals')
    body, size = [], 0
    for ln in T._fused_sam(rng, 40, names, 'plain').split('\n')[2:]:
        if size + len(ln) + 1 > 4000:    # (one tile: a grid of one workgroup)
            break
        body.append(ln + '\n')
        size += len(ln) + 1
    body = ''.join(body)
    assert 3000 < len(body) <= 4000
    unmapped = ''.join(f'u{i // 3}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n'
                       for i in range(30000))
    # (reads of eight lines that name one subject: a record per eight lines)
    tiny = ''.join(f'r{q}\t0\t{names[q % 7]}\t\n' * 8 for q in range(5000))
    return {
        'one_tile': body,
        'open_end': T._fused_sam(rng, 20000, names, 'open_end').split(
            '\n', 2)[2],
        'unmapped_only': unmapped,
        'tiny': tiny,
    }


def test_block_totals_equal_the_six_kernels():
    """`n_lines`, `n_reads` and the records of a block as `dtok_scan_emit`
    reports them (the records: `words_pending`), through the one kernel and
    through the six, and the cells both leave."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        job, tok, names = _totals_context(ctx, nat)
        try:
            for name, text in _block_texts(names).items():
                raw = np.frombuffer(text.encode(), np.uint8)
                ok, begin, stop, _ = nat.Tokenizer.sam_span(raw, True, False,
                                                            'sam')
                assert ok and begin == 0 and stop == raw.size, name
                got = {}
                for fused in (0, 1):
                    ctx.tune('dtok_fused', fused)
                    assert ctx.words_begin(job, 0)
                    before = ctx.dtok_fused_counts()
                    status, n_lines, reads = ctx.dtok_scan_emit(tok, raw,
                                                                begin, stop)
                    assert status == 0, (name, fused)
                    if reads is None:       # (scanned only: the second call)
                        st, reads, _ = ctx.dtok_emit()
                        assert st == 0, (name, fused)
                    records = ctx.words_pending()[0]
                    ctx.words_flush()
                    after = ctx.dtok_fused_counts()
                    cells = nat.canonical_counts(*ctx.counts_fetch())
                    ctx.counts_clear()
                    assert (after[0] - before[0], after[1] - before[1]) == \
                        (fused, 0), (name, fused, before, after)
                    got[fused] = (n_lines, reads, records, cells)
                print('totals', name, got[1][:3])
                assert got[0][:3] == got[1][:3], name
                assert np.array_equal(got[0][3][0], got[1][3][0]) and \
                    np.array_equal(got[0][3][1], got[1][3][1]), name
                lines = text.count('\n') + (0 if text.endswith('\n') else 1)
                assert got[1][0] == lines, name
                if name == 'unmapped_only':
                    assert got[1][1:3] == (0, 0)
                if name == 'tiny':
                    assert got[1][2] == lines // 8
        finally:
            ctx.tune('dtok_fused', 1)
            tok.close()


def test_one_workgroup_flags_the_block(tmp_path, monkeypatch):
    """One subject the dictionary does not know, named once, in the last tile
    of the second 256 KB block of a text that is otherwise clean: the block is
    handed back, the name is listed in the table, the tables are the host's."""
    from woltka_amd import classify as C
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 18)
    rng = random.Random('exit:flags')
    subjects = D.tax_subjects()
    out, size, q, planted = [D.HEADER, D._prologue(subjects)], 0, 0, False
    size = sum(map(len, out))
    while size < 5 << 18:
        if not planted and size >= (2 << 18) - 3000:
            ln = f'stranger\t0\tNOBODY_KNOWS_ME\t{TAIL}\n'
            planted = True
        else:
            ln = ''.join(f'read{q:07d}\t0\t{rng.choice(subjects)}\t{TAIL}\n'
                         for _ in range(rng.choice([1, 1, 2])))
        out.append(ln)
        size += len(ln)
        q += 1
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(''.join(out))
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    tables, routes = _three_routes(tmp_path, monkeypatch, **kw)
    assert routes['dtok_fused'] > 0, routes
    assert routes['dtok_fused_back'] >= 1, routes
    assert routes.get('host_block', 0) == 0, routes
    assert any(b'NOBODY_KNOWS_ME\t1\n' in t for t in tables.values())


def test_first_of_two_chained_blocks_is_handed_back(tmp_path, monkeypatch):
    """The `late_subjects` text of test_verdicts_read_one_block_late at blocks
    of 128 KB: a block is handed back with the next one's kernel queued behind
    it; the cursors return to the state in front of the first of the two (the
    ring buffer the second one's record count is taken against is the first
    one's `backup_next`, not the begin kernel's)."""
    from woltka_amd import classify as C
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 17)
    rng = random.Random(zlib.crc32(b'exit:late_subjects'))
    tax = os.path.join(ROOT, 'tests', 'golden', 'data', 'taxonomy')
    subjects = D.tax_subjects()
    indir = tmp_path / 'in'
    indir.mkdir()
    for s in ('S1', 'S2'):
        n = 30000 if s == 'S1' else 5000
        text = T._fused_sam(rng, n, subjects[:30], 'plain')
        for lo in (30, 50, 70):
            more = T._fused_sam(rng, n // 3, subjects[:lo + 20], 'plain')
            text += more.split('\n', 2)[2]
        (indir / f'{s}.sam').write_text(text)
    kw = dict(input_fp=str(indir), input_fmt='sam',
              nodes_fps=[os.path.join(tax, 'nodes.dmp')],
              map_fps=[os.path.join(tax, 'taxid.map')],
              ranks='none,phylum,genus')
    tables, routes = _three_routes(tmp_path, monkeypatch, **kw)
    assert routes['dtok_fused'] > 0, routes
    assert routes.get('dtok_lag', 0) > 0, routes
    assert routes.get('dtok_lag_back', 0) > 0, routes


def test_records_that_find_no_room(tmp_path, monkeypatch):
    """Blocks of 2 MB, read untrimmed: the sample's first blocks (1 MB the
    two-call way, then 2 MB through the one kernel) hold lines of about 1 000
    bytes, the blocks behind them 10-byte lines, a record each -- 200 k a
    block against an estimate of 2 MB x 0.001 x 1.25 + 65 536 = 68 k lines.
    On this route that estimate never sizes the streams: the first block that
    goes through the one kernel is sized before any block has shown its lines
    per byte, for block / 7 lines (the shortest mapped line) twice over
    (`words_room`), which no later block of the same size exceeds.  The
    blocks are kept and the tables are the host's; the flush that finds no
    room is reached below, with blocks of two sizes."""
    from woltka_amd import classify as C
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 21)
    monkeypatch.setattr(device_text, 'TRIM', False)
    rng = random.Random('exit:room')
    subjects = D.DENSE_SUBJECTS
    two = [s for s in subjects if len(s) == 2]
    out = [D.HEADER, D._prologue(subjects)]
    size, q = 0, 0
    while size < 3 << 20:
        ln = (f'read{q:07d}\t0\t{rng.choice(subjects)}\t1\t42\t960M\t*\t0\t0\t' +
              'ACGT' * 240 + '\t*\n')
        out.append(ln)
        size += len(ln)
        q += 1
    for i in range(260_000):     # (2.6 MB: one whole block and a rest)
        out.append(f'{QNAMES[i % 512]}\t0\t{two[i % len(two)]}\t\n')
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(''.join(out))
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    tables, routes = _three_routes(tmp_path, monkeypatch, **kw)
    print('routes', routes)
    assert routes['dtok_fused'] > 0, routes
    assert routes.get('host_block', 0) == 0, routes


QNAMES = [a + b + c for a in 'abcdefgh' for b in 'abcdefgh' for c in 'abcdefgh']


def test_flush_that_finds_no_room_hands_the_block_back():
    """kDtokSpill from `flush_all`, block by block on one context.  A block of
    70 lines of 1 000 bytes is kept and leaves 0.001 lines per byte; the next
    block -- 240 000 lines of 16 bytes, a read and a record each, 512 lines to
    an 8 KB window -- gets room for 3.84 MB x 0.001 x 1.25 + 65 536 = 70 k
    lines, twice over (`words_room`) and a quarter more (the headroom of every
    device buffer): 176 k records.  The kernel hands it back, the six kernels
    take it within the same call, and counts and cells are those of the six
    kernels alone.  The same block with room for it (the buffers have grown)
    is kept: nothing but the room made the difference."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        job, tok, names = _totals_context(ctx, nat)
        long_ = np.frombuffer(''.join(
            f'read{q:07d}\t0\t{names[q % 50]}\t1\t42\t960M\t*\t0\t0\t' +
            'ACGT' * 240 + '\t*\n' for q in range(70)).encode(), np.uint8)
        n_short = 240_000
        short = np.frombuffer(''.join(
            f'{QNAMES[i % 512]}\t0\t{names[i % 7]}\t\n'
            for i in range(n_short)).encode(), np.uint8)

        def run(fused):
            ctx.tune('dtok_fused', fused)
            assert ctx.words_begin(job, 0)
            seen = [ctx.dtok_fused_counts()]
            res = []
            for raw in (long_, short):
                status, n_lines, reads = ctx.dtok_scan_emit(tok, raw, 0,
                                                            raw.size)
                assert status == 0 and reads is not None
                res.append((n_lines, reads, ctx.words_pending()[0]))
                seen.append(ctx.dtok_fused_counts())
            ctx.words_flush()
            cells = nat.canonical_counts(*ctx.counts_fetch())
            ctx.counts_clear()
            steps = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(seen, seen[1:])]
            return res, cells, steps
        try:
            tight, cells_tight, steps = run(1)
            print('no room', tight, steps)
            assert steps == [(1, 0), (0, 1)], steps      # (kept, handed back)
            assert tight == [(70, 70, 70),
                             (n_short, n_short, 70 + n_short)]
            six, cells_six, steps = run(0)
            assert steps == [(0, 0), (0, 0)], steps
            assert six == tight
            roomy, cells_roomy, steps = run(1)
            assert steps == [(1, 0), (1, 0)], steps      # (both kept)
            assert roomy == tight
            for got in (cells_tight, cells_roomy):
                assert np.array_equal(got[0], cells_six[0]) and \
                    np.array_equal(got[1], cells_six[1])
        finally:
            ctx.tune('dtok_fused', 1)
            tok.close()
