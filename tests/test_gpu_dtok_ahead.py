"""The one-kernel SAM tokenizer (csrc/wk_dtok_fused.hpp) asks for the text of
the window that follows as soon as that window is known -- behind the
ownership chain, in front of the planes and the records -- instead of at that
window's top (`kAhead`).  The product's instance has it on; the measuring
instance decides at run time: bit 2048 of `wk_tune("fz_ablate")` = loads at
every window's top, as before.  Like bit 1024 the bit leaves nothing out, so
every case here goes three ways over the same bytes and must give the same
thing each time:

  top    the measuring instance with fz_ablate = 2048 (run first: what the
         kernel kept and handed back before the change),
  ahead  the product's instance,
  six    the six kernels.

Geometry: `dtok_fused_per_cu` = 1 and a block of 16 MB read untrimmed, so
spans of 64 KB in four windows and more (tests/test_gpu_dtok_instances.py,
tests/test_gpu_dtok_exit.py).  The cases are the smallest shapes where a
window loaded ahead can differ from one loaded at its top: where the next
window begins inside its first chunk, where it ends (the span, the text, an
open last line), whether there is one at all, where the issue point is (the
usual chain, a run put aside, a window of unmapped lines) and what lies
between the issue and the use (a mid-kernel flush of the record buffers)."""
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
import test_gpu_dtok as T  # noqa: E402  (its `_run`, `_random_sam`)
import test_gpu_dtok_exit as E  # noqa: E402  (`_per_cu`, `_spy_counts`, `_totals_context`, `TAIL`)
import test_gpu_dtok_instances as I  # noqa: E402  (`_tuned`)

BLOCK = 1 << 24
SPAN = 1 << 16          # (16 MB over the 256 workgroups of per_cu = 1)
WAYS = (('top', 1, 2048), ('ahead', 1, 0), ('six', 0, 0))
UNMAPPED = '\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n'


def _lines(rng, names, size, plant=None):
    """Mapped lines of 39 to 44 bytes (the CIGAR's digits vary: a window that
    follows another begins at every byte of a chunk), reads of 1 to 3 lines,
    nearly a record a line -- about 1 500 records per 64 KB span against the
    1 024 a slice's buffer holds, so the buffers leave mid-kernel, between
    the issue of a window's loads and their use.  `plant(q, size)`: text to
    put behind read q, or None."""
    out, n, q = [], 0, 0
    while n < size:
        for _ in range(rng.choice((1, 1, 1, 2, 3))):
            ln = (f'q{q:07d}\t0\t{rng.choice(names)}\t1\t42\t'
                  f'{rng.randrange(10 ** rng.randrange(1, 7))}M\t*\t0\t0\t*\t*\n')
            out.append(ln)
            n += len(ln)
        extra = plant(q, n) if plant else None
        if extra:
            out.append(extra)
            n += len(extra)
        q += 1
    return ''.join(out)


def _cut(text, size):
    """`text` cut behind the last line that ends at or in front of `size`."""
    return text[:text.rindex('\n', 0, size) + 1]


def _stretch(tag, size):
    """Unmapped lines, `size` bytes of them."""
    out, n, i = [], 0, 0
    while n < size:
        ln = f'u{tag}_{i // 2}{UNMAPPED}'
        out.append(ln)
        n += len(ln)
        i += 1
    return ''.join(out)


def _planted(rng, names, at):
    """_lines() with text planted where the size first passes each key of
    `at` (byte offsets of the block, ascending)."""
    todo = sorted(at.items())

    def plant(q, n):
        if todo and n >= todo[0][0]:
            return todo.pop(0)[1]
        return None
    text = _lines(rng, names, BLOCK + 4096, plant)
    assert not todo
    return text


def _case(name, names):
    rng = random.Random(f'ahead:{name}')
    if name in ('lead', 'open_end', 'short'):
        if name == 'short':         # (one span, one window: nothing follows)
            return _cut(_lines(rng, names, 4096), 3000)
        text = _cut(_lines(rng, names, BLOCK + 4096), BLOCK)
        # (`open_end`: position n ends the last line -- the last span's last
        # window, loaded ahead like the others, ends at the text's end)
        return text[:-1] if name == 'open_end' else text
    if name == 'wide':
        # Runs of 130 lines that name one subject, about 5.5 KB, one every
        # 23 KB: some forty of the 255 span ends fall into one that does not
        # end 3 KB behind the span -- whole windows ahead, past the span.
        def plant(q, n):
            if q % 550 == 0:
                s = rng.choice(names)
                return ''.join(f'long{q:07d}\t0\t{s}\t{E.TAIL}\n'
                               for _ in range(130))
            return None
        return _cut(_lines(rng, names, BLOCK + 4096, plant), BLOCK)
    if name == 'aside':
        # A mapped line and 22 KB of unmapped lines behind it: the window that
        # begins at that line sees its run's start and not its end -- the run
        # is put aside and the window behind begins at `trail`, mode 2 (the
        # other issue point).  In a span's first, second and third window
        # (2, 20 and 38 KB into spans 3, 9 and 15 -- and, whatever the spans
        # are, at every 777th KB further on), and twice in one span (21).
        at = {3 * SPAN + 2048: 0, 9 * SPAN + 20480: 0, 15 * SPAN + 38912: 0,
              21 * SPAN + 2048: 0, 21 * SPAN + 34816: 0}
        at.update({k << 10: 0 for k in range(2000, 16000, 777)})
        at = {k: _stretch(i, 22 << 10) for i, k in enumerate(sorted(at))}
        return _cut(_planted(rng, names, at), BLOCK)
    if name == 'unmapped':
        # 150 KB of unmapped lines: windows that hold nothing else, in the
        # middle of a span (behind a run put aside) and at the top of the
        # next two (no run starts: on behind the last whole line).
        at = {k: _stretch(i, 150 << 10)
              for i, k in enumerate((5 * SPAN + 30000, 40 * SPAN + 100,
                                     100 * SPAN + 60000))}
        return _cut(_planted(rng, names, at), BLOCK)
    raise KeyError(name)


def _three_ways(ctx, nat, job, tok, raw):
    res = {}
    for tag, fused, ablate in WAYS:
        ctx.tune('dtok_fused', fused)
        ctx.tune('fz_ablate', ablate)
        assert ctx.words_begin(job, 0)
        before = ctx.dtok_fused_counts()
        status, n_lines, reads = ctx.dtok_scan_emit(tok, raw, 0, raw.size)
        assert status == 0, tag
        if reads is None:
            st, reads, _ = ctx.dtok_emit()
            assert st == 0, tag
        records = ctx.words_pending()[0]
        ctx.words_flush()
        after = ctx.dtok_fused_counts()
        cells = nat.canonical_counts(*ctx.counts_fetch())
        ctx.counts_clear()
        res[tag] = ((n_lines, reads, records), cells,
                    (after[0] - before[0], after[1] - before[1]))
    return res


@pytest.mark.parametrize('name', ['lead', 'open_end', 'short', 'wide',
                                  'aside', 'unmapped'])
def test_block_three_ways(name):
    """Lines, reads, records and cells of one block, and what the kernel kept
    and handed back: the same with the loads at the top, ahead, and (but for
    the last) through the six kernels.  The plain cases are kept."""
    from woltka_amd import _native as nat
    with nat.Context(0) as ctx:
        ctx.tune('dtok_fused_per_cu', 1)
        job, tok, names = E._totals_context(ctx, nat)
        text = _case(name, names)
        raw = np.frombuffer(text.encode(), np.uint8)
        assert raw.size <= BLOCK
        try:
            res = _three_ways(ctx, nat, job, tok, raw)
        finally:
            ctx.tune('fz_ablate', 0)
            ctx.tune('dtok_fused', 1)
            tok.close()
    print(name, raw.size, {k: (v[0], v[2]) for k, v in res.items()})
    lines = text.count('\n') + (0 if text.endswith('\n') else 1)
    for tag in ('top', 'ahead', 'six'):
        assert res[tag][0] == res['top'][0], tag
        assert res[tag][0][0] == lines and res[tag][0][1] > 0, tag
        assert np.array_equal(res[tag][1][0], res['top'][1][0]) and \
            np.array_equal(res[tag][1][1], res['top'][1][1]), tag
    assert res['six'][2] == (0, 0)
    assert res['ahead'][2] == res['top'][2], 'kept / handed back'
    assert sum(res['top'][2]) == 1
    if name in ('lead', 'open_end', 'short', 'wide'):
        assert res['ahead'][2] == (1, 0)


def _files_three_ways(tmp_path, monkeypatch, **kw):
    """The same through the workflow (two samples, S1 and S2): equal tables
    and logs; the one kernel ran in both schedules and kept and handed back
    the same blocks of either sample."""
    from woltka_amd import classify as C
    from woltka_amd.hostio import ROUTES
    from woltka_amd.routes import device_text
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', BLOCK)
    monkeypatch.setattr(device_text, 'TRIM', False)
    E._per_cu(monkeypatch, 1)
    knobs = {'fz_ablate': 0}
    I._tuned(monkeypatch, knobs)
    per_file = E._spy_counts(monkeypatch)
    got, routes, counts = {}, {}, {}
    for tag, fused, ablate in WAYS:
        knobs['fz_ablate'] = ablate
        if not fused:
            monkeypatch.setenv('WOLTKA_NO_FUSED', '1')
        ROUTES.clear()
        got[tag] = T._run(tmp_path, tag, False, **kw)
        routes[tag] = dict(ROUTES)
        counts[tag] = (per_file[-2], per_file[-1])   # (behind S1, behind S2)
        if not fused:
            monkeypatch.delenv('WOLTKA_NO_FUSED')
    print('routes', routes, counts)
    assert got['top'] == got['six'], 'loads at the top'
    assert got['ahead'] == got['six'], 'loads ahead'
    assert routes['six']['dtok_fused'] == 0 and routes['six']['dtok'] > 0
    for tag in ('top', 'ahead'):
        assert routes[tag]['dtok_fused'] > 0, routes
    assert routes['ahead'].get('dtok_fused_back', 0) == \
        routes['top'].get('dtok_fused_back', 0), routes
    assert counts['ahead'] == counts['top'] and counts['top'][1][0] >= 1, counts
    return got['ahead'], routes['ahead'], counts['ahead']


def test_four_slices_flush_between_issue_and_use(tmp_path, monkeypatch):
    """A subject table of four slices and about 1 600 records per workgroup:
    `flush_all` -- its returning atomics wait for everything under way, the
    next window's text included -- runs mid-kernel for all four buffers.
    (One slice: every case of test_block_three_ways.)"""
    n_subjects = 4 * D.SLICE - 200
    rng = random.Random('ahead:slices')
    indir = tmp_path / 'in'
    indir.mkdir()
    first = D._slices(rng, n_subjects, None)
    (indir / 'S1.sam').write_text(first)
    warm = len(first) > 1 << 20
    out, size, q = [D.HEADER], 0, 0
    while size < (33 if warm else 22) << 20:
        for _ in range(rng.choice([1, 1, 1, 2, 3])):
            out.append(f'q{q:07d}\t0\tg{rng.randrange(n_subjects):06d}\t'
                       f'{E.TAIL}\n')
            size += 41
        q += 1
    (indir / 'S2.sam').write_text(''.join(out))
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    _, routes, counts = _files_three_ways(tmp_path, monkeypatch, **kw)
    # (the second sample's blocks behind its first: kept, none handed back --
    # tests/test_gpu_dtok_instances.py::test_slices_and_waves_in_front)
    s2 = [x - y for x, y in zip(counts[1], counts[0])]
    assert s2[0] >= 1 and s2[1] == 0, (routes, counts)


@pytest.mark.parametrize('how', ['trimsub', 'exclude'])
def test_subject_map(tmp_path, monkeypatch, how):
    """`--trim-sub` and `--exclude` (ids through `submap`, runs dropped whole)
    over spans of several windows: mates, unmapped lines, reads of up to 16
    subjects."""
    rng = random.Random(f'ahead:{how}')
    genomes = D.tax_subjects()[:50]
    subjects = [f'{g}_{k}' for g in genomes for k in (1, 2)] \
        if how == 'trimsub' else genomes
    indir = tmp_path / 'in'
    indir.mkdir()
    (indir / 'S1.sam').write_text(T._random_sam(
        rng, 3000, subjects, paired=True, unmapped=True, long_names=False))
    # (the reader's blocks of a sample: 1, 4, 16 MB -- the third is a whole one)
    (indir / 'S2.sam').write_text(T._random_sam(
        rng, 130_000, subjects, paired=True, unmapped=True, long_names=False))
    assert os.path.getsize(indir / 'S2.sam') > 22 << 20
    kw = dict(input_fp=str(indir), input_fmt='sam', ranks='none')
    if how == 'trimsub':
        kw['trimsub'] = '_'
    else:
        ex = tmp_path / 'excl.txt'
        ex.write_text('\n'.join(subjects[::9]) + '\n')
        kw['exclude'] = str(ex)
    _files_three_ways(tmp_path, monkeypatch, **kw)
