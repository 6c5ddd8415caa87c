"""Demultiplexing on the device text route (csrc/wk_demux.hpp): the kernels
through the C ABI against the per-read samples, and whole commands against the
tables, of tests/golden/vectors/demux_device.json -- what the reference makes
of the cases of tests/demux_cases.py (tests/golden/make_demux_reference.py)."""
import contextlib
import gzip
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import demux_cases as T                 # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('demux_device.json')
READ_CASES = {c['name']: c for c in T.read_cases()}
CLI_CASES = {c['name']: c for c in T.cli_cases()}
_TEXTS = {}


def _text(kind):
    if kind not in _TEXTS:
        _TEXTS[kind] = T.mux5_text() if kind == 'mux5' else T.trimsub_text()
    return _TEXTS[kind]


# ---- the kernels -------------------------------------------------------------
def _device_reads(case, hash_mask=0, max_samples=0):
    """One block through dtok_scan, demux_pending / _register and
    dtok_stage_reads.  Returns (status of the lookup, reads as (sample slot
    or -1, subject names), sample names in the table's order, met bytes,
    groups)."""
    from woltka_amd import _native as nat
    excl = set(case['exclude']) if case['exclude'] else None
    allow = set(case['samples']) if case['samples'] else None
    ctx, tok = nat.Context(0), nat.Tokenizer(2, excl)
    try:
        ctx.set_option('demux_hash_mask', hash_mask)
        ctx.set_option('demux_max_samples', max_samples)
        ctx.dtok_format(case['fmt'])
        ctx.demux_begin(True)
        if excl:        # (a subject map is coming)
            ctx.dtok_subject_map(np.empty(0, dtype=np.int32))
        text = np.frombuffer(case['text'].encode(), dtype=np.uint8)
        ok, begin, stop, _ = nat.Tokenizer.sam_span(text, True, True,
                                                    case['fmt'])
        assert ok and stop == text.size
        status, n_lines = ctx.dtok_scan(tok, text, begin, stop)
        assert status == 0 and n_lines > 50
        names = tok.new_subjects()
        subjects = names
        if excl:
            subjects = [x for x in names if x not in excl]
            where = {x: i for i, x in enumerate(subjects)}
            ctx.dtok_subject_map(np.asarray(
                [where.get(x, -4) for x in names], dtype=np.int32))
        status, fresh = ctx.demux_pending()
        if status != 0:
            return status, None, None, None, None
        samples = [x.decode() for x in fresh]
        groups = [i if (allow is None or x in allow) else -1
                  for i, x in enumerate(samples)]
        ctx.demux_register(fresh, groups)
        assert ctx.demux_pending() == (0, [])       # (all in the table now)
        status, n_reads, n_records = ctx.dtok_stage_reads()
        assert status == 0
        subj, qoff = ctx.chunk_download()
        assert qoff.size == n_reads + 1 and subj.size == n_records
        met, group = ctx.demux_fetch(len(samples), n_reads)
        off, subj = qoff.tolist(), subj.tolist()
        reads = [(g, [subjects[s] for s in subj[off[i]:off[i + 1]]])
                 for i, g in enumerate(group.tolist())]
        return 0, reads, samples, met, group
    finally:
        tok.close()
        ctx.close()


def _labels(reads, samples):
    return [[None if g < 0 else samples[g], sorted(subs)] for g, subs in reads]


@pytest.mark.parametrize('name', [c['name'] for c in T.read_cases()])
def test_samples_and_subjects_of_every_read(name):
    case = READ_CASES[name]
    status, reads, samples, met, _ = _device_reads(case)
    assert status == 0
    assert _labels(reads, samples) == GOLD['reads'][name]
    # a read's subjects are a set
    assert all(len(set(subs)) == len(subs) for _, subs in reads)
    # the samples in order of the first read that brought them (the text's
    # samples: those of the same text without a whitelist)
    plain = GOLD['reads']['sam-paired' if name == 'sam-whitelist' else name]
    assert samples == list(dict.fromkeys(x[0] for x in plain))
    assert len(set(samples)) == len(samples)
    # met: the samples that a read with a group belongs to
    kept = {x[0] for x in GOLD['reads'][name]} - {None}
    assert {s for s, m in zip(samples, met.tolist()) if m} == kept
    assert set(met.tolist()) <= {0, 1}


def test_whitelist_drops_groups_and_met_flags():
    case = READ_CASES['sam-whitelist']
    _, reads, samples, met, group = _device_reads(case)
    allow = set(case['samples'])
    assert (group < 0).sum() == sum(x[0] is None
                                    for x in GOLD['reads']['sam-whitelist'])
    for s, m in zip(samples, met.tolist()):
        assert bool(m) == (s in allow), s
    assert set(samples) - allow         # (dropped samples are in the table)


@pytest.mark.parametrize('name', ['sam-paired', 'sam-exclude', 'nine-samples'])
def test_names_that_share_a_hash_are_told_apart_by_their_bytes(name):
    """`demux_hash_mask` = 3: every name has one of 4 hash values."""
    status, reads, samples, met, _ = _device_reads(READ_CASES[name],
                                                   hash_mask=0x3)
    assert status == 0 and len(samples) > 4
    assert _labels(reads, samples) == GOLD['reads'][name]
    assert samples == list(dict.fromkeys(x[0] for x in GOLD['reads'][name]))


def test_more_samples_than_the_table_holds_refuse_the_block():
    status, *_ = _device_reads(READ_CASES['nine-samples'], max_samples=4)
    assert status & 1
    status, reads, samples, _, _ = _device_reads(READ_CASES['nine-samples'],
                                                 max_samples=9)
    assert status == 0 and len(samples) == 9


def test_stage_reads_wants_the_pending_samples_registered():
    from woltka_amd import _native as nat
    case = READ_CASES['nine-samples']
    ctx, tok = nat.Context(0), nat.Tokenizer(2)
    try:
        ctx.dtok_format('sam')
        text = np.frombuffer(case['text'].encode(), dtype=np.uint8)
        _, begin, stop, _ = nat.Tokenizer.sam_span(text, True, True, 'sam')
        with pytest.raises(RuntimeError):   # (wk_demux_begin first)
            ctx.demux_pending()
        ctx.demux_begin(True)
        assert ctx.dtok_scan(tok, text, begin, stop)[0] == 0
        with pytest.raises(RuntimeError):
            ctx.dtok_stage_reads()
    finally:
        tok.close()
        ctx.close()


# ---- commands ----------------------------------------------------------------
def _command(case, root, **more):
    """The case through workflow.workflow; returns (digest of its tables,
    routes)."""
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    ROUTES.clear()
    got = T.run_cli(workflow, case, str(root), _text(case['text']), **more)
    return got, dict(ROUTES)


def _on_device(routes):
    assert routes.get('ddemux', 0) > 0, routes
    assert routes.get('host_block', 0) == 0, routes
    assert routes.get('text_ahead', 0) == 0, routes


@pytest.mark.parametrize('name', [c['name'] for c in T.cli_cases()])
def test_commands_match_the_reference_on_the_device_route(tmp_path,
                                                          monkeypatch, name):
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    got, routes = _command(CLI_CASES[name], tmp_path)
    _on_device(routes)
    assert got == GOLD['cli'][name]


@pytest.mark.parametrize('name', ['ranks3', 'exclude', 'trimsub'])
def test_small_blocks_meet_samples_late_and_runs_at_cuts(tmp_path, monkeypatch,
                                                         name):
    from woltka_amd import classify as C
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 13)
    got, routes = _command(CLI_CASES[name], tmp_path)
    _on_device(routes)
    # (the smallest text, ~36 KB of trimmed SAM, is several 8 KB blocks)
    assert routes['ddemux'] >= 3, routes
    assert got == GOLD['cli'][name]


def test_gz_copy(tmp_path, monkeypatch):
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    case = CLI_CASES['ranks3-samples']
    args = T.write_cli(case, str(tmp_path), _text('mux5'))
    gz = str(tmp_path / 'mux.sam.gz')
    with open(args['input_fp'], 'rb') as src, gzip.open(gz, 'wb') as dst:
        dst.write(src.read())
    got, routes = _command(case, tmp_path, input_fp=gz)
    _on_device(routes)
    assert got == GOLD['cli'][case['name']]


def test_switch_keeps_the_host_route_and_the_bytes(tmp_path, monkeypatch):
    monkeypatch.setenv('WOLTKA_NO_DDEMUX', '1')
    for name in ('ranks3', 'ranks3-samples'):
        got, routes = _command(CLI_CASES[name], tmp_path / name)
        assert routes.get('ddemux', 0) == 0, routes
        assert got == GOLD['cli'][name]


def test_a_full_table_leaves_the_file_to_the_host(tmp_path, monkeypatch):
    """`demux_max_samples` = 4 on the five-sample file: the block that brings
    the fifth sample is refused and the rest of the file stays on the host
    route; the tables are the same."""
    from woltka_amd import _native as nat
    from woltka_amd import classify as C
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 13)
    begin = nat.Context.demux_begin

    def small_table(self, on=True):
        self.set_option('demux_max_samples', 4)
        return begin(self, on)
    monkeypatch.setattr(nat.Context, 'demux_begin', small_table)
    got, routes = _command(CLI_CASES['ranks3'], tmp_path)
    assert routes.get('ddemux', 0) > 0 and routes.get('host_block', 0) > 1, \
        routes
    assert got == GOLD['cli']['ranks3']


@pytest.mark.parametrize('more', [dict(outcov_dir='cov'),
                                  dict(sizes='$TAX/length.map')],
                         ids=['outcov', 'sizes'])
def test_outcov_and_sizes_keep_todays_route(tmp_path, monkeypatch, more):
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    more = {k: (os.path.join(T.SC.TAX, v[5:]) if v.startswith('$TAX/')
                else str(tmp_path / v)) for k, v in more.items()}
    _, routes = _command(CLI_CASES['ranks3-samples'], tmp_path / 'run', **more)
    assert routes.get('ddemux', 0) == 0, routes


def test_byte_range_parts_equal_the_whole_file(tmp_path, monkeypatch):
    from woltka_amd import align, shard, workflow
    from woltka_amd.hostio import ROUTES
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    mux = tmp_path / 'mux.sam'
    mux.write_text(_text('mux5'))
    kw = dict(demux=True, ranks=['none'], fmt='sam', exact=True)
    ROUTES.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        whole = workflow.classify(align.plain_mapper, [str(mux)], **kw)
        n_whole = ROUTES.get('ddemux', 0)
        assert n_whole >= 1, dict(ROUTES)
        parts = [workflow.classify(align.plain_mapper,
                                   [shard.FilePart(str(mux), i, 3)], **kw)
                 for i in range(3)]
    assert ROUTES.get('ddemux', 0) >= n_whole + 3 and \
        ROUTES.get('host_block', 0) == 0, dict(ROUTES)
    assert shard.merge_profiles(parts) == whole
    assert sorted(whole['none']) == ['S01', 'S02', 'S03', 'S04', 'S05']
