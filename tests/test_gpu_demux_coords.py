"""Coord-match under demultiplexing on the device text route
(csrc/wk_demux.hpp, `_run_dhits_demux`): the kernels through the C ABI against
the per-read samples and genes, and whole commands against the tables, of
tests/golden/vectors/demux_coords_device.json -- what the reference makes of
the cases of tests/demux_coords_cases.py
(tests/golden/make_demux_coords_reference.py)."""
import contextlib
import gzip
import io
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import demux_coords_cases as T          # noqa: E402
from helpers import load_vectors        # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = load_vectors('demux_coords_device.json')
READ_CASES = {c['name']: c for c in T.read_cases()}
CLI_CASES = {c['name']: c for c in T.cli_cases()}


# ---- the kernels -------------------------------------------------------------
def _scan(ctx, tok, case):
    from woltka_amd import _native as nat
    text = np.frombuffer(case['text'].encode(), dtype=np.uint8)
    ok, begin, stop, _ = nat.Tokenizer.sam_span(text, True, True, case['fmt'])
    assert ok and stop == text.size
    status, n_lines = ctx.dtok_scan(tok, text, begin, stop, extra=True)
    assert status == 0 and n_lines >= 50
    return text


def _device_reads(case, hash_mask=0, max_samples=0, whitelist=False):
    """One block through dtok_scan ("ex" flavour), demux_pending / _register,
    dtok_stage_hits_demux and ordinal_match.  Returns (status, reads as
    (group, gene names), sample names in the table's order, met bytes)."""
    from woltka_amd import _native as nat
    allow = set(case['samples']) if (case['samples'] and whitelist) else None
    genomes, off, start0, end, genes = T.gene_tables()
    ctx, tok = nat.Context(0), nat.Tokenizer(2)
    try:
        ctx.set_option('demux_hash_mask', hash_mask)
        ctx.set_option('demux_max_samples', max_samples)
        ctx.set_genes(off, start0, end, np.arange(len(genes)))
        ctx.dtok_format(case['fmt'])
        ctx.demux_begin(True)
        _scan(ctx, tok, case)
        where = {g: i for i, g in enumerate(genomes)}
        gmap = np.asarray([where.get(x, -1) for x in tok.new_subjects()],
                          dtype=np.int32)
        status, fresh = ctx.demux_pending()
        if status != 0:
            st2, _, _ = ctx.dtok_stage_hits_demux(gmap, 0.8)
            assert st2 == 1                 # (the block is refused, status 1)
            return status, None, None, None
        samples = [x.decode() for x in fresh]
        groups = [i if (allow is None or x in allow) else -1
                  for i, x in enumerate(samples)]
        ctx.demux_register(fresh, groups)
        assert ctx.demux_pending() == (0, [])       # (all in the table now)
        status, n_reads, n_hits = ctx.dtok_stage_hits_demux(gmap, 0.8)
        assert status == 0 and n_hits >= n_reads > 0
        ctx.ordinal_match()
        subj, qoff = ctx.chunk_download()
        assert qoff.size == n_reads + 1
        met, group = ctx.demux_fetch(len(samples), n_reads)
        off, subj = qoff.tolist(), subj.tolist()
        reads = [(g, [genes[s] for s in subj[off[i]:off[i + 1]]])
                 for i, g in enumerate(group.tolist())]
        return 0, reads, samples, met
    finally:
        tok.close()
        ctx.close()


def _key(x):
    return (x[0] is None, x[0] or '', x[1])


def _labels(reads, samples):
    """What the fixture holds: the reads that matched a gene (sorted: the
    reference yields them in its matcher's order, the device in the
    text's)."""
    return sorted(([None if g < 0 else samples[g], sorted(set(genes))]
                   for g, genes in reads if genes), key=_key)


def _check(name, reads, samples, met, whitelist):
    gold = GOLD['reads'][name]
    if not whitelist:       # (the same text without its whitelist)
        gold = GOLD['reads']['sam-paired' if name == 'sam-whitelist' else name]
    assert _labels(reads, samples) == sorted(gold, key=_key)
    assert len(set(samples)) == len(samples)
    # the table holds the samples of the reads that have a hit of aligned
    # length > 0 -- not those met in unmapped lines or hits of length 0 only
    assert not {'ZERO', 'UNM'} & set(samples)
    # met: the samples a read with a group and a gene belongs to
    kept = {x[0] for x in gold} - {None}
    assert {s for s, m in zip(samples, met.tolist()) if m} == kept
    assert set(met.tolist()) <= {0, 1}


@pytest.mark.parametrize('whitelist', [False, True], ids=['all', 'whitelist'])
@pytest.mark.parametrize('name', list(READ_CASES))
def test_samples_and_genes_of_every_read(name, whitelist):
    case = READ_CASES[name]
    if whitelist and not case['samples']:
        case = dict(case, samples=['S1', 'A', 'ABSENT', 'NOGENE'])
        gold = [[x[0] if x[0] in case['samples'] else None, x[1]]
                for x in GOLD['reads'][name]]
    else:
        gold = None
    status, reads, samples, met = _device_reads(case, whitelist=whitelist)
    assert status == 0
    if gold is not None:    # (the whitelist applied to the reference's samples)
        assert _labels(reads, samples) == sorted(gold, key=_key)
        kept = {x[0] for x in gold} - {None}
        assert {s for s, m in zip(samples, met.tolist()) if m} == kept
        return
    _check(name, reads, samples, met, whitelist)
    if name.startswith('sam-') and name != 'nine-samples':
        # registered (they have hits) but never met: no gene matched
        assert {'NOGENE', 'BELOW'} <= set(samples)


@pytest.mark.parametrize('name', ['sam-paired', 'sam-whitelist',
                                  'nine-samples'])
def test_names_that_share_a_hash_are_told_apart_by_their_bytes(name):
    """`demux_hash_mask` = 3: every name has one of 4 hash values."""
    status, reads, samples, met = _device_reads(
        READ_CASES[name], hash_mask=0x3, whitelist=True)
    assert status == 0 and len(samples) > 4
    _check(name, reads, samples, met, True)


def test_more_samples_than_the_table_holds_refuse_the_block():
    status, *_ = _device_reads(READ_CASES['nine-samples'], max_samples=4)
    assert status & 1
    status, _, samples, _ = _device_reads(READ_CASES['nine-samples'],
                                          max_samples=9)
    assert status == 0 and len(samples) == 9


def test_stage_hits_wants_the_pending_samples_registered():
    from woltka_amd import _native as nat
    case = READ_CASES['nine-samples']
    genomes, off, start0, end, genes = T.gene_tables()
    ctx, tok = nat.Context(0), nat.Tokenizer(2)
    try:
        ctx.set_genes(off, start0, end, np.arange(len(genes)))
        ctx.dtok_format('sam')
        ctx.demux_begin(True)
        _scan(ctx, tok, case)
        gmap = np.zeros(len(tok.new_subjects()), dtype=np.int32)
        with pytest.raises(RuntimeError, match='samples the table does not'):
            ctx.dtok_stage_hits_demux(gmap, 0.8)
    finally:
        tok.close()
        ctx.close()


# ---- commands ----------------------------------------------------------------
def _command(case, root, text=None, **more):
    """The case through workflow.workflow; returns ({'tables', 'classified'},
    routes)."""
    from woltka_amd.hostio import ROUTES
    from woltka_amd.workflow import workflow
    ROUTES.clear()
    args = T.write_cli(case, str(root), text)
    args.update(more)
    args['output_fp'] = os.path.join(str(root), 'out')
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        workflow(**args)
    n = re.findall(r'Number of sequences classified: (\d+)\.', said.getvalue())
    return {'tables': T.digest(T.tables_of(args['output_fp'])),
            'classified': [int(x) for x in n]}, dict(ROUTES)


def _on_device(routes):
    assert routes.get('dhits_demux', 0) > 0, routes
    assert routes.get('host_block', 0) == 0, routes
    assert routes.get('text_ahead', 0) == 0, routes


@pytest.mark.parametrize('name', [c['name'] for c in T.cli_cases()
                                  if c['name'] != 'cigar'])
def test_commands_match_the_reference_on_the_device_route(tmp_path,
                                                          monkeypatch, name):
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    got, routes = _command(CLI_CASES[name], tmp_path)
    _on_device(routes)
    assert got == GOLD['cli'][name]


@pytest.mark.parametrize('name', ['orf', 'orf-sizes', 'function'])
def test_small_blocks_meet_samples_late_and_runs_at_cuts(tmp_path, monkeypatch,
                                                         name):
    from woltka_amd import classify as C
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 13)
    got, routes = _command(CLI_CASES[name], tmp_path)
    _on_device(routes)
    assert routes['dhits_demux'] >= 3, routes
    assert got == GOLD['cli'][name]


def test_gz_copy(tmp_path, monkeypatch):
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    case = CLI_CASES['orf-samples']
    args = T.write_cli(case, str(tmp_path))
    gz = str(tmp_path / 'mux.sam.gz')
    with open(args['input_fp'], 'rb') as src, gzip.open(gz, 'wb') as dst:
        dst.write(src.read())
    got, routes = _command(case, tmp_path, input_fp=gz)
    _on_device(routes)
    assert got == GOLD['cli'][case['name']]


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
    got, routes = _command(CLI_CASES['orf'], tmp_path)
    assert routes.get('dhits_demux', 0) > 0 and \
        routes.get('host_block', 0) > 0, routes
    assert got == GOLD['cli']['orf']


def test_a_cigar_the_device_hands_back_goes_through_the_host(tmp_path,
                                                             monkeypatch):
    from woltka_amd import classify as C
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 13)
    got, routes = _command(CLI_CASES['cigar'], tmp_path)
    assert routes.get('dhits_demux', 0) > 0 and \
        routes.get('host_block', 0) > 0, routes
    assert got == GOLD['cli']['cigar']


def test_switch_keeps_the_host_route_and_the_bytes(tmp_path, monkeypatch):
    monkeypatch.setenv('WOLTKA_NO_DDEMUX', '1')
    for name in ('orf', 'orf-samples'):
        got, routes = _command(CLI_CASES[name], tmp_path / name)
        assert routes.get('dhits_demux', 0) == 0, routes
        assert got == GOLD['cli'][name]


@pytest.mark.parametrize('more', ['exclude', 'stratify'])
def test_exclude_and_stratify_keep_todays_route(tmp_path, monkeypatch, more):
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    if more == 'exclude':
        fp = tmp_path / 'exclude.txt'
        fp.write_text('G000006745\n')
        kw = dict(exclude=str(fp))
    else:
        sdir = tmp_path / 'strata'
        sdir.mkdir()
        for i in range(1, 6):
            (sdir / f'S0{i}.txt').write_text('r1\tx\n')
        kw = dict(strata_dir=str(sdir))
    _, routes = _command(CLI_CASES['orf'], tmp_path / 'run', **kw)
    assert routes.get('dhits_demux', 0) == 0, routes


def test_byte_range_parts_equal_the_whole_file(tmp_path, monkeypatch):
    from woltka_amd import shard, workflow
    from woltka_amd.hostio import ROUTES
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    mux = tmp_path / 'mux.sam'
    mux.write_text(T.text_of('mux5'))
    kw = dict(demux=True, ranks=['none'], fmt='sam', exact=True)
    ROUTES.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        mapper, _ = workflow.build_mapper(T.COORDS_XZ, None, 80)
        whole = workflow.classify(mapper, [str(mux)], **kw)
        n_whole = ROUTES.get('dhits_demux', 0)
        assert n_whole >= 1, dict(ROUTES)
        parts = [workflow.classify(mapper,
                                   [shard.FilePart(str(mux), i, 3)], **kw)
                 for i in range(3)]
    assert ROUTES.get('dhits_demux', 0) >= n_whole + 3 and \
        ROUTES.get('host_block', 0) == 0, dict(ROUTES)
    assert shard.merge_profiles(parts) == whole
    assert sorted(whole['none']) == ['S01', 'S02', 'S03', 'S04', 'S05']
