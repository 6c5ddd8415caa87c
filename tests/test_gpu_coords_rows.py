"""The "ex" flavour of the device tokenizer -- `dtok_parse_kernel<true>`,
`dtok_row_ex`, `dtok_int_field`, `dtok_float_field` (csrc/wk_dtok.hpp) -- against
the reference row by row, on the hand-written rows of
tests/coords_rows_cases.py and what the reference makes of them
(tests/golden/vectors/coords_rows.json).

A block the device hands back looks like a parsed one from outside -- the host
tokenizer produces the right table either way --, so the rows go through the
direct doors: `dtok_scan` says whether the device parsed the block (status 0)
or handed it back (status 1); the cover door (`dtok_cover_append`,
`cover_fetch`) shows the start and end of every line the device parsed, the
match door (`dtok_stage_hits`, `ordinal_match`) the genes of every hit, which
the probe genes of the cases tie to start, end and length within one base
(tests/test_coords_rows_host.py shows that they do).  Every comparison is of
exact integers or bytes."""
import builtins
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import coords_rows_cases as T           # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('coords_rows.json')
CASES = {c['name']: c for c in T.cases()}


class Doors:
    """A context of its own for one format, its tokenizer, and the probe
    genes of every case of the format."""

    def __init__(self, fmt):
        from woltka_amd import _native as nat
        self.fmt = fmt
        self.ctx = nat.Context(0)
        self.tok = nat.Tokenizer(2)
        self.ctx.dtok_format(fmt)
        self.genomes, self.off, self.start0, self.end, self.names = \
            T.gene_tables(T.cases(fmt), GOLD)
        self.ctx.set_option('gene_index_pairs', 1)
        self.ctx.set_genes(self.off, self.start0, self.end,
                           np.arange(len(self.names), dtype=np.int32))
        self.subjects = []          # the tokenizer's subject ids -> names
        self.ctx.cover_begin(0)

    def close(self):
        self.tok.close()
        self.ctx.close()

    def scan(self, text):
        """(status, lines) of the text as one block of the "ex" flavour."""
        raw = np.frombuffer(text.encode(), np.uint8)
        status, n = self.ctx.dtok_scan(self.tok, raw, 0, raw.size, extra=True)
        self.subjects += self.tok.new_subjects()
        return status, n

    def ranges(self):
        """The cover door: {subject: merged [beg, end, ...]} of the block
        scanned last."""
        self.ctx.cover_reset()
        self.ctx.dtok_cover_append()
        out = {}
        for k, b, e in zip(*(x.tolist() for x in self.ctx.cover_fetch())):
            out.setdefault(self.subjects[k], []).extend((b, e))
        return out

    def _lists(self, n_hits):
        """After a match: the gene names of every hit, the reads' offsets and
        the hits' offsets into the gene lists."""
        self.ctx.ordinal_match()
        pairs, qoff = self.ctx.chunk_download()
        poff = self.ctx.ordinal_hit_offsets(n_hits)
        genes = self.ctx.ordinal_pair_genes(pairs.size)
        # (the chunk's records are the genes' features: here their indices)
        assert np.array_equal(pairs, genes)
        per_hit = [sorted(self.names[g] for g in genes[poff[h]:poff[h + 1]])
                   for h in range(n_hits)]
        return per_hit, qoff.tolist(), poff.tolist()

    def hits(self):
        """The match door on the block scanned last: (reads, hits, genes per
        hit, reads' offsets, hits' offsets)."""
        gmap = np.asarray([self.genomes.index(s) if s in self.genomes else -1
                           for s in self.subjects] or [-1], np.int32)
        status, reads, hits = self.ctx.dtok_stage_hits(gmap, 1.0)
        assert status == 0
        return (reads, hits) + self._lists(hits)

    def staged(self, expected):
        """The same calls over hits handed to `ordinal_stage`: `expected` =
        [(query, [(subject, s, e, L), ...])]."""
        flat = [h for _, hs in expected for h in hs]
        hoff = np.cumsum([0] + [len(hs) for _, hs in expected])
        self.ctx.ordinal_stage(
            [self.genomes.index(h[0]) if h[0] in self.genomes else -1
             for h in flat], [h[1] for h in flat], [h[2] for h in flat],
            [h[3] for h in flat], hoff, 1.0)
        return (len(expected), len(flat)) + self._lists(len(flat))


@pytest.fixture(scope='module', params=T.FORMATS)
def doors(request):
    d = Doors(request.param)
    yield d
    d.close()


def _expected_reads(some):
    """[(query, [(subject, s, e, L)])] of the reads with a hit of positive
    length, as the reference's matcher takes them from its parser."""
    out = []
    for c in some:
        for q, recs in GOLD['cases'][c['name']]['records']:
            hs = [(s, b, e, ln) for s, ln, b, e in recs if ln > 0]
            if hs:
                out.append((q, hs))
    return out


def _expected_ranges(some):
    out = {}
    for c in some:
        out.update(GOLD['cases'][c['name']]['ranges'])
    return out


def _expected_genes(some):
    return {q: g for c in some for q, g in GOLD['cases'][c['name']]['genes']}


def test_all_stay_rows_in_one_block_are_parsed_like_the_reference(doors):
    some = T.cases(doors.fmt, T.STAY)
    text = T.block_of(some)
    status, n = doors.scan(text)
    assert (status, n) == (0, text.count('\n'))
    # the cover door: every mapped line, those of length 0 too
    want = _expected_ranges(some)
    assert len(want) >= 8
    assert doors.ranges() == want
    # the match door: reads, hits, and the genes of every hit in order
    reads = _expected_reads(some)
    n_hits = sum(len(hs) for _, hs in reads)
    got = doors.hits()
    assert got[:2] == (len(reads), n_hits)
    firsts = np.cumsum([0] + [len(hs) for _, hs in reads]).tolist()
    assert got[3] == [got[4][h] for h in firsts]   # a read begins at its first hit
    genes = _expected_genes(some)
    assert len(genes) >= 7
    for (q, _), lo, hi in zip(reads, firsts, firsts[1:]):
        assert sorted({g for h in range(lo, hi) for g in got[2][h]}) == \
            genes.get(q, []), q
    # the same hits handed over by the host: the same lists, hit by hit
    assert doors.staged(reads) == got


def _good_block(doors, tag):
    """A block of three good rows: parsed, and matched as usual."""
    text = ''.join(T.good(doors.fmt, f'{tag}-g{i}') + '\n' for i in range(3))
    assert doors.scan(text) == (0, 3)
    assert doors.ranges() == {T.GOOD_SUBJECT: list(T.GOOD_GENE)}
    assert doors.hits() == (3, 3, [[f'{T.GOOD_SUBJECT}_g']] * 3,
                            [0, 1, 2, 3], [0, 1, 2, 3])


def test_the_rows_handed_back_are_the_rows_the_cases_name(doors):
    """Every row in a block of its own between good rows.  A `back` or `wide`
    row: status 1, and the flag does not stick -- a good block scanned next is
    parsed.  A `stay` row: status 0.  A row found on the other side is a
    finding about the kernel or about its documented grammar, not a reason to
    move it."""
    back = set()
    for case in T.cases(doors.fmt):
        status, _ = doors.scan(T.around(case))
        assert status in (0, 1)
        if status == 1:
            back.add(case['name'])
            _good_block(doors, case['query'])
        else:
            # between its good rows, a row the device parses alone: the
            # reference's numbers once more
            want = dict(_expected_ranges([case]),
                        **{T.GOOD_SUBJECT: list(T.GOOD_GENE)})
            assert doors.ranges() == want, case['name']
    named = {c['name'] for c in T.cases(doors.fmt) if c['cls'] != T.STAY}
    assert back == named, (sorted(back - named), sorted(named - back))
    assert len(named) >= 9


# ---- the commands ----------------------------------------------------------------
def _command(tmp, fmt, text, rows=None, host=False, tag='d'):
    """workflow over one file S1.<fmt>: `rows` (cases) given: `--coords` over
    their probe genes at overlap 100; else the plain classification with
    `--outcov`.  Returns (table, classified, routes, cov)."""
    from woltka_amd import workflow
    from woltka_amd.hostio import ROUTES
    indir = tmp / f'in_{tag}'
    indir.mkdir()
    (indir / f'S1.{fmt}').write_bytes(text.encode())
    kw = dict(input_fp=str(indir), input_fmt=fmt,
              output_fp=str(tmp / f'out_{tag}.tsv'))
    if rows is not None:
        (tmp / f'coords_{tag}.txt').write_text(
            T.coords_text(rows, GOLD, command=True))
        kw.update(coords_fp=str(tmp / f'coords_{tag}.txt'), overlap=100)
    else:
        kw.update(outcov_dir=str(tmp / f'cov_{tag}'))
    os.environ.pop('WOLTKA_NO_DTOK', None)
    if host:
        os.environ['WOLTKA_NO_DTOK'] = '1'
    ROUTES.clear()
    try:
        with contextlib.redirect_stdout(io.StringIO()) as log:
            workflow.workflow(**kw)
    finally:
        os.environ.pop('WOLTKA_NO_DTOK', None)
    cov = None if rows is not None else {
        fn: (tmp / f'cov_{tag}' / fn).read_text()
        for fn in sorted(os.listdir(tmp / f'cov_{tag}'))}
    return ((tmp / f'out_{tag}.tsv').read_text(),
            [int(x) for x in re.findall(
                r'Number of sequences classified: (\d+)\.', log.getvalue())],
            dict(ROUTES), cov)


@pytest.fixture
def small_blocks(monkeypatch):
    from woltka_amd import classify as C
    monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 12)
    monkeypatch.delenv('WOLTKA_NO_DCOVER', raising=False)


@pytest.mark.parametrize('fmt', T.FORMATS)
def test_the_command_level_file_on_the_device_route(tmp_path, small_blocks,
                                                    fmt):
    gold = GOLD['cli'][fmt]
    rows = [CASES[n] for n in gold['rows']]
    text = T.cli_text(rows)
    # `--coords`: blocks of good rows staged on the device, the blocks with a
    # row the device hands back through the host tokenizer
    table, said, routes, _ = _command(tmp_path, fmt, text, rows)
    assert (table, said) == (gold['coords']['table'],
                             gold['coords']['classified'])
    assert routes.get('dhits', 0) > 0 and routes.get('host_block', 0) > 0, \
        routes
    # ... and with the stay rows alone nothing is handed back
    stay = [c for c in rows if c['cls'] == T.STAY]
    table, said, routes, _ = _command(tmp_path, fmt, T.cli_text(stay), stay,
                                      tag='s')
    assert routes.get('dhits', 0) > 0 and routes.get('host_block', 0) == 0, \
        routes
    assert (table, said) == _command(tmp_path, fmt, T.cli_text(stay), stay,
                                     host=True, tag='sh')[:2]
    # `--outcov`
    table, said, routes, cov = _command(tmp_path, fmt, text, tag='c')
    assert (table, said, cov) == (gold['outcov']['table'],
                                  gold['outcov']['classified'],
                                  gold['outcov']['cov'])
    assert routes.get('dcover', 0) > 0 and routes.get('host_block', 0) > 0, \
        routes
    routes = _command(tmp_path, fmt, T.cli_text(stay), tag='cs')[2]
    assert routes.get('dcover', 0) > 0 and routes.get('host_block', 0) == 0, \
        routes


@pytest.mark.parametrize('fmt', T.FORMATS)
def test_rows_the_reference_s_command_raises_on_raise_the_same(tmp_path,
                                                               small_blocks,
                                                               fmt):
    """Each such row alone in the middle of good rows, on the device route
    and with the device tokenizer switched off.  (Not the wide rows: there
    this package raises "32 bits" by contract where the reference carries a
    Python int -- tests/test_coords_rows_host.py.)  The rows with a negative
    length are among them (coords_rows_cases.FINDING): OverflowError under
    `--coords`, like the reference's matcher; accepted under `--outcov`,
    where nobody reads the length, with the reference's range."""
    n = 0
    for case in T.cases(fmt):
        gold = GOLD['raises'][case['name']]
        if case['cls'] == T.WIDE or gold['coords'] is None:
            continue
        text = T.around(case, k=5)
        for host in (False, True):
            tag = f'{case["query"]}{"h" if host else "d"}'
            with pytest.raises(getattr(builtins, gold['coords'])) as info:
                _command(tmp_path, fmt, text, [case], host=host, tag=tag)
            assert info.type.__name__ == gold['coords'], case['name']
            if gold['outcov'] is not None:
                with pytest.raises(getattr(builtins, gold['outcov'])) as info:
                    _command(tmp_path, fmt, text, host=host, tag=tag + 'c')
                assert info.type.__name__ == gold['outcov'], case['name']
            else:
                assert case['finding']
                cov = _command(tmp_path, fmt, text, host=host,
                               tag=tag + 'c')[3]['S1.cov']
                got = [x.split('\t')[1:] for x in cov.splitlines()
                       if x.startswith(case['subject'] + '\t')]
                assert [int(v) for x in got for v in x] == \
                    GOLD['cases'][case['name']]['ranges'][case['subject']]
        n += 1
    assert n >= 1
