"""`woltka classify --rank none,genus` on three samples that name 1 310 000
distinct subjects: more than the 1 299 456 the team layout of the weighted
histogram takes, so the second and the third sample's flushes go through the
wide layout (csrc/wk_weigh_wide.hpp).  Before that layout the command ended with
ValueError, "subject table too large for the weighted histogram".

The tables are held against what the reference wrote for the same bytes
(tests/golden/vectors/wide_subjects.json, made by
tests/golden/make_wide_reference.py from the input of tests/wide_cases.py):
sha256, row count, first and last ten rows of every table -- once from
simple-map text and once from the same records as SAM lines in blocks of
1 MB: the third sample names known subjects only, so the one-kernel tokenizer
keeps its later blocks and feeds the unsliced stream."""
import pytest

import wide_cases as W
from helpers import load_vectors

pytestmark = pytest.mark.gpu

GOLD = load_vectors('wide_subjects.json')


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return tmp_path_factory.mktemp('wide')


@pytest.mark.parametrize('fmt', ['map', 'sam'])
def test_wide_table_against_the_reference(root, fmt, monkeypatch):
    from click.testing import CliRunner
    from woltka_amd import classify as C
    from woltka_amd.cli import cli
    from woltka_amd.hostio import ROUTES
    if fmt == 'sam':
        # About 30 blocks per file.  A block that brings unknown subjects is
        # handed back by the one kernel, and after two such blocks in a row the
        # kernel is left out for 2, 4, ... 32 blocks: over the first two files
        # that comes to six blocks handed back and some ten blocks still to
        # sit out when the third file starts, so the kernel is back for the
        # second half of that file, whose subjects are all known.
        monkeypatch.setattr(C.Engine, 'DTOK_BLOCK', 1 << 20)
    assert GOLD['seed'] == W.SEED and GOLD['args'] == W.ARGS
    assert GOLD['n_subjects'] == W.N_SUBJECTS > 32 * 40608
    args = W.write_inputs(str(root), fmt)
    out = str(root / ('out_' + fmt))
    ROUTES.clear()
    res = CliRunner().invoke(cli, ['classify'] + args + ['--output', out])
    assert res.exit_code == 0, res.output + repr(res.exception)
    routes = dict(ROUTES)
    print(fmt, routes)
    got = W.digests(out)
    assert sorted(got) == sorted(GOLD['tables'])
    for fn, want in GOLD['tables'].items():
        assert got[fn]['rows'] == want['rows'], fn
        assert got[fn]['head'] == want['head'], fn
        assert got[fn]['tail'] == want['tail'], fn
        assert got[fn]['sha256'] == want['sha256'], fn
    # (cells that round to 0 -- a subject named only in reads of many hits -- are
    # not written: fewer rows than subjects)
    assert got['none.tsv']['rows'] > W.N_SUBJECTS // 2
    # the device text route took the blocks
    assert routes.get('dtok', 0) > 0, routes
    if fmt == 'sam':
        assert routes.get('dtok_fused', 0) > 0, routes
