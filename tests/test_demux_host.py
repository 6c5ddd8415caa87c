"""Demultiplexing on the device text route (csrc/wk_demux.hpp), the parts that
need no GPU: when the route is chosen (`classify.demux_on_device`), and the
host tokenizer -- the route's fallback -- against the per-read samples of
tests/golden/vectors/demux_device.json (made by
tests/golden/make_demux_reference.py from the reference's
workflow.demultiplex), so that the fixture and the fallback agree before any
device run."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import demux_cases as T                 # noqa: E402
from helpers import load_vectors        # noqa: E402

GOLD = load_vectors('demux_device.json')


def test_the_route_is_chosen_for_plain_demultiplexing_only(monkeypatch):
    from woltka_amd import _native as nat
    from woltka_amd.classify import demux_on_device
    monkeypatch.delenv('WOLTKA_NO_DDEMUX', raising=False)
    monkeypatch.delenv('WOLTKA_NO_DTOK', raising=False)
    for fmt in ('sam', 'b6o', 'paf', 'map'):
        for n_jobs in range(1, nat.MAX_JOBS + 1):
            assert demux_on_device(True, fmt, n_jobs=n_jobs)
    # every flag that keeps today's route, alone and together
    for native, coords, sizes, replay in itertools.product((True, False),
                                                           repeat=4):
        want = native and not coords and not sizes and not replay
        assert demux_on_device(native, 'sam', coords=coords, sizes=sizes,
                               n_jobs=3, replay=replay) is want
    assert not demux_on_device(True, 'sam', n_jobs=nat.MAX_JOBS + 1)
    assert not demux_on_device(True, 'sam', n_jobs=0)
    for fmt in ('b6', 'cent', 'unknown', None):
        assert not demux_on_device(True, fmt)
    for switch in ('WOLTKA_NO_DDEMUX', 'WOLTKA_NO_DTOK'):
        monkeypatch.setenv(switch, '1')
        assert not demux_on_device(True, 'sam')
        monkeypatch.delenv(switch)
    assert demux_on_device(True, 'sam')


def test_the_cases_hold_the_shapes_they_promise():
    reads = {c['name']: GOLD['reads'][c['name']] for c in T.read_cases()}
    flat, pair = reads['sam-unpaired'], reads['sam-paired']
    for got in (flat, pair):
        samples = {x[0] for x in got}
        assert {'', 'S1', 'S10', 'S1x', 'ninebytes', T.LONG} <= samples
        assert 'UNM' not in samples         # met in unmapped reads only
        assert max(len(x[1]) for x in got) == 17
    # an id that ends in its first '_': '' unpaired, its left part as a mate
    assert 'Q0' not in {x[0] for x in flat} and 'Q0' in {x[0] for x in pair}
    assert 'EXC' in {x[0] for x in pair}
    assert 'EXC' not in {x[0] for x in reads['sam-exclude']}
    assert {x[0] for x in reads['sam-whitelist']} == {
        None, 'S1', 'ninebytes', 'S3'}
    assert len({x[0] for x in reads['nine-samples']}) == 9
    assert reads['b6o'] == reads['paf'] == reads['map']


@pytest.mark.parametrize('case', T.read_cases(), ids=lambda c: c['name'])
def test_host_tokenizer_tells_the_samples_like_the_reference(case):
    from woltka_amd import _native as nat
    tok = nat.Tokenizer(2, set(case['exclude']) if case['exclude'] else None)
    try:
        text = case['text'].encode()
        res = tok.parse(text, first=True, final=True, fmt=case['fmt'],
                        want_samples=True)
        assert res['consumed'] == len(text)
        names, samples = tok.new_subjects(), tok.new_samples()
    finally:
        tok.close()
    off = res['off'].tolist()
    subj = res['subj'].tolist()
    reads = [(sid, [names[s] for s in subj[off[i]:off[i + 1]]])
             for i, sid in enumerate(res['sample'].tolist())]
    allow = set(case['samples']) if case['samples'] else None
    assert T.label_reads(reads, samples, allow) == GOLD['reads'][case['name']]
    # (samples in order of their first read, as the device route registers them)
    first = list(dict.fromkeys(samples[sid] for sid, _ in reads))
    assert samples == first
    assert np.all(np.diff(res['off']) > 0)
