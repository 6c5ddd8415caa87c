"""The inflate kernel (`csrc/wk_dinflate.hpp`) through its direct door,
`wk_inflate_members_device`: all members of a chain in one launch.

The chains are those of `tests/dinflate_cases.py`, which the host program of
`test_dinflate_core_host.py` has been through under AddressSanitizer: what
zlib writes (stored, fixed, dynamic at levels 1 / 6 / 9, several blocks, empty
and one-byte members, a run of one byte, a full BGZF member, a 'WK' member of
1 MB with matches 32 000 back, 300 members of 1 byte and 60 KB in turn) and
streams assembled bit by bit (distance 32 768 = all that was written, codes of
15 bits, one and no distance code, 5 and 13 extra bits).  The expected bytes
are zlib's.  A damaged member between two good ones has its status pinned,
leaves its neighbours' bytes alone, and the entry point itself checks the
guard bytes around the text on the device."""
import numpy as np
import pytest

import dinflate_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from woltka_amd import _native as nat
    with nat.Context(0) as c:
        yield c


GOOD = dc.good_cases()
DAMAGED = dc.damage_cases()


def run(ctx, case):
    name, blob, lo, hi, off, want, status = case
    got, st = ctx.inflate_members_device(blob, lo, hi, off)
    assert got.size == off[-1]
    return got.tobytes(), st.tolist(), want, status, off


@pytest.mark.parametrize('case', GOOD, ids=[c[0] for c in GOOD])
def test_members_inflate_to_what_zlib_gives(ctx, case):
    got, st, want, status, _ = run(ctx, case)
    assert st == status == [0] * len(st)
    assert got == want


@pytest.mark.parametrize('case', DAMAGED, ids=[c[0] for c in DAMAGED])
def test_a_damaged_member_has_a_status_and_harms_nothing(ctx, case):
    got, st, want, status, off = run(ctx, case)
    print(case[0], 'status', st)
    assert st[0] == 0 and st[2] == 0
    assert st[1] != 0 if status[1] == dc.ANY else st[1] == status[1]
    assert got[off[0]:off[1]] == want[off[0]:off[1]]
    assert got[off[2]:off[3]] == want[off[2]:off[3]]


def test_spans_outside_the_bytes_given_are_refused(ctx):
    name, blob, lo, hi, off, want, status = GOOD[0]
    with pytest.raises((ValueError, RuntimeError)):
        ctx.inflate_members_device(blob, lo, [len(blob) + 1], off)
    with pytest.raises((ValueError, RuntimeError)):
        ctx.inflate_members_device(blob, [hi[0] - 4], hi, off)
