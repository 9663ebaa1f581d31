"""GPU: pass 2 of the device decoder (itxi_resolve, iteres_amd/csrc/itx_inflate_core.h) with the 64-lane wave it is written for,
on the hand-made streams of tests/deflatecraft.py, through itx_inflate_bgzf (k_tokens + k_resolve). The host build replays with
one lane, where no step ends early, no step holds two tokens and a ballot is one bit; zlib's own streams leave to chance which
distance meets which lane. Here every small distance stands at every phase of a step, far, near and literal lanes share steps
around ITXI_NEAR and ITXI_RING, tokens end on the bitmap's and the literal stage's limits, and the fullest scratch regions lie
side by side. Expected bytes: the plain replay of the token list, which tests/test_deflatecraft.py holds equal to zlib's."""
import numpy as np
import pytest

import deflatecraft as dc
from iteres_amd import engine as eng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inf():
    h = eng.Inflater()
    yield h
    h.close()


def check(inf, items):
    """items: (label, member, expected bytes, expected status) — all in one call; every member's status, and the bytes of every
    member that is to decode"""
    comp = b"".join(m for _, m, _, _ in items)
    out, status = inf.inflate(comp)
    assert len(status) == len(items)
    out = out.tobytes()
    at = 0
    for i, (label, _, want, st) in enumerate(items):
        got = out[at:at + len(want)]
        at += len(want)
        assert status[i] == st, "member %d (%s): status %d, expected %d" % (i, label, int(status[i]), st)
        if st == 0 and got != want:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
            k = int(np.flatnonzero(a != b)[0])
            raise AssertionError("member %d (%s): first wrong byte at offset %d of %d: %d, expected %d (%d members differ)" % (
                i, label, k, len(want), int(a[k]), int(b[k]), _n_differ(out, items)))
    assert at == len(out)


def _n_differ(out, items):
    n = at = 0
    for _, _, want, st in items:
        n += st == 0 and out[at:at + len(want)] != want
        at += len(want)
    return n


def plain(family):
    return [(label, dc.member(raw, want), want, 0) for label, raw, want in family]


def test_step_grid(inf):
    """A: every distance 1 .. 70 at every phase of a step, matches that read their own step, matches of matches"""
    check(inf, plain(dc.cases("A")))


def test_near_far_and_the_ring(inf):
    """B: at output offsets 0, 1, 3 and 255 mod 256"""
    check(inf, [item + (0,) for item in dc.phased(dc.cases("B"))])


def test_batch_bitmap_and_stage_limits(inf):
    check(inf, plain(dc.cases("C")))


def test_fullest_regions_side_by_side(inf):
    """D: 65 536 literals, 21 801 tokens, 65 536 literals in adjacent scratch regions; then the token-full ones next to each other"""
    small = plain(dc.cases("C")[:3])
    d = plain(dc.cases("D"))
    check(inf, small + d + [d[1], d[1], d[0]] + small)


def test_pass_one_code_shapes(inf):
    """E: hand-made dynamic blocks between zlib's own, in the lanes of the same pass-1 waves"""
    check(inf, plain(dc.cases("E")))


def test_refusals_leave_the_neighbours_alone(inf):
    """F: a distance one byte before the block (7), a match one byte past usize (2)"""
    items = [(label, dc.member(raw, data), data, status) for label, raw, data, status in dc.cases("F")]
    assert [st for _, _, _, st in items] == [0, 7, 0, 7, 0, 2, 0]
    check(inf, items)
