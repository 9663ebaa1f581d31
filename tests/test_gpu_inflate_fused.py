"""GPU: the device decoder's fused launches (iteres_amd/csrc/itx_inflate.hip, k_decode: pass 1 of a group of pushes beside pass 2
of the group before it, a group's pass 2 flushed alone where no later group follows) through itx_bamwin_push_begin / push_copied /
push_end on up to 12 slots. ITX_FUSE is read once per process, so every case runs tests/fusedcase.py in a fresh child, one at a
time; the child compares every window's bytes with zlib and hands back the status bytes and a digest per push, and its ITX_TIMING
line says how many launches and flushes there were."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 129, 0)
_done = {}


def run_case(scenario, fuse=1):
    """the child's result, once per (scenario, ITX_FUSE) and session; ["launches"] / ["flushes"]: what its timing line counted"""
    key = (scenario, fuse)
    if key not in _done:
        env = dict(os.environ, ITX_FUSE=str(fuse), ITX_GROUP="4", ITX_LANES="1", ITX_TIMING="1")
        env.pop("ITX_PUSHES", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fusedcase.py"), scenario], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, f"ITX_FUSE={fuse} {scenario}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        assert len(line) == 1, r.stdout[-2000:]
        res = json.loads(line[0][7:])
        assert res["fuse"] == str(fuse)
        m = re.search(r"device decoder: (\d+) pushes in (\d+) fused launches .* (\d+) flush launches", r.stderr)
        if fuse:
            assert m, r.stderr[-2000:]
            res["launches"], res["flushes"] = int(m.group(2)), int(m.group(3))
        else:
            assert not m and re.search(r"device decoder: \d+ pushes in \d+ launches", r.stderr), r.stderr[-2000:]
        _done[key] = res
    return _done[key]


def clean(res):
    return not any(any(p["status"]) for p in res["pushes"])


@pytest.mark.parametrize("slots", [1, 2, 4])
def test_one_group_is_flushed(slots):
    res = run_case(f"flush{slots}")
    assert [len(p["status"]) for p in res["pushes"]] == [65, 129, 1, 64][:slots] and clean(res)
    assert (res["launches"], res["flushes"]) == (1, 1)


@pytest.mark.parametrize("groups", [2, 3, 5])
def test_groups_back_to_back(groups):
    """slots of 1, 63, 64, 65, 129 and 0 blocks; the last group has three members; every group but the last gets its pass 2 from
    the launch behind it"""
    res = run_case(f"groups{groups}")
    sizes = [len(p["status"]) for p in res["pushes"]]
    assert sizes == [SIZES[k % 6] for k in range(len(sizes))] and sum(1 for n in sizes if n) == 4 * groups - 1 and clean(res)
    assert (res["launches"], res["flushes"]) == (groups, 1)


def test_newest_push_ended_first():
    """the open group is launched short and flushed at once; the two groups before it got their pass 2 on the way"""
    res = run_case("newest_first")
    assert [len(p["status"]) for p in res["pushes"]] == [64, 1, 129, 63, 65, 65, 2, 130, 64, 33] and clean(res)
    assert (res["launches"], res["flushes"]) == (3, 1)


def test_all_twelve_slots_in_flight():
    res = run_case("all12")
    assert [len(p["status"]) for p in res["pushes"]] == [SIZES[k % 5] for k in range(12)] and clean(res)
    assert (res["launches"], res["flushes"]) == (3, 1)


def test_damaged_blocks_are_flagged_a_launch_later_in_their_slots_only():
    """block type 3 (status 3) and a match that reaches before its block (status 7), both in the second of three groups"""
    res = run_case("damaged")
    flagged = [(k, i, s) for k, p in enumerate(res["pushes"]) for i, s in enumerate(p["status"]) if s]
    assert flagged == [(5, 17, 3), (6, 5, 7)]
    assert (res["launches"], res["flushes"]) == (3, 1)


@pytest.mark.parametrize("scenario", ["groups5", "damaged", "newest_first"])
def test_two_kernels_give_the_same(scenario):
    """ITX_FUSE=0, k_tokens and k_resolve one behind the other as before, against the fused launches: windows and status"""
    a, b = run_case(scenario, 0), run_case(scenario, 1)
    assert a["pushes"] == b["pushes"] and len(a["pushes"]) > 0


def test_hand_made_streams_through_both_launches():
    """tests/deflatecraft.py's families B, C and D (near/far around the ring's limits, the bitmap's and the stage's limits, the fullest
    scratch regions side by side and across two pushes) in pushes of 64, 65 and 3 blocks: the child holds every block equal to zlib's
    bytes; the fused launches, where four replaying waves share one LDS block, and the two kernels give the same"""
    a, b = run_case("crafted", 0), run_case("crafted", 1)
    sizes = [len(p["status"]) for p in b["pushes"]]
    assert sizes[:3] == [64, 65, 3] and sizes[-4:] == [64, 65, 3, 64] and sum(sizes) > 200 and clean(a) and clean(b)
    assert a["pushes"] == b["pushes"]
