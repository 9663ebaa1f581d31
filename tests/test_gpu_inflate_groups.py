"""GPU: the device decoder's grouped launches (iteres_amd/csrc/itx_inflate.hip: one launch of each pass over the blocks of up
to ITX_GROUP consecutive pushes, on ITX_LANES compute lanes in turn) through itx_bamwin_push_begin / push_copied / push_end.
Both knobs are read once per process, so every setting runs tests/groupcase.py in a fresh child, one at a time; the child
compares every window's bytes with zlib and hands back the status bytes and a digest per push."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_done = {}


def run_case(scenario, group, lanes):
    """the child's result, once per (scenario, setting) and session"""
    key = (scenario, group, lanes)
    if key not in _done:
        env = dict(os.environ, ITX_GROUP=str(group), ITX_LANES=str(lanes))
        env.pop("ITX_PUSHES", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "groupcase.py"), scenario], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, f"ITX_GROUP={group} ITX_LANES={lanes} {scenario}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        assert len(line) == 1, r.stdout[-2000:]
        _done[key] = json.loads(line[0][7:])
        assert (_done[key]["group"], _done[key]["lanes"]) == (group, lanes)
    return _done[key]


GROUPED = [(2, 2), (4, 1)]


@pytest.mark.parametrize("group,lanes", GROUPED)
def test_slots_of_1_63_64_65_129_and_no_blocks(group, lanes):
    """stored, fixed and dynamic blocks; a push without blocks between the members of a group; the last group is partial"""
    res = run_case("sizes", group, lanes)
    assert [len(p["status"]) for p in res["pushes"]] == [1, 63, 0, 64, 65, 129, 129, 1]
    assert not any(any(p["status"]) for p in res["pushes"])


def test_partial_group_is_launched_by_push_end():
    """three begins with groups of four, push_copied on each before any push_end"""
    res = run_case("partial", 4, 1)
    assert [len(p["status"]) for p in res["pushes"]] == [65, 1, 64]


@pytest.mark.parametrize("group,lanes", GROUPED)
def test_damaged_block_is_flagged_in_its_slot_only(group, lanes):
    res = run_case("damaged", group, lanes)
    flagged = [(k, i) for k, p in enumerate(res["pushes"]) for i, s in enumerate(p["status"]) if s]
    assert flagged == [(2, 17)]


@pytest.mark.parametrize("group,lanes", GROUPED)
def test_scratch_reused_by_later_groups(group, lanes):
    res = run_case("reuse", group, lanes)
    assert len(res["pushes"]) == 2 * group * lanes + 1
    assert not any(any(p["status"]) for p in res["pushes"])


@pytest.mark.parametrize("scenario", ["sizes", "damaged"])
def test_groups_of_one_on_four_lanes_give_the_same(scenario):
    """ITX_GROUP=1 ITX_LANES=4 (one launch per push, as before there were groups) against groups of two on two lanes"""
    a, b = run_case(scenario, 1, 4), run_case(scenario, 2, 2)
    assert a["pushes"] == b["pushes"]
