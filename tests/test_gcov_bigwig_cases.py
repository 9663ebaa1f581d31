"""CPU: what the GPU tests of `filter -W` rest on (tests/test_gpu_gcov_bigwig.py). The recorded digests of
tests/golden/gcov_bigwig/ are what the model gives, and what the reference's converter gives wherever oracle/_ref/libcuskent.a
exists; and every case of tests/gcovbwcases.py has the property it is named for, read off the model's first-level summaries."""
import struct

import numpy as np
import pytest

import bwsparse as bs
import gcovbwcases as cases


@pytest.fixture(scope="module")
def everything():
    return cases.all_cases()


def first_level(m, cid=None):
    red, recs = m["zooms"][0]
    v = [struct.unpack_from("<IIIIffff", recs, k) for k in range(0, len(recs), 32)]
    return red, [r for r in v if cid is None or r[0] == cid]


def test_recorded_digests_are_the_models(everything):
    rec = bs.recorded()
    keys = set()
    for key, (sizes, per) in everything.items():
        for w, items in enumerate(per):
            if any(items.values()):
                keys.add(f"{key}/{w}")
                assert bs.digest(bs.model_as_decoded(bs.model(items, sizes))) == rec[f"{key}/{w}"], (key, w)
    assert keys == set(rec)


@pytest.mark.skipif(not bs.have_reference(), reason="oracle/_ref/libcuskent.a (make -C oracle ref) or gcc is absent")
def test_recorded_digests_are_the_references(everything, tmp_path):
    rec = bs.recorded()
    for key, (sizes, per) in everything.items():
        for w, items in enumerate(per):
            if not any(items.values()):
                continue
            bg, cs = bs.write_inputs(str(tmp_path), items, sizes, f"{key}_{w}")
            out = str(tmp_path / f"{key}_{w}.bw")
            pr = bs.reference_bigwig(str(tmp_path), bg, cs, out)
            assert pr.returncode == 0, pr.stderr
            assert bs.digest(bs.decode(open(out, "rb").read())) == rec[f"{key}/{w}"], (key, w)


def test_sections_case(everything):
    sizes, per = everything["sections"]
    assert {n: len(v) for n, v in per[0].items()} == {"chr1": 1023, "chr10": 1024, "chr2": 1025, "chr3": 2049, "chr5": 1}
    m = bs.model(per[0], sizes)
    assert [n for n, _, _ in m["chroms"]] == ["chr1", "chr10", "chr2", "chr3", "chr5"]          # chr4 has no data and no id
    assert [s[7] for s in m["sections"]] == [1023, 1024, 1024, 1, 1024, 1024, 1, 1]


def test_chain_case(everything):
    sizes, per = everything["chain"]
    m = bs.model(per[0], sizes)
    R, sums = first_level(m, cid=1)
    iv, size, marks = cases.chain_layout(R)                # the layout was made for the reduction the model finds
    assert size == sizes["chrG"] and sorted(bs.depth_items(iv)) == sorted(per[0]["chrG"])
    starts = {r[1] for r in sums}
    at = lambda p: next(r for r in sums if r[1] <= p < r[2])
    # measured against the open summary's end E: R - 1 goes on at E, R and more start anew at the item
    assert marks["gap_R-1"] not in starts and at(marks["gap_R-1"])[1] == marks["gap_R-1"] - (R - 1)
    for k in ("gap_R", "gap_2R-2", "gap_2R-1"):
        assert marks[k] in starts, k
    # the same gap between neighbours (2 R - 6, ambiguous), two phases
    assert marks["amb_stays"] not in starts and at(marks["amb_stays"])[1] == marks["amb_stays"] - (R - 1)
    assert marks["amb_anchors"] in starts
    # two ambiguous gaps in a row (R + 3 each): neither anchors, the summaries go on from the group's first item in steps of R
    a = marks["amb_twice"] - 10 - 2 * (R + 3)
    assert a in starts and a + R in starts and marks["amb_twice"] not in starts and at(marks["amb_twice"])[1] == a + 2 * R
    # one item over four summaries: each part is weighed against what is left of the item, so the bases are over-counted
    parts = [r for r in sums if marks["long"] <= r[1] < marks["long"] + 3 * R + 7]
    assert len(parts) == 4 and [r[1] for r in parts] == [marks["long"] + k * R for k in range(4)]
    assert sum(r[3] for r in parts) > 3 * R + 7
    # 120 items inside one summary
    assert at(marks["many"])[1] == marks["many"] and at(marks["many"])[3] == 120
    # the last summary is clipped to the chromosome's size
    assert sums[-1][1] == marks["clipped"] and sums[-1][2] == size and size - marks["clipped"] < R


def test_loop_and_twoblocks_cases(everything):
    sizes, per = everything["loop"]
    assert bs.model(per[0], sizes)["rounds"] >= 3           # the loop went round at least twice
    sizes, per = everything["twoblocks"]
    assert len(bs.model(per[0], sizes)["zooms"][0][1]) // 32 > 1024
    sizes, per = everything["uniq_empty"]
    assert any(per[0].values()) and not any(per[1].values())


def test_no_small_input_drops_a_level():
    """the search behind the statement in tests/test_gpu_gcov_bigwig.py: over these draws the reference's lastSummarySize comparison
    never refuses a later level"""
    for seed in range(60):
        rng = np.random.default_rng(seed)
        n, gm, lm = int(rng.integers(2, 300)), int(rng.choice([1, 5, 50, 500, 5000])), int(rng.choice([1, 3, 30, 300]))
        iv = bs.blocks(rng, n, 10, gm, lm)
        assert bs.model({"c": bs.depth_items(iv)}, {"c": iv[-1][1] + 10})["dropped"] == [], seed
