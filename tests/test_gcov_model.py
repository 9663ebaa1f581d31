"""CPU: what the `filter -G` tests rest on (tests/gcovcase.py).
1. the bedGraph model against hand-written cases;
2. the generated reads have unique names, and single-end, paired and unknown-chromosome reads are all there;
3. the recorded expectations (tests/golden/gcov/) belong to the inputs the generator makes here;
4. where the reference binary is built: every name its `filter -r` lists has exactly one `stat -B` bed line, and the counted
   intervals equal the recording — for every option set of the command tests."""
import os

import numpy as np
import pytest

import gcovcase as gv


# ---- 1. the model

def test_model_single_read():
    assert gv.bedgraph([("chr1", 10, 20)]) == b"chr1\t10\t20\t1\n"


def test_model_abutting_reads_of_equal_depth_are_one_line():
    assert gv.bedgraph([("chr1", 10, 20), ("chr1", 20, 35)]) == b"chr1\t10\t35\t1\n"


def test_model_identical_reads():
    assert gv.bedgraph([("chr1", 10, 20), ("chr1", 10, 20)]) == b"chr1\t10\t20\t2\n"


def test_model_nested_read_gives_three_lines():
    assert gv.bedgraph([("chr1", 10, 40), ("chr1", 20, 30)]) == b"chr1\t10\t20\t1\nchr1\t20\t30\t2\nchr1\t30\t40\t1\n"


def test_model_overlap_and_gap():
    assert gv.bedgraph([("c", 0, 5), ("c", 3, 8), ("c", 9, 10)]) == b"c\t0\t3\t1\nc\t3\t5\t2\nc\t5\t8\t1\nc\t9\t10\t1\n"


def test_model_abutting_reads_of_different_depth_are_two_lines():
    assert gv.bedgraph([("c", 0, 5), ("c", 0, 5), ("c", 5, 9)]) == b"c\t0\t5\t2\nc\t5\t9\t1\n"


def test_model_chromosomes_in_byte_order_whatever_the_input_order():
    got = gv.bedgraph([("chr2", 1, 2), ("chrM", 1, 2), ("chr10", 1, 2), ("chr1", 1, 2), ("Chr9", 1, 2), ("chr1_alt", 1, 2)])
    assert [l.split(b"\t")[0] for l in got.splitlines()] == [b"Chr9", b"chr1", b"chr10", b"chr1_alt", b"chr2", b"chrM"]


def test_model_no_reads_is_empty_and_unique_splits_at_the_threshold():
    assert gv.bedgraph([]) == b""
    a, u = gv.both([("c", 1, 5, gv.MAPQ_MIN - 1), ("c", 1, 5, gv.MAPQ_MIN)])
    assert a == b"c\t1\t5\t2\n" and u == b"c\t1\t5\t1\n"


def test_model_many_reads_against_a_dense_array():
    rng = np.random.default_rng(5)
    s = rng.integers(0, 900, 400)
    e = s + rng.integers(1, 90, 400)
    dense = np.zeros(1000, np.int64)
    for a, b in zip(s, e):
        dense[a:b] += 1
    want, k = [], 0
    while k < 1000:
        j = k
        while j < 1000 and dense[j] == dense[k]:
            j += 1
        if dense[k]:
            want.append(b"c\t%d\t%d\t%d\n" % (k, j, dense[k]))
        k = j
    assert gv.bedgraph([("c", a, b) for a, b in zip(s, e)]) == b"".join(want)


# ---- 2, 3. the inputs

@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gcov_inputs") / "in")
    t, r, big, name, fam = gv.make_inputs(d)
    return d, r, big, name, fam


def test_generated_names_are_unique_and_the_kinds_are_there(inputs):
    d, r, big, name, fam = inputs
    assert len(set(r.qname)) == len(r.qname) == gv.N_READS
    paired = (r.flag & 1) != 0
    assert 1000 < paired.sum() < 3000
    assert (r.tid == 1).sum() > 50 and r.header[1][0] == "chrU" and "chrU" not in dict(gv.CHROMS)
    assert len(set(r.tid[r.tid >= 0])) == len(gv.BAM_HEADER) >= 4
    assert ((r.isize > 0) & paired).sum() > 100 and ((r.isize < 0) & paired).sum() > 100


@pytest.mark.parametrize("key", list(gv.OPTSETS))
def test_recording_belongs_to_these_inputs(inputs, key):
    d = inputs[0]
    counted, digest = gv.recorded_counted(key)
    assert digest == gv.input_digest(d)
    assert len(counted) > (300 if key not in ("name", "class", "family") else 20)
    if key != "R":                                                              # (-R drops every read below -Q: generic.c:907-919)
        assert sum(c[3] >= gv.MAPQ_MIN for c in counted) < len(counted)         # the two files differ
    sizes = dict(gv.CHROMS)
    assert all(0 <= s < e <= sizes[c] - 1 for c, s, e, q in counted)
    assert len({c[0] for c in counted}) >= (3 if key not in ("name", "class", "family") else 1)


def test_the_sam_text_is_the_same_reads_to_the_reference():
    assert gv.recorded_counted("S")[0] == gv.recorded_counted("ALL")[0]


# ---- 4. the reference itself

@pytest.mark.skipif(not os.path.exists(gv.REF), reason="oracle/_ref/iteres is not built (make -C oracle ref needs the reference tree)")
@pytest.mark.parametrize("key", list(gv.OPTSETS))
def test_reference_lists_one_bed_line_per_name_and_equals_the_recording(inputs, key, tmp_path):
    d, r, big, name, fam = inputs
    aln, opts = gv.OPTSETS[key]
    bed, listed = gv.reference_outputs(d, aln, gv.fill(opts, big, name, fam), str(tmp_path))
    assert len(set(listed)) == len(listed) > 0
    assert all(len(bed.get(n, ())) == 1 for n in listed)
    assert sorted(bed[n][0] for n in listed) == gv.recorded_counted(key)[0]
