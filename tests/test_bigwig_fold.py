"""The host bigWig writer (iteres_amd/host/bw_dense.c and bw_sum.c, through the test tool bw_from_wig) against tests/bwfold.py, the
plain numpy restatement of the sections and of bbiAddToSummary's sequential float fold, on wigs that leave the exact
regime of the golden runs: counts above 2^24 (up to 4294967295), plateaus that make sum_data round at level 0, and
sequence lengths around the section size and around every reduction the plan picks. And, where the reference binary
is built, the writer against the reference's own bigWig on a pile-up deep enough to round. Everything is compared
bit for bit."""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import bwcases
import bwfold
import refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "iteres_amd", "host")
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-s", "-C", HOST, "test/bw_from_wig"])
    return os.path.join(HOST, "test", "bw_from_wig")


def _write_wig(path, named):
    with open(path, "w") as f:
        for name, v in named:
            f.write(f"fixedStep chrom={name} start=1 step=1 span=1\n")
            f.write("\n".join(map(str, v.tolist())) + "\n")


def _through_writer(tool, named, tmp_path, tag):
    wig, out = str(tmp_path / f"{tag}.wig"), str(tmp_path / f"{tag}.bigWig")
    _write_wig(wig, named)
    subprocess.check_call([tool, wig, out])
    return refio.bigwig_decode(open(out, "rb").read())


def _assert_equals_fold(dec, named):
    """the decoded file holds bwfold's sections and zoom records; returns (reductions, levels)"""
    by_id = sorted(named, key=lambda nv: nv[0].encode())                 # ids follow strcmp of the names
    assert [(nm, cid, size) for nm, cid, size in dec["chroms"]] == [(nm, i, len(v)) for i, (nm, v) in enumerate(by_id)]
    cov = np.concatenate([v for _, v in by_id]).astype(np.uint32)
    seqs, at = [], 0
    for _, v in by_id:
        seqs.append((at, len(v)))
        at += len(v)
    reds = [z[0] for z in dec["zooms"]]
    want = bwfold.build(cov, seqs, reds)
    got_sec = dec["sections"]
    assert len(got_sec) == len(want["sections"])
    for g, w in zip(got_sec, want["sections"]):
        cid, start, end, step, span, typ, _, cnt = struct.unpack_from("<IIIIIBBH", w, 0)
        assert g == (cid, start, end, step, span, typ, w[24:]), (cid, start)
    for k, (red, bounds, recs) in enumerate(dec["zooms"]):
        w = want["levels"][k].tobytes()
        if recs != w:
            a, b = np.frombuffer(recs, bwfold.SUMMARY), want["levels"][k]
            assert len(a) == len(b), (k, red, len(a), len(b))
            i = int(np.flatnonzero(a.view("V32") != b.view("V32"))[0])
            raise AssertionError(f"level {k} (reduction {red}), summary {i}: writer {a[i]} / fold {b[i]}")
    return reds, want["levels"], cov, seqs


def _lengths_with_reductions(tool, tmp_path, base):
    """base lengths plus r - 1, r, r + 1 for every reduction r the plan picks for the resulting set. The plan depends on
    the lengths, so this is iterated until it stands; and it goes on adding levels until a reduction holds every
    sequence in one summary, so no sequence can be longer than the TOP reduction: that one gets r - 1 and r only."""
    lens = list(base)
    for it in range(12):
        named = [(f"s{i:04d}", np.zeros(n, np.uint32)) for i, n in enumerate(lens)]
        reds = [z[0] for z in _through_writer(tool, named, tmp_path, f"plan{it}")["zooms"]]
        need = [x for r in reds for x in ((r - 1, r, r + 1) if r != reds[-1] else (r - 1, r)) if x >= 1 and x not in lens]
        if not need:
            return lens, reds
        lens += need
    raise AssertionError("the plan's reductions did not settle")


def test_writer_equals_fold_on_synthetic_wigs(tool, tmp_path):
    base = [1, 1023, 1024, 1025, 2, 3, 2049, 40_000]
    lens, reds = _lengths_with_reductions(tool, tmp_path, base)
    assert len(reds) >= 3
    for r in reds:
        assert {r - 1, r} <= set(lens) and (r == reds[-1] or r + 1 in lens)
    print(f"reductions {reds}, {len(lens)} sequences, {sum(lens)} bases")
    rng = np.random.default_rng(11)
    seen_big = seen_max = False
    rounds0 = roundsk = 0
    for ci, kind in enumerate(bwcases.CONTENT):
        # every class as a wig of its own, and the names in an order that is not the id order
        named = [(f"q{(7 * i + 3) % len(lens):03d}_{i}", bwcases.content(kind, n, 100 + i)) for i, n in enumerate(lens)]
        if kind == "uniform_u32":
            named[0][1][0] = 0xFFFFFFFF
        dec = _through_writer(tool, named, tmp_path, kind)
        got_reds, levels, cov, seqs = _assert_equals_fold(dec, named)
        assert got_reds == reds                      # the plan looks at the lengths only
        seen_big |= bool((cov > (1 << 24)).any())
        seen_max |= bool((cov == 0xFFFFFFFF).any())
        # the fold order matters for these inputs: a float64 sum of the same items gives other floats
        vals = bwfold.base_values(cov).astype(np.float64)
        l0 = levels[0]
        first = np.concatenate([[0], np.cumsum([(n + reds[0] - 1) // reds[0] for _, n in seqs])])
        for c, (off, n) in enumerate(seqs):
            s = l0[first[c]:first[c + 1]]
            exact = np.add.reduceat(vals[off:off + n], np.arange(0, n, reds[0]))
            rounds0 += int((s["sum_data"] != exact.astype(np.float32)).sum())
        roundsk += int(sum((lv["sum_data"] > 2.0 ** 24).sum() for lv in levels[1:]))
    assert seen_big and seen_max
    assert rounds0 > 0 and roundsk > 0, (rounds0, roundsk)


def test_writer_equals_fold_on_one_base_and_single_sequences(tool, tmp_path):
    for tag, named in (("one", [("a", np.array([4294967295], np.uint32))]),
                       ("zero", [("a", np.array([0], np.uint32))]),
                       ("pair", [("b", np.array([16777217, 16777219], np.uint32)), ("a", np.array([7], np.uint32))]),
                       ("sec", [("x", bwcases.content("uniform_u32", 1024, 5))]),
                       ("sec1", [("x", bwcases.content("plateaus", 1025, 6))])):
        _assert_equals_fold(_through_writer(tool, named, tmp_path, tag), named)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/iteres not built (make -C oracle ref)")
def test_writer_matches_reference_in_the_rounding_regime(tool, tmp_path):
    """The reference's `stat -w` on the pile-up input of bwcases (400 000 reads: generating it takes about 3 s, the
    reference's run about 0.4 s on one core of the build machine), its wig through our writer, and the two bigWig
    files by digest. The depth is asserted on the reference's wig: level-0 summaries with sum_squares > 2^24 and
    summaries with sum_data > 2^24 both exist, so the comparison happens where floats round."""
    inp = tmp_path / "in"
    inp.mkdir()
    paths = bwcases.write_pileup_input(inp)
    work = tmp_path / "ref"
    work.mkdir()
    t0 = time.time()
    pr = subprocess.run([REF, "stat"] + bwcases.PILEUP_OPTS + ["-o", "out"] + paths, cwd=work, capture_output=True, text=True, timeout=600)
    print(f"reference run: {time.time() - t0:.2f} s")
    assert pr.returncode == 0, pr.stderr[-1500:]
    for wig, bw in (("out.iteres.wig", "out.iteres.bigWig"), ("out.iteres.unique.wig", "out.iteres.unique.bigWig")):
        ref = (work / bw).read_bytes()
        vals, order = refio.parse_wig(str(work / wig))
        dec = refio.bigwig_decode(ref)
        n_sq, n_sd = bwcases.wig_depth(vals, [nm for nm, _, _ in dec["chroms"]], [z[0] for z in dec["zooms"]])
        print(f"{wig}: max {max(int(v.max()) for v in vals.values())}, level-0 summaries with sum_squares > 2^24: {n_sq}, "
              f"summaries with sum_data > 2^24: {n_sd}")
        assert n_sq >= 1 and n_sd >= 1, (wig, n_sq, n_sd)
        out = str(tmp_path / bw)
        subprocess.check_call([tool, str(work / wig), out])
        got = open(out, "rb").read()
        assert refio.bigwig_digest(got) == refio.bigwig_digest(ref), bw
        # and the reference's own file holds what the restatement says
        _assert_equals_fold(dec, [(nm, vals[nm]) for nm in order])
