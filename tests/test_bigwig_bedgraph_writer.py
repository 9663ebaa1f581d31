"""The sparse bigWig writer of the host program (iteres_amd/host/bw_sparse.c write_bigwig_sparse, through the test tool
bw_from_bedgraph) against the reference's converter, on CPU: a driver of a few lines (bwsparse.DRIVER) calls bigWigFileCreate from
oracle/_ref/libcuskent.a on the same bedGraph and size file. The two files are the same bytes (same rule, same zlib), and the model
of the rule (bwsparse.model) gives the sections and zoom records that the file decodes to.

The draws: two chromosomes with data and one without; item counts from a few hundred to 60 000; gaps from 0 (items that touch) to
100 000, so that summaries re-anchor, continue and split items; draw 3 makes the first-reduction loop go round more than once
(asserted)."""
import os
import subprocess

import numpy as np
import pytest

import bwsparse as bs

HOST = os.path.join(bs.ROOT, "iteres_amd", "host")

pytestmark = pytest.mark.skipif(not bs.have_reference(), reason="oracle/_ref/libcuskent.a (make -C oracle ref) or gcc is absent")


def draw(seed, n, gap_max, len_max, frac=False):
    """n items over chr2 and chr10 (chr1 of the size file stays empty): random lengths in [1, len_max], gaps in [0, gap_max]"""
    rng = np.random.default_rng(seed)
    items, sizes = {}, {"chr1": 5000, "chr10": 0, "chr2": 0}
    for name, k in (("chr2", n - n // 3), ("chr10", n // 3)):
        ln = rng.integers(1, len_max + 1, k)
        gap = rng.integers(0, gap_max + 1, k)
        if gap_max > 1000:
            gap[rng.random(k) < 0.5] //= 1000                                 # dense stretches between the long gaps
        start = np.cumsum(gap + np.concatenate([[0], ln[:-1]])) + int(rng.integers(0, 50))
        val = rng.integers(1, 60, k).astype(np.float64)
        if frac:
            val = val + rng.integers(0, 8, k) / 8.0
        items[name] = list(zip(start.tolist(), (start + ln).tolist(), val.tolist()))
        sizes[name] = int(start[-1] + ln[-1]) + int(rng.integers(0, 3))
    return items, sizes


DRAWS = {
    "small": (1, 200, 30, 20, False),
    "touching": (2, 3000, 0, 7, False),
    "loop": (3, 20000, 3, 1, False),
    "far": (4, 5000, 100000, 300, True),
    "big": (5, 60000, 2000, 50, False),
}


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-s", "-C", HOST, "test/bw_from_bedgraph"])
    return os.path.join(HOST, "test", "bw_from_bedgraph")


@pytest.mark.parametrize("key", list(DRAWS))
def test_writer_matches_reference_and_model(key, tool, tmp_path):
    items, sizes = draw(*DRAWS[key])
    bg, cs = bs.write_inputs(str(tmp_path), items, sizes)
    ours, ref = str(tmp_path / "ours.bw"), str(tmp_path / "ref.bw")
    subprocess.check_call([tool, bg, cs, ours])
    pr = bs.reference_bigwig(str(tmp_path), bg, cs, ref)
    assert pr.returncode == 0, pr.stderr
    got, want = open(ours, "rb").read(), open(ref, "rb").read()
    m = bs.model(items, sizes)
    print(f"{key}: {sum(len(v) for v in items.values())} items, {len(m['sections'])} sections, reductions {[z[0] for z in m['zooms']]}, "
          f"{[len(z[1]) // 32 for z in m['zooms']]} summaries, {m['rounds']} rounds, dropped {m['dropped']}")
    bs.check_against_model(bs.decode(want), m)
    bs.check_against_model(bs.decode(got), m)
    assert got == want
    if key == "loop":
        assert m["rounds"] >= 2


def test_empty_input_is_refused_like_the_reference(tool, tmp_path):
    bg, cs = bs.write_inputs(str(tmp_path), {}, {"chr1": 1000})
    ours, ref = str(tmp_path / "ours.bw"), str(tmp_path / "ref.bw")
    a = subprocess.run([tool, bg, cs, ours], capture_output=True, text=True)
    b = bs.reference_bigwig(str(tmp_path), bg, cs, ref)
    assert a.returncode == 255 and b.returncode == 255
    assert "is empty of data" in a.stderr and "is empty of data" in b.stderr
    assert not os.path.exists(ours) and not os.path.exists(ref)
