"""Which zoom levels a bigWig gets (iteres_amd/csrc/itx_bwzoomrule.h: the first reduction tried again until its summaries fit, every
further level x4 and counted from the last level kept, a level dropped when its size is the last one refused, the three ways the
levels end, a reduction outside 1 .. 0x3fffffff reported instead of computed with): the header built into a stand-alone program
(tests/bwzoomrule_main.c) as C11 and as C++17, plain and with the address and undefined-behaviour sanitizers, driven with tables
reduction -> count, its decisions held equal to the restatement in tests/bwsparse.py (zoom_levels) fed the same tables. The rule
decides from counts alone, so a table need not be one that data can give: no input was found that makes the reference drop a later
level (tests/test_gpu_gcov_bigwig.py), and here a table does. The dense writer's counts are closed-form (host/bw_dense.c): for the
sequence lengths of two geometries of tests/test_gpu_bigwig_kernels.py (restated here) the levels are also held equal to what bw_plan_levels
answered before the rule was stated once."""
import os
import subprocess

import pytest

import bwsparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bwzoomrule_main.c")
BUILDS = {"c11": ["gcc", "-std=c11"], "cxx17": ["g++", "-std=c++17", "-x", "c++"]}
SANITIZE = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
MAX_RED = bwsparse.MAX_RED


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("bwzoomrule")
    for b, cc in BUILDS.items():
        for s, flags in SANITIZE.items():
            exe = str(d / f"bwzoomrule_{b}_{s}")
            subprocess.check_call(cc + ["-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
            out[b, s] = exe
    return out


def _model(full, min_res, n_chrom, count_of):
    """bwsparse.zoom_levels with the counts of count_of(reduction), and the table it asked for"""
    table = {}

    def count(red, src):
        table[red] = count_of(red)
        return table[red]
    return bwsparse.zoom_levels(full, min_res, n_chrom, count), table


def _program(exe, full, min_res, n_chrom, table):
    r = subprocess.run([exe, str(full), str(min_res), str(n_chrom)] + [f"{k}:{v}" for k, v in table.items()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {"tries": [], "refused": None, "levels": None, "fixed": None, "steps": [], "rounds": None}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "try":
            out["tries"].append(int(w[1]))
        elif w[0] == "range":
            out["refused"], out["rounds"] = int(w[1]), int(w[3])
        elif w[0] == "fixed":
            out["fixed"], out["rounds"] = int(w[1]), int(w[3])
        elif w[0] in ("keep", "drop"):
            out["steps"].append((int(w[1]), int(w[3]), w[0] == "keep"))
        elif w[0] == "levels":
            out["levels"] = [int(x) for x in w[1:]]
        else:
            raise AssertionError(line)
    return out


def _agree(exe, full, min_res, n_chrom, count_of):
    want, table = _model(full, min_res, n_chrom, count_of)
    got = _program(exe, full, min_res, n_chrom, table)
    assert got["tries"] == want["tries"] and got["rounds"] == len(want["tries"])
    if want["refused"] is not None:
        # (what no int holds the header reports as MAX_RED + 1; the restatement has no int)
        assert got["refused"] == (want["refused"] if want["refused"] < 1 << 31 else MAX_RED + 1) and got["levels"] is None and not got["steps"]
    else:
        assert got["refused"] is None and got["fixed"] == want["levels"][0]
        assert got["steps"] == want["steps"] and got["levels"] == want["levels"]
    return want


def _table(t):
    return lambda red: t[red]


CASES = {
    # name: (full size, mean resolution, chromosomes, reduction -> count)
    "fixed_at_the_first_try": (1_000_000, 1, 1, lambda red: -(-1000 // red)),
    # 10: size 3200 of 1000, 1.1 * 10 * 3.2 = 35 > 20; 35: size 1280, 1.1 * 35 * 1.28 = 49 < 70; 70: size 640 fits
    "three_tries_formula_then_doubling": (2000, 1, 1, _table({10: 50, 35: 20, 70: 10, 280: 3, 1120: 1})),
    "the_size_repeats": (2000, 1, 1, _table({10: 50, 35: 50, 140: 9, 560: 2, 2240: 1})),
    # 10: size 25600 of 20000 is refused (and remembered), 20 fits; 80 gives 32 * 800 == 25600: dropped; 320 is counted from 20
    "a_later_level_dropped": (40_000, 1, 1, _table({10: 400, 20: 300, 80: 800, 320: 50, 1280: 10, 5120: 1})),
    "ends_above_1e9": (1 << 40, 30_000_000, 1, lambda red: 7),
    "nine_further_levels": (1 << 40, 1, 1, lambda red: 5),
    "as_many_summaries_as_chromosomes": (1 << 40, 1, 7, lambda red: 7),
    "refused_at_once_zero": (1000, 0, 1, _table({})),
    "refused_at_once_negative": (1000, -1, 1, _table({})),
    "refused_at_once_large": (1000, 200_000_000, 1, _table({})),
    "refused_after_doubling": (1000, 60_000_000, 1, _table({600_000_000: 8})),
    "refused_product_beyond_int": (1000, 50_000_000, 1, _table({500_000_000: 80})),
}


@pytest.mark.parametrize("sanitize", list(SANITIZE))
@pytest.mark.parametrize("build", list(BUILDS))
def test_decisions_equal_the_restatement(programs, build, sanitize):
    exe = programs[build, sanitize]
    seen = {name: _agree(exe, *case) for name, case in CASES.items()}
    # the tables are what they claim
    assert seen["fixed_at_the_first_try"]["tries"] == [10] and seen["fixed_at_the_first_try"]["levels"] == [10, 40, 160, 640, 2560]
    assert seen["three_tries_formula_then_doubling"]["tries"] == [10, 35, 70]
    assert seen["the_size_repeats"]["tries"] == [10, 35] and seen["the_size_repeats"]["levels"][0] == 35
    d = seen["a_later_level_dropped"]
    assert d["dropped"] == [80] and d["steps"][:2] == [(80, 20, False), (320, 20, True)] and d["levels"] == [20, 320, 1280, 5120]
    assert seen["ends_above_1e9"]["levels"] == [300_000_000] and not seen["ends_above_1e9"]["steps"]
    assert seen["nine_further_levels"]["levels"] == [10 * 4 ** k for k in range(10)]
    assert seen["as_many_summaries_as_chromosomes"]["levels"] == [10, 40]
    for name, tries, red in (("refused_at_once_zero", [], 0), ("refused_at_once_negative", [], -10), ("refused_at_once_large", [], 2_000_000_000),
                             ("refused_after_doubling", [600_000_000], 1_200_000_000)):
        assert seen[name]["tries"] == tries and seen[name]["refused"] == red, name
    assert seen["refused_product_beyond_int"]["tries"] == [500_000_000] and seen["refused_product_beyond_int"]["refused"] > 1 << 31


def _dense_lengths():
    """the sequence lengths of GEOMETRY["r1_ten_levels"] and ["many_short_sequences"] in tests/test_gpu_bigwig_kernels.py (that module
    needs the engine; the lengths are restated here: lengths around 1 and the section size, and its 2500 draws from 1 .. 40)"""
    import numpy as np
    many = [int(x) for x in np.random.default_rng([77, 6]).integers(1, 41, 2500)]      # 6: the geometry's place in GEOMETRY
    assert sum(many) == 50493
    return {"r1_ten_levels": [1, 2, 1023, 1024, 1025, 1, 2, 1024, 1025, 300_000, 5], "many_short_sequences": many}


# bw_plan_levels for these lengths, as the writer answered when its loop was its own
PLAN_LEVELS_BEFORE = {"r1_ten_levels": [34, 136, 544, 2176, 8704, 34816, 139264, 557056], "many_short_sequences": [132, 528]}


@pytest.mark.parametrize("geometry", list(PLAN_LEVELS_BEFORE))
def test_dense_closed_form_counts(programs, geometry):
    """every sequence is covered from 0 to its size, so a reduction's summaries tile it: sum of ceil(length / reduction)"""
    lengths = _dense_lengths()[geometry]
    full = sum(24 + 4 * min(1024, n - s) for n in lengths for s in range(0, n, 1024))
    want = _agree(programs["c11", "asan_ubsan"], full, 1, len(lengths), lambda red: sum(-(-n // red) for n in lengths))
    assert want["levels"] == PLAN_LEVELS_BEFORE[geometry] and not want["dropped"]


def test_the_host_plan_gives_these_levels(tmp_path):
    """the dense writer itself (host/bw_dense.c bw_plan_make, through a main of a few lines)"""
    host = os.path.join(ROOT, "iteres_amd", "host")
    src = tmp_path / "plan_main.c"
    src.write_text("""
#include "itx_host.h"
#include <stdlib.h>
int main(int argc, char **argv)
{
    size_t n = (size_t)argc - 1;
    const char **names = calloc(n, sizeof *names);
    uint32_t *len = calloc(n, sizeof *len);
    for (size_t i = 0; i < n; i++) {
        char *nm = malloc(32);
        snprintf(nm, 32, "s%06u", (unsigned)i);
        names[i] = nm;
        len[i] = (uint32_t)strtoul(argv[i + 1], NULL, 10);
    }
    const uint32_t *red;
    const int nl = bw_plan_levels(bw_plan_make("x", names, len, n), &red);
    for (int i = 0; i < nl; i++) printf("%u ", red[i]);
    return 0;
}
""")
    exe = str(tmp_path / "plan_main")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-fopenmp", "-I", host, "-o", exe, str(src)] +
                          [os.path.join(host, f) for f in ("bigwig.c", "bw_sum.c", "bw_dense.c", "bw_sparse.c", "tables.c")] + ["-lz", "-lm"])
    for geometry, lengths in _dense_lengths().items():
        out = subprocess.run([exe] + [str(n) for n in lengths], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        assert [int(x) for x in out.stdout.split()] == PLAN_LEVELS_BEFORE[geometry], geometry
