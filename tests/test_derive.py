"""The record derivation (generic.c:764-905) is stated once for the cold users (-R, the XA veto, the host's bed lines:
itx_derive in iteres_amd/csrc/itx_derive.h) and once in the form k_stream runs (lut_entry + derive_one, same header).
Both are built for the host (tests/derive_host.cpp) and held, record by record,
  * itx_derive against the suite's own statement of the rule (goldencase.derive_py): drop/keep, start, end, strand;
  * the fast form against itx_derive: bit 18 of the table entry <=> keep; start and end equal whenever keep;
    uq <=> MAPQ >= -Q (and bit 21 <=> keep and uq); LUT_OK <=> keep and F5_NOLOOKUP clear. derive_one's caller may
    pass tile_pe = false only for a tile without a paired record: every record goes through tile_pe = true, and every
    record without F5_PAIRED through tile_pe = false as well.
Cases: all 64 flag5 values x 32 option sets x a coordinate grid around every edge of the rule, and 10^6 seeded random
records. Integer arithmetic throughout: equality is exact."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import goldencase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAPQ_MIN = 10
LUT_OK = 1 << 24

# (treat, discard, extension, isize_max): 2 x 2 x 4 x 2 = 32 sets
OPTIONS = list(itertools.product((0, 1), (0, 1), (0, 1, 300, 1 << 31), (0, 500)))


class Opts(C.Structure):
    _fields_ = [("mapq_min", C.c_uint32), ("extension", C.c_uint32), ("isize_max", C.c_uint32), ("treat", C.c_int32), ("discard", C.c_int32)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("derive") / "libderive_host.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # as iteres_amd/build.py finds the toolkit
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", inc,
                           "-o", so, os.path.join(ROOT, "tests", "derive_host.cpp")])
    L = C.CDLL(so)
    p = C.c_void_p
    L.itx_derive_host.restype = None
    L.itx_derive_host.argtypes = [C.POINTER(Opts), C.c_size_t] + [p] * 11
    L.itx_derive_fast_host.restype = None
    L.itx_derive_fast_host.argtypes = [C.POINTER(Opts), C.c_int, C.c_size_t] + [p] * 12
    return L


def i32(a):
    """Values given as 32-bit patterns (signed or unsigned) -> int32."""
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def sam_flag(f5):
    """include/iteres_amd.h: flag5 bit0 PAIRED(0x1) bit1 UNMAP(0x4) bit2 MUNMAP(0x8) bit3 REVERSE(0x10) bit4 READ1(0x40)."""
    f5 = f5.astype(np.int64)
    return (f5 & 1) | (f5 & 2) << 1 | (f5 & 4) << 1 | (f5 & 8) << 1 | (f5 & 16) << 2


def grid():
    """Every flag5 value x MAPQ either side of -Q x chromosome (unknown; size 0, 1, 2 — cend == 1 —, 3, 2^31 - 1) x
    pos (0, size - 1) x tmpend (below, at, past cend) x mpos (0, past the end) x isize (0, +-1, +-500, +-501, extremes)."""
    sizes = [0, 1, 2, 3, I32_MAX]
    tid2chrom = [-1] + list(range(len(sizes)))
    rows = []
    for tid in range(len(tid2chrom)):
        size = 0 if tid == 0 else sizes[tid - 1]
        cend = (size - 1) & 0xFFFFFFFF
        for pos, tmpend, mpos, isz in itertools.product((0, size - 1), (cend - 1, cend, cend + 1), (0, size + 7),
                                                        (0, 1, -1, 500, -500, 501, -501, I32_MAX, I32_MIN)):
            rows.append((tid, pos, tmpend, mpos, isz))
    rows = np.array(rows, np.int64)
    f5, mq, k = np.meshgrid(np.arange(64), np.array([MAPQ_MIN - 1, MAPQ_MIN]), np.arange(len(rows)), indexing="ij")
    f5, mq, k = f5.ravel(), mq.ravel(), k.ravel()
    return dict(tid2chrom=tid2chrom, chrom_size=sizes, tid=rows[k, 0].astype(np.int32), flag5=f5.astype(np.uint8), mapq=mq.astype(np.uint8),
                pos=i32(rows[k, 1]), tmpend=i32(rows[k, 2]), mpos=i32(rows[k, 3]), isize=i32(rows[k, 4]))


def random_records(seed, n):
    """Coordinates that sit near the rule's edges half of the time and anywhere in 32 bits otherwise."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 2, 3, 1000, 46709983, 248956422, I32_MAX] + [int(v) for v in rng.integers(0, 1 << 31, 24)]
    tid2chrom = [-1, -2] + list(range(len(sizes)))
    tid = rng.integers(0, len(tid2chrom), n)
    size = np.array([0, 0] + sizes, np.int64)[tid]

    def near(base, spread):
        wide = rng.integers(I32_MIN, 1 << 31, n)
        return i32(np.where(rng.random(n) < 0.5, base + rng.integers(-spread, spread + 1, n), wide))
    pos = near(rng.integers(0, np.maximum(size, 1)), 3)
    tmpend = near(np.where(rng.random(n) < 0.5, size - 1, pos.astype(np.int64) + 100), 3)
    mpos = near(pos.astype(np.int64) + rng.integers(-600, 601, n), 3)
    isize = near(rng.choice([0, 500, -500, I32_MAX, I32_MIN], n), 2)
    return dict(tid2chrom=tid2chrom, chrom_size=sizes, tid=tid.astype(np.int32), flag5=rng.integers(0, 64, n).astype(np.uint8),
                mapq=rng.choice([0, MAPQ_MIN - 1, MAPQ_MIN, MAPQ_MIN + 1, 255], n).astype(np.uint8), pos=pos, tmpend=tmpend, mpos=mpos, isize=isize)


def check(lib, opt, rec):
    treat, discard, extension, isize_max = opt
    o = Opts(MAPQ_MIN, extension, isize_max, treat, discard)
    n = len(rec["tid"])
    t2c = np.array(rec["tid2chrom"], np.int32)
    chrom = t2c[rec["tid"]]
    size = np.where(chrom >= 0, np.array(rec["chrom_size"], np.int64)[np.maximum(chrom, 0)], 0).astype(np.int32)
    cols = [np.ascontiguousarray(rec[k]) for k in ("pos", "tmpend", "mpos", "isize")]
    f5, mq = rec["flag5"], rec["mapq"]
    ptr = lambda a: a.ctypes.data

    keep, strand = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    start, end = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    lib.itx_derive_host(o, n, ptr(chrom), ptr(size), ptr(f5), *map(ptr, cols), ptr(keep), ptr(start), ptr(end), ptr(strand))
    keep = keep.astype(bool)

    # ---- itx_derive against the suite's own statement
    p = dict(extension=extension, isize_max=isize_max, treat_pe_as_se=treat, discard_half_mapped=discard)
    rd = dict(flag=sam_flag(f5).tolist(), tid=rec["tid"].tolist(), pos=cols[0].tolist(), tmpend=cols[1].tolist(), mpos=cols[2].tolist(),
              isize=cols[3].tolist())
    want = [goldencase.derive_py(p, rec["tid2chrom"], rec["chrom_size"], rd, i) for i in range(n)]
    w_keep = np.array([w is not None for w in want])
    assert np.array_equal(keep, w_keep)
    kept = np.flatnonzero(w_keep)
    assert np.array_equal(start[kept], np.array([want[i][0] for i in kept], np.uint32))
    assert np.array_equal(end[kept], np.array([want[i][1] for i in kept], np.uint32))
    assert np.array_equal(strand[kept], np.array([want[i][2] == "-" for i in kept], np.uint8))

    # ---- the fast form against itx_derive
    def fast(tile_pe, sel):
        m = len(sel)
        a = [np.ascontiguousarray(v[sel]) for v in [chrom, size, f5, mq] + cols]
        lut, st, en, uq = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        lib.itx_derive_fast_host(o, tile_pe, m, *map(ptr, a), ptr(lut), ptr(st), ptr(en), ptr(uq))
        k, u = keep[sel], mq[sel] >= MAPQ_MIN
        assert np.array_equal((lut >> 18 & 1).astype(bool), k)
        assert np.array_equal(st[k], start[sel][k]) and np.array_equal(en[k], end[sel][k])
        assert np.array_equal(uq.astype(bool), u)
        assert np.array_equal((lut >> 21 & 1).astype(bool), k & u)
        assert np.array_equal((lut & LUT_OK) != 0, k & ((f5[sel] & 32) == 0))
    fast(1, np.arange(n))
    unpaired = np.flatnonzero((f5 & 1) == 0)
    assert len(unpaired)
    fast(0, unpaired)


GRID = grid()


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "T%d-D%d-E%d-I%d" % o)
def test_derive_grid(lib, opt):
    assert len(GRID["tid"]) == 64 * 2 * 6 * 2 * 3 * 2 * 9
    check(lib, opt, GRID)


@pytest.mark.parametrize("k", range(len(OPTIONS)), ids=lambda k: "T%d-D%d-E%d-I%d" % OPTIONS[k])
def test_derive_random(lib, k):
    """10^6 random records in all, 31250 under each option set."""
    check(lib, OPTIONS[k], random_records(20240 + k, 1_000_000 // len(OPTIONS)))
