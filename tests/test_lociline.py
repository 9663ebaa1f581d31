"""The line of the .loci files of `filter` / `cpgfilter` (iteres_amd/csrc/itx_lociline.h, the rule csrc/itx_loci.hip runs per table
row) built for the host (tests/lociline_host.cpp):
1. "%.3f" by the integer rule against Python's own `'%.3f' % v` (correctly rounded, like glibc's): zeros, subnormals, exact ties to
   even, ties next to integers up to 2^40, 2^52 .. 2^63 - 1024, negative values, 200 k random bit patterns, 200 k RPKM / RPM
   quotients whose doubles Python computes with the same expression;
2. whole lines of both kinds laid down in pieces of 1, 7 and 64 bytes; 3. the predicate "the host has to look";
4. the sort key: (chromosome rank, bin, -row) against goldencase.loci_row_order on the golden tables, rows on all six bin levels."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import goldencase as gc
import refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER, CPG = 0, 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lociline") / "liblociline_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, os.path.join(ROOT, "tests", "lociline_host.cpp")])
    L = C.CDLL(so)
    L.itxl_bin.argtypes = [C.c_int, C.c_int]
    L.itxl_key.argtypes = [C.c_uint32, C.c_int]
    L.itxl_key.restype = C.c_uint32
    L.itxl_f3_hard.argtypes = [C.c_double]
    L.itxl_f3_many.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.itxl_f3_many.restype = None
    L.itxl_filter_doubles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.itxl_filter_doubles.restype = None
    L.itxl_line.restype = C.c_longlong
    L.itxl_line.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_uint64, C.c_double, C.c_char_p, C.c_uint32, C.c_uint32]
    return L


def f3(lib, values):
    """the header's "%.3f" of every value (None: the rule does not model it)"""
    v = np.ascontiguousarray(values, np.float64)
    out = np.zeros(32 * len(v), np.uint8)
    ln = np.zeros(len(v), np.int32)
    lib.itxl_f3_many(v.ctypes.data, len(v), out.ctypes.data, ln.ctypes.data)
    raw = out.tobytes()
    res = []
    for i, l in enumerate(ln):
        assert l >= -1, (i, v[i])
        if l >= 0:
            assert raw[32 * i + l:32 * i + 32] == b"\xaa" * (32 - l), "wrote past the number"
        res.append(None if l < 0 else raw[32 * i:32 * i + l].decode())
    return res


def check_f3(lib, values):
    got = f3(lib, values)
    bad = [(float(v), g, "%.3f" % v) for v, g in zip(values, got) if g != "%.3f" % v]
    assert not bad, (len(bad), bad[:5])


def test_f3_named_values(lib):
    vals = [0.0, 4.9e-324, 2.2250738585072014e-308, 0.0005, 0.0015, 0.0625, 0.1875, 0.3125, 0.4375, 0.9995, 0.99949999999999994, 1e-3, 0.5, 1.0, 999.9995,
            2.0 ** 52, 2.0 ** 53 + 2, 2.0 ** 63 - 1024, 2.0 ** 62, 1e15 + 0.5, 1e18, 9.2e18, 123456789.0125, 12345678901234567.0]
    ties = [0.0625, 0.1875, 0.3125, 0.4375]
    for k in list(range(0, 41)):
        vals += [t + float(2 ** k) for t in ties] + [t + float(2 ** k - 1) for t in ties]
    vals += [t + n for t in ties for n in (1, 2, 7, 10, 99, 1000, 123456, 10 ** 9 + 7)]
    got = f3(lib, vals)
    assert got[:9] == ["0.000", "0.000", "0.000", "0.001", "0.002", "0.062", "0.188", "0.312", "0.438"]
    assert got[15] == "4503599627370496.000" and got[16] == "9007199254740994.000" and got[17] == "9223372036854774784.000"
    check_f3(lib, vals)
    # the CpG kind: a sign, and -0.000 for what rounds to nothing
    neg = [-0.0, -0.0001, -0.0005, -0.0015, -1.0] + [-t for t in ties] + [-(t + 5) for t in ties] + [-(2.0 ** 63 - 1024), -4.9e-324]
    got = f3(lib, neg)
    assert got[:3] == ["-0.000", "-0.000", "-0.001"] and got[5] == "-0.062" and got[6] == "-0.188"
    check_f3(lib, neg)


def test_f3_random_bit_patterns(lib):
    rng = np.random.default_rng(20240611)
    bits = rng.integers(0, 0x43E0000000000000, 200_000, dtype=np.uint64)          # every finite non-negative double below 2^63
    vals = bits.view(np.float64)
    assert vals.max() < 2.0 ** 63 and (vals < 1e-300).sum() > 1000 and (vals > 1e15).sum() > 1000
    check_f3(lib, vals)
    # where the third decimal is decided: one ulp either side of k * 0.0005
    k = rng.integers(1, 4_000_000, 50_000)
    mid = k * 0.0005
    check_f3(lib, np.concatenate([mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.inf)]))
    check_f3(lib, -vals[:20_000])


def test_f3_of_the_filter_quotients(lib):
    rng = np.random.default_rng(7)
    n = 200_000

    def spread(n):                                                                  # 1 .. 2^31 - 1, every magnitude
        v = (2.0 ** rng.uniform(0, 31, n)).astype(np.int64)
        v[:4] = [1, 2 ** 31 - 1, 1, 2 ** 31 - 1]
        return np.clip(v, 1, 2 ** 31 - 1)
    count, length, reads = spread(n), np.roll(spread(n), 1), np.roll(spread(n), 2)
    reads[100:200] = 360_000_000
    rpkm = np.zeros(n)
    rpm = np.zeros(n)
    c32, l32, r64 = count.astype(np.uint32), length.astype(np.uint32), reads.astype(np.uint64)
    lib.itxl_filter_doubles(c32.ctypes.data, l32.ctypes.data, r64.ctypes.data, n, rpkm.ctypes.data, rpm.ctypes.data)
    want_rpkm = np.array([float(c) / (float(r) * 1e-9 * float(l)) for c, l, r in zip(count.tolist(), length.tolist(), reads.tolist())])
    want_rpm = np.array([float(c) / (float(r) * 1e-6) for c, r in zip(count.tolist(), reads.tolist())])
    assert np.array_equal(rpkm, want_rpkm) and np.array_equal(rpm, want_rpm)
    assert rpkm.max() < 2.0 ** 63
    check_f3(lib, want_rpkm)
    check_f3(lib, want_rpm)


# ---- lines

def py_line(kind, chrom, rep, cla, fam, start, end, count, reads_num, total):
    def i32(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31
    length = (end - start) % 2 ** 32
    cnt = i32(count)
    head = b"%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t" % (chrom, i32(start), i32(end), i32(length), rep, cla, fam, cnt)
    if kind == CPG:
        return head + b"%.3f\n" % total
    c64 = float(cnt % 2 ** 64)
    return head + b"%.3f\t%.3f\n" % (c64 / (float(reads_num) * 1e-9 * float(length)), c64 / (float(reads_num) * 1e-6))


def host_line(lib, piece, kind, chrom, rep, cla, fam, start, end, count, reads_num, total):
    cap = len(chrom) + len(rep) + len(cla) + len(fam) + 160
    out = C.create_string_buffer(cap)
    n = lib.itxl_line(kind, chrom, len(chrom), rep, len(rep), cla, len(cla), fam, len(fam), start, end, count % 2 ** 32, reads_num, total, out, cap, piece)
    if n < 0:
        return n
    assert out.raw[n:] == b"\xaa" * (cap - n), "wrote past the line"
    return out.raw[:n]


LINES = [
    (b"c", b"r", b"k", b"f", 0, 1, 0, 1, 0.0),
    (b"chr1", b"AluY", b"SINE", b"Alu", 9, 10, 9, 3, 0.0625),
    (b"chr10_random", b"L1PA2", b"LINE", b"L1", 99, 1234, 10, 360_000_000, -0.0001),
    (b"X" * 255, b"n" * 255, b"c" * 255, b"f" * 255, 123456, 7654321, 99_999, 360_000_000, 1234567.0005),
    (b"chrUn", b"(CA)n", b"Simple_repeat", b"Simple_repeat", 12345678, 123456789, 2 ** 31 - 1, 2 ** 40, -17.1875),
    (b"chr2", b"MER5A", b"DNA", b"hAT-Charlie", 1234567890, 2147483647, 1, 1, 2.0 ** 63 - 1024),
    (b"chrW", b"x", b"y", b"z", 5, 4000000000, 7, 12, 1e-9),                          # a coordinate that prints as a negative %d
    (b"chrY", b"big", b"q", b"w", 100, 110, 2 ** 31 - 1, 1, -(2.0 ** 62)),             # RPKM of 19 digits
]


@pytest.mark.parametrize("kind", [FILTER, CPG], ids=["filter", "cpgfilter"])
def test_lines_in_pieces(lib, kind):
    for args in LINES:
        want = py_line(kind, *args)
        for piece in (0, 1, 7, 64):
            assert host_line(lib, piece, kind, *args) == want, (args, piece)
    assert any(len(py_line(kind, *a)) > 1000 for a in LINES)
    digits = {len(b"%d" % a[4]) for a in LINES} | {len(b"%d" % a[5]) for a in LINES}
    assert {1, 2, 10} <= digits


def test_the_host_has_to_look(lib):
    names = (b"chr1", b"r", b"k", b"f")
    assert host_line(lib, 0, FILTER, *names, 10, 20, 5, 0, 0.0) == -1                # reads_num 0: inf
    assert host_line(lib, 0, FILTER, *names, 10, 20, 0, 0, 0.0) == -1                # 0 / 0: nan
    assert host_line(lib, 0, FILTER, *names, 10, 10, 5, 100, 0.0) == -1              # length 0
    assert host_line(lib, 0, FILTER, *names, 10, 20, 5, 100, 0.0) not in (-1, -2)
    for v in (float("inf"), float("-inf"), float("nan"), 2.0 ** 63, -(2.0 ** 63), 1e300):
        assert lib.itxl_f3_hard(v) == 1 and host_line(lib, 0, CPG, *names, 1, 2, 3, 0, v) == -1, v
    below = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", 2.0 ** 63))[0] - 1))[0]
    for v in (below, -below, 0.0, -0.0, 4.9e-324):
        assert lib.itxl_f3_hard(v) == 0 and host_line(lib, 0, CPG, *names, 1, 2, 3, 0, v) == py_line(CPG, *names, 1, 2, 3, 0, v), v


# ---- the sort key

def test_bins_on_all_six_levels(lib):
    seen = set()
    for k in range(0, 30):
        for start in (0, 1, 131071, 131072, 1 << 20, (1 << 26) + 5, 300_000_000, (1 << 29) - 1):
            end = start + (1 << k)
            b = lib.itxl_bin(start, end)
            assert b == gc.bin_of(start, end) and b >= 0
            if b >= 8192:                                                             # a short row at 460 M and above: not the key's
                assert start >= 3511 << 17
                continue
            seen.add(sum(b >= o for o in (1, 9, 73, 585, 4681)))
            assert lib.itxl_key(5, b) == 5 << 13 | b
    assert seen == {0, 1, 2, 3, 4, 5}
    assert lib.itxl_bin((1 << 29) - 1, (1 << 29) + 1) == 0                            # across 512 M: the one bin of the top level
    assert lib.itxl_bin(0, 0) == -1                                                   # no level holds it (binRange.c:136 errAborts)


@pytest.mark.parametrize("case,field,name", [("quirks", 0, "ALL"), ("mid", 0, "ALL"), ("mid", 10, "Rep1"), ("cpg", 0, "ALL"), ("cpg", 12, "Fam17"), ("addchr", 0, "ALL"),
                                             ("sidechan", 0, "ALL")])
def test_sort_key_reproduces_the_file_order(lib, case, field, name):
    tm = gc.build_table_model(case, field, name)
    first_seen = list(dict.fromkeys(tm.chrom_names[c] for c in tm.chrom))
    rank = {nm: k for k, nm in enumerate(refio.kent_hash_order(first_seen))}
    keys = [lib.itxl_key(rank[tm.chrom_names[c]], lib.itxl_bin(r["start"], r["end"])) for c, r in zip(tm.chrom, tm.rows)]
    order = sorted(range(len(tm.rows)), key=lambda k: (keys[k], -k))
    assert order == gc.loci_row_order(tm) and len(order) > 5
