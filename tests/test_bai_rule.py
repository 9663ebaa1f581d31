"""The rule a record follows into the .bai index of `filter -b -i` (iteres_amd/csrc/itx_bairule.h, what csrc/itx_bamidx.hip runs per
record) built for the host (tests/bairule_host.cpp) and held against the Python restatement (tests/baicase.py):
1. reg2bin at every level boundary +- 1; 2. the end of a record for every kind of CIGAR operation, an all-zero CIGAR and none;
3. the limit 2^29 and the reference's length; 4. virtual offsets, a record that ends exactly on a payload boundary among them;
5. the restatement's own reader finds what a linear scan finds (so the GPU tests can lean on it);
6. the command: -i without -b is refused while the options are read, and the usage text lists -i. It also compiles as C."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import baicase as bai
import bedcase as bc
from iteres_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bairule") / "libbairule_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", so, os.path.join(ROOT, "tests", "bairule_host.cpp")])
    L = C.CDLL(so)
    L.itxb_reg2bin.argtypes = [C.c_int64, C.c_int64]
    L.itxb_reg2bin.restype = C.c_uint32
    L.itxb_record.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
    L.itxb_win_first.argtypes = [C.c_int32]
    L.itxb_win_first.restype = C.c_uint32
    L.itxb_win_last.argtypes = [C.c_int64]
    L.itxb_win_last.restype = C.c_uint32
    L.itxb_windows.argtypes = [C.c_int32]
    L.itxb_windows.restype = C.c_uint32
    L.itxb_voff.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32]
    L.itxb_voff.restype = C.c_uint64
    return L


def fields(lib, rec, l_ref):
    out = (C.c_int64 * 4)()
    lr = (C.c_int32 * len(l_ref))(*l_ref)
    why = lib.itxb_record(rec, len(rec), len(l_ref), lr, out)
    return why, tuple(out)


def test_header_is_valid_c(tmp_path):
    (tmp_path / "t.c").write_text('#include "%s"\nint main(void) { return (int)itx_bai_reg2bin(0, 1) == 4681 ? 0 : 1; }\n'
                                  % os.path.join(ROOT, "iteres_amd", "csrc", "itx_bairule.h"))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_reg2bin_at_the_level_boundaries(lib):
    n = 0
    for shift in (14, 17, 20, 23, 26):
        for k in (1, 2, 3, (1 << (29 - shift)) - 1):
            edge = k << shift
            for beg in (edge - 2, edge - 1, edge, edge + 1):
                for end in (beg + 1, edge - 1, edge, edge + 1, edge + 2, beg + (1 << shift), beg + (1 << shift) + 1, 1 << 29):
                    if 0 <= beg < end <= 1 << 29:
                        assert lib.itxb_reg2bin(beg, end) == bai.reg2bin(beg, end), (beg, end)
                        assert bai.reg2bin(beg, end) in bai.reg2bins(beg, end)
                        n += 1
    assert n > 500
    assert lib.itxb_reg2bin(0, 1) == 4681 and lib.itxb_reg2bin(0, 1 << 29) == 0 and lib.itxb_reg2bin((1 << 29) - 1, 1 << 29) == 37448
    assert lib.itxb_reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585 and lib.itxb_reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0


M, I, D, N, S, H, P, EQ, X = range(9)


@pytest.mark.parametrize("cigar,ref", [
    (((M, 50),), 50), (((EQ, 30), (X, 2), (EQ, 8)), 40), (((S, 5), (M, 20), (I, 3), (M, 10), (S, 7)), 30), (((H, 9), (M, 10), (D, 4), (M, 6), (H, 2)), 20),
    (((M, 10), (P, 6), (M, 10)), 20), (((M, 10), (N, 100000), (M, 10)), 100020), (((S, 30),), 0), (((I, 12), (P, 3), (H, 1)), 0), (((M, 0), (D, 0)), 0), ((), 0),
    (((M, (1 << 28) - 1),), (1 << 28) - 1)])
def test_end_of_a_record(lib, cigar, ref):
    rec = bc.record(tid=2, pos=777, qname=b"read/1\0", cigar=cigar, aux=bc.tag("ZZ", "Z", b"xyz\0"))
    why, (tid, pos, n_cigar, end) = fields(lib, rec, [1 << 30] * 3)
    assert (why, tid, pos, n_cigar) == (0, 2, 777, len(cigar))
    assert end == 777 + (ref or 1) == bai.record_fields(rec, 0)[2]
    assert lib.itxb_win_first(pos) == 0 and lib.itxb_win_last(end) == (end - 1) >> 14


def test_the_records_own_bin_field_is_not_used(lib):
    rec = bytearray(bc.record(tid=0, pos=20000, cigar=((M, 10),)))
    rec[14:16] = struct.pack("<H", 1234)
    why, (tid, pos, n_cigar, end) = fields(lib, bytes(rec), [100000])
    assert why == 0 and lib.itxb_reg2bin(pos, end) == 4682


def test_limits(lib):
    top = 1 << 29
    at_top = bc.record(tid=0, pos=top - 10, cigar=((M, 10),))
    beyond = bc.record(tid=0, pos=top - 10, cigar=((M, 11),))
    assert fields(lib, at_top, [1 << 30])[0] == bai.OK and fields(lib, at_top, [top])[0] == bai.OK
    assert fields(lib, beyond, [1 << 30]) == (bai.BEYOND_MAX, (0, top - 10, 1, top + 1))
    assert fields(lib, at_top, [top - 1])[0] == bai.BEYOND_REF
    one = bc.record(tid=1, pos=99, cigar=((S, 10),))                       # no reference bases: [99, 100)
    assert fields(lib, one, [500, 100])[0] == bai.OK and fields(lib, one, [500, 99])[0] == bai.BEYOND_REF
    assert fields(lib, one, [500])[0] == bai.BEYOND_REF                    # names no reference of the header
    assert fields(lib, bc.record(tid=-1, pos=-1), [500])[0] == bai.BEYOND_REF
    assert fields(lib, bc.record(tid=0, pos=-1), [500])[0] == bai.BEYOND_REF
    # a CIGAR that claims more operations than the record holds is cut at the record's end
    liar = bytearray(bc.record(tid=0, pos=5, qname=b"q\0", cigar=((M, 7),)))
    liar[16:18] = struct.pack("<H", 60000)
    assert fields(lib, bytes(liar), [1 << 20])[1][2] == 1
    assert [lib.itxb_windows(v) for v in (-5, 0, 1, 16384, 16385, top, 2**31 - 1)] == [0, 0, 1, 1, 2, 32768, 32768]


def test_virtual_offsets(lib):
    P = bai.PAYLOAD
    sizes = [700, 650, 9000, 28]
    coff = np.cumsum([0] + sizes).astype(np.uint64)
    F = 12345

    def v(s):
        return lib.itxb_voff(F, coff.ctypes.data, s, P)
    assert v(0) == F << 16 and v(1) == (F << 16) + 1 and v(P - 1) == (F << 16) + P - 1
    assert v(P) == (F + 700) << 16                                         # the last byte of a payload, then the next member's first
    assert v(3 * P + 17) == (F + 700 + 650 + 9000) << 16 | 17
    # a record that ends exactly on the last payload's boundary ends where whatever follows the members starts
    assert v(4 * P) == (F + sum(sizes)) << 16
    # the restatement agrees: four records of P bytes in four members
    pad = P - len(bc.record(cigar=((M, 5),), aux=bc.tag("ZZ", "Z", b"\0")))
    recs = [bc.record(tid=0, pos=10 * i, cigar=((M, 5),), aux=bc.tag("ZZ", "Z", b"A" * pad + b"\0")) for i in range(4)]
    assert all(len(r) == P for r in recs)
    st, idx = bai.expected([1000], b"".join(recs), sizes, F)
    assert st == bai.OK
    chunks = bai.parse_bai(idx)[0]["bins"][4681]
    assert chunks == [(v(0), v(4 * P))] and bai.parse_bai(idx)[0]["meta"] == (v(0), v(4 * P), 4, 0)


def test_restatement_reader_against_a_linear_scan():
    """no product code: the restatement's index, read back by its own reader, fetches what walking every record finds"""
    rng = np.random.default_rng(5)
    l_ref = [3_000_000, 50_000, 2_000_000]
    recs = []
    for tid in (0, 2):
        pos = np.sort(rng.integers(0, l_ref[tid] - 300_000, 3000))
        for i, p in enumerate(pos):
            cig = ((M, 40), (N, int(rng.integers(1000, 250_000))), (M, 30)) if i % 97 == 0 else ((M, int(rng.integers(20, 150))),)
            recs.append(bc.record(tid=tid, pos=int(p), qname=b"r%d\0" % i, cigar=cig))
    stream = b"".join(recs)
    n_mem = -(-len(stream) // bai.PAYLOAD)
    sizes = [int(x) for x in rng.integers(500, 3000, n_mem)]
    F = 4321
    st, idx = bai.expected(l_ref, stream, sizes, F)
    assert st == bai.OK
    coff = np.cumsum([0] + sizes)
    ustart = {F + int(coff[k]): min(k * bai.PAYLOAD, len(stream)) for k in range(n_mem + 1)}
    parsed = bai.parse_bai(idx)
    assert parsed[1] == {"bins": {}, "meta": None, "lin": []} and parsed[0]["meta"][2] == 3000
    hits = 0
    for k in range(120):
        tid = (0, 2, 1)[k % 3]
        beg = int(rng.integers(0, l_ref[tid] - 1))
        end = min(beg + int(rng.integers(1, 40_000)), l_ref[tid])
        got = bai.fetch(parsed, stream, ustart, tid, beg, end)
        assert got == bai.linear_scan(stream, 0, tid, beg, end)
        hits += bool(got)
    assert hits >= 60


@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


def test_i_without_b_is_refused_while_the_options_are_read(exe, tmp_path):
    r = subprocess.run([exe, "filter", "-i", "-o", "out", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and "-i" in r.stderr and "without -b" in r.stderr
    assert "Start to parse" not in r.stderr and os.listdir(tmp_path) == []
    r = subprocess.run([exe, "filter", "-i", "-b", "-S", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and os.listdir(tmp_path) == []


def test_usage_lists_i(exe):
    r = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stderr.splitlines() if l.strip().startswith("-i ")]
    assert r.returncode == 1 and len(lines) == 1 and ".bam.bai" in lines[0]
