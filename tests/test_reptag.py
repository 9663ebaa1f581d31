"""The tags of `filter -b -a` (iteres_amd/csrc/itx_reptag.h, what k_bo_gather<.., true> of csrc/itx_bamout.hip and the host route of
host/out_bam.c lay behind a counted record) built for the host (tests/reptag_host.cpp) and held against the Python restatement
(tests/reptagcase.py):
1. whole records: every name length in every position, the coordinates' edge values, records from 36 to 70 000 bytes, seeded pairs;
2. the piecewise writer: every (from, to) of a short record, every pair of cuts near a field boundary of a long one, guard bytes;
3. the header compiles as C; the stand-alone program (the form the sanitizer run of DESIGN.md uses) passes its own cases;
4. the command: -a without -b is refused while the options are read, -b's refusals cover -b -a, the usage text lists -a once;
5. the ABI: itx_bamout_annotate_enable(NULL, ...) is ITX_E_ARG without a device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bedcase as bc
import reptagcase as rt
from iteres_amd import build, engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "reptag_host.cpp")
HEADER = os.path.join(ROOT, "iteres_amd", "csrc", "itx_reptag.h")
GUARD = 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("reptag") / "libreptag_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", so, SRC])
    L = C.CDLL(so)
    L.itxr_len.argtypes = [C.c_uint32] * 3
    L.itxr_len.restype = C.c_uint32
    L.itxr_piece.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                             C.c_void_p]
    L.itxr_piece.restype = None
    L.itxr_check_pairs.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                   C.c_uint32, C.c_char_p]
    L.itxr_check_pairs.restype = C.c_long
    return L


def piece(lib, rec, row, a, b):
    """bytes [a, b) of the annotated record by the host build, written between guard bytes that must survive"""
    rep, cla, fam, start, end = row
    buf = C.create_string_buffer(b"\xa5" * (b - a + 2 * GUARD), b - a + 2 * GUARD)
    lib.itxr_piece(rec, len(rec), rep, len(rep), cla, len(cla), fam, len(fam), start, end, a, b, C.addressof(buf) + GUARD)
    raw = buf.raw
    assert raw[:GUARD] == b"\xa5" * GUARD and raw[GUARD + b - a:] == b"\xa5" * GUARD, (a, b)
    return raw[GUARD:GUARD + b - a]


def whole(lib, rec, row):
    n = len(rec) + lib.itxr_len(len(row[0]), len(row[1]), len(row[2]))
    return piece(lib, rec, row, 0, n)


def name(n, first):
    return bytes((first + i % 23) for i in range(n))


def record_of(L, i=0):
    """a well-formed record of exactly L >= 36 bytes"""
    if L == 36:                                                            # the fixed part alone: no name, no CIGAR, no sequence
        return check_len(bc.record(tid=i % 3, pos=50 + i, qname=b"", cigar=()), L)
    if L < 60:                                                             # a name and nothing else
        return check_len(bc.record(tid=i % 3, pos=50 + i, qname=b"q" * (L - 37) + b"\0", cigar=()), L)
    pad = L - len(bc.record(tid=i % 3, pos=50 + i, qname=b"r%d\0" % (i % 10), cigar=((0, 10),))) - 4
    return check_len(bc.record(tid=i % 3, pos=50 + i, qname=b"r%d\0" % (i % 10), cigar=((0, 10),), aux=bc.tag("XX", "Z", bytes([66 + i % 20]) * pad + b"\0")), L)


def check_len(r, L):
    assert len(r) == L and struct.unpack_from("<I", r, 0)[0] == L - 4, (len(r), L)
    return r


def test_header_is_valid_c(tmp_path):
    (tmp_path / "t.c").write_text('#include "%s"\nint main(void) { ItxRepTag t; t.rep_len = 1; t.cla_len = 2; t.fam_len = 3; return itx_reptag_len(&t) == 32u ? 0 : 1; }\n' % HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(tmp_path / "t.c")])
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("n", [0, 1, 2, 254, 65535])
@pytest.mark.parametrize("where", [0, 1, 2])
def test_name_lengths_in_each_position(lib, n, where):
    names = [name(3, 65), name(4, 97), name(5, 75)]
    names[where] = name(n, 48)
    row = (names[0], names[1], names[2], 1000, 2000)
    rec = record_of(120)
    assert lib.itxr_len(*(len(x) for x in names)) == 26 + sum(len(x) for x in names) == len(rt.tags(*row))
    assert whole(lib, rec, row) == rt.annotate(rec, *row)


@pytest.mark.parametrize("start", [0, 1, 2**31, 2**32 - 1])
@pytest.mark.parametrize("end", [0, 1, 2**31, 2**32 - 1])
def test_coordinates_are_uint32_whatever_their_value(lib, start, end):
    row = (b"AluY", b"SINE", b"Alu", start, end)
    rec = record_of(77)
    got = whole(lib, rec, row)
    assert got == rt.annotate(rec, *row) and len(got) == 77 + 26 + 11
    assert got[-14:] == b"ZSI" + struct.pack("<I", start) + b"ZEI" + struct.pack("<I", end)
    assert rt.strip(got) == (rec, row)


@pytest.mark.parametrize("L", [36, 37, 43, 44, 100, 8191, 8192, 8193, 32768, 70000])
def test_record_sizes(lib, L):
    row = (b"L1PA2", b"LINE", b"L1", 123456, 234567)
    rec = record_of(L, L)
    got = whole(lib, rec, row)
    assert got == rt.annotate(rec, *row)
    assert got[4:L] == rec[4:] and struct.unpack_from("<I", got, 0)[0] == len(got) - 4 == L - 4 + 26 + 11
    assert rt.strip(got) == (rec, row)                                      # the way back, by the specification's aux types


def test_seeded_pairs(lib):
    rng = np.random.default_rng(20)
    for k in range(2000):
        L = int(rng.integers(36, 70001)) if k % 100 == 0 else int(rng.integers(36, 400))
        row = (name(int(rng.integers(0, 40)), 65), name(int(rng.integers(0, 12)), 97), name(int(rng.integers(0, 20)), 70), int(rng.integers(0, 2**32)),
               int(rng.integers(0, 2**32)))
        rec = record_of(L, k)
        want = rt.annotate(rec, *row)
        assert whole(lib, rec, row) == want, (k, L)
        a, b = sorted(int(x) for x in rng.integers(0, len(want) + 1, 2))
        assert piece(lib, rec, row, a, b) == want[a:b], (k, a, b)


def pairs(lib, rec, row, cuts):
    rep, cla, fam, start, end = row
    want = rt.annotate(rec, *row)
    c = np.asarray(sorted(set(cuts)), np.uint32)
    n = lib.itxr_check_pairs(rec, len(rec), rep, len(rep), cla, len(cla), fam, len(fam), start, end, c.ctypes.data, len(c), want)
    assert n == len(c) * (len(c) + 1) // 2, n                               # every pair from <= to, guard bytes intact (reptag_host.cpp)
    return n


def test_every_piece_of_a_short_record(lib):
    row = (b"MER5A", b"DNA", b"hAT", 0x01020304, 0xA1B2C3D4)
    rec = record_of(61)
    want = rt.annotate(rec, *row)
    n = len(want)
    assert pairs(lib, rec, row, range(n + 1)) == (n + 1) * (n + 2) // 2
    # and through the single-piece entry, so that the pair checker is not the only witness
    for a in range(0, n + 1, 3):
        for b in (a, a + 1, min(a + 5, n), n):
            if b <= n:
                assert piece(lib, rec, row, a, b) == want[a:b]
    # consecutive pieces concatenate to the whole, wherever they are cut
    for step in (1, 2, 3, 7, 16, 61, 62):
        assert b"".join(piece(lib, rec, row, a, min(a + step, n)) for a in range(0, n, step)) == want


def test_cuts_at_every_field_boundary_of_a_long_record(lib):
    rep, cla, fam = name(254, 65), name(100, 97), name(60, 70)                # (long enough that no two boundaries share their cuts)
    row = (rep, cla, fam, 0x01020304, 0xA1B2C3D4)
    rec = record_of(70000, 7)
    L = len(rec)
    edges = [0, 4, L]                                                       # the end of block_size, the end of the original bytes
    at = L
    for nm in (rep, cla, fam):                                              # each key, each name's end, each NUL
        edges += [at + 3, at + 3 + len(nm), at + 4 + len(nm)]
        at += 4 + len(nm)
    edges += [at + 3, at + 7, at + 10, at + 14]                             # each integer's key and end
    total = L + len(rt.tags(*row))
    assert edges[-1] == total
    cuts = [e + d for e in edges for d in range(-8, 9) if 0 <= e + d <= total]
    assert len(set(cuts)) == 99 and pairs(lib, rec, row, cuts) == 99 * 100 // 2   # (a key's end and its neighbours share cuts: 99 distinct ones)


def test_standalone_program(tmp_path):
    """the program the sanitizer run uses, built plainly here: its own cases pass"""
    exe = str(tmp_path / "reptag_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all as the whole record says" in r.stdout, r.stderr


# ---- the command and the ABI

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


def test_a_without_b_is_refused_while_the_options_are_read(exe, tmp_path):
    r = subprocess.run([exe, "filter", "-a", "-o", "out", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and "-a" in r.stderr and "without -b" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    assert "Start to parse" not in r.stderr and os.listdir(tmp_path) == []
    r = subprocess.run([exe, "filter", "-a", "-S", "-b", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and "-S" in r.stderr and os.listdir(tmp_path) == []
    r = subprocess.run([exe, "filter", "-a", "-b", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120, env=dict(os.environ, ITX_HOST_INFLATE="1"))
    assert r.returncode == 255 and "ITX_HOST_INFLATE" in r.stderr and os.listdir(tmp_path) == []


def test_usage_lists_a_once(exe):
    r = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True, timeout=120)
    lines = [ln.strip() for ln in r.stderr.splitlines()]
    mine = [ln for ln in lines if ln.startswith("-a ")]
    assert r.returncode == 1 and len(mine) == 1 and "with -b" in mine[0] and "extension" in mine[0]
    assert not {"-l", "-s", "-i"} & set(mine[0].split())
    for opt, word in (("-b ", ".iteres.bam"), ("-i ", ".bam.bai"), ("-s ", "coordinate"), ("-l ", "level")):
        assert len([ln for ln in lines if ln.startswith(opt) and word in ln]) == 1, opt


def test_annotate_enable_null_object_is_an_argument_error():
    L = eng.load()
    off = (C.c_uint64 * 2)(0, 1)
    assert L.itx_bamout_annotate_enable(None, None, 0, b"a", off, 1, b"b", off, 1, b"c", off, 1) == -1
    assert b"itx_bamout_annotate_enable" in L.itx_last_error()
    n = C.c_uint64(7)
    assert L.itx_bamout_annotate_get_stats(None, C.byref(n)) == -1
