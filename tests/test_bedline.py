"""The bed line of `stat -B / -V` (iteres_amd/csrc/itx_bedline.h, the rule csrc/itx_bed.hip runs per record) built for the host
(tests/bedline_host.cpp) against lines formatted by Python's own `%` from an independent reading of the records
(tests/bedcase.py): names of length 0, 1 and 254, a name with a NUL inside, MAPQ 0 and 255, coordinates of 1 to 10 digits, every
NM type, XA absent / empty / kilobytes long / without its NUL / of a type that is no string / behind a float the reference's walk
gets lost in (tests/auxmodel.py), a B array before XA, -C names; and
every line laid down in pieces of 1, 7 and 64 bytes, as the device lays it down window by window."""
import ctypes as C
import os
import subprocess

import pytest

import bedcase as bc
import goldencase as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = [("chr1", 2147483647), ("MT", 16571), ("GL000191.1", 106433), ("1", 2147483647)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bedline") / "libbedline_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, os.path.join(ROOT, "tests", "bedline_host.cpp")])
    L = C.CDLL(so)
    L.itxb_line_host.restype = C.c_longlong
    L.itxb_line_host.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32]
    return L


def host_line(lib, rec, chrom, start, end, mapq, strand, with_xa, piece):
    cap = len(rec) + len(chrom) + 128
    out = C.create_string_buffer(cap)
    n = lib.itxb_line_host(rec, chrom, len(chrom), start, end, mapq, 1 if strand == "-" else 0, int(with_xa), out, cap, piece)
    assert 0 < n <= cap
    assert out.raw[n:] == b"\xaa" * (cap - n), "wrote past the line"
    return out.raw[:n]


@pytest.mark.parametrize("add_chr", [False, True], ids=["names-as-they-are", "-C"])
@pytest.mark.parametrize("opt", [dict(), dict(extension=0), dict(treat_pe_as_se=True), dict(mapq_min=0)], ids=["default", "E0", "T", "Q0"])
def test_lines_equal_python_formatting(lib, opt, add_chr):
    p = bc.params(**opt)
    recs = bc.corner_records()
    names = [gc.rename_chr(n, add_chr) for n, _ in HEADER]
    chrom_names = [n for n in dict.fromkeys(names) if n is not None]
    sizes = [next(l for (h, l), nm in zip(HEADER, names) if nm == c) for c in chrom_names]
    want_b, want_v, t2c, names = bc.lines(p, HEADER, chrom_names, sizes, recs, add_chr)
    rd, arr = bc.soa(recs)
    n_lines = 0
    for piece in (0, 1, 7, 64):
        got_b, got_v = [], []
        for i, (rec, r) in enumerate(zip(recs, rd)):
            d = gc.derive_py(p, t2c, sizes, arr, i)
            if d is None:
                continue
            chrom = names[r["tid"]].encode()
            got_b.append(host_line(lib, rec, chrom, d[0], d[1], r["mapq"], d[2], True, piece))
            if r["mapq"] >= p["mapq_min"]:
                got_v.append(host_line(lib, rec, chrom, d[0], d[1], r["mapq"], d[2], False, piece))
        n_lines = len(got_b)
        assert b"".join(got_b) == want_b, piece
        assert b"".join(got_v) == want_v, piece
    assert n_lines > 50 and want_b.count(b"\n") == n_lines
    if add_chr:
        assert b"chrM\t" in want_b and b"chr1\t" in want_b and b"GL0" not in want_b
    else:
        assert b"MT\t" in want_b and b"GL000191.1\t" in want_b and b"\n1\t" in want_b


def test_expected_text_has_the_corners_in_it():
    """the Python side really holds what the case list promises (so that equality above means something)"""
    p = bc.params(extension=0)
    want_b, want_v, _, _ = bc.lines(p, HEADER, [n for n, _ in HEADER], [l for _, l in HEADER], bc.corner_records())
    for piece in (b"\t\t37\t", b"\ta\t", b"\t" + b"q" * 254 + b"\t", b"\tab\t", b"\t0\t-", b"\t255\t-", b"\t2147483647\t", b"\t0\t1\tp0\t", b"\t-5\tchr1,", b"\t200\t",
                  b"\t-30000\t", b"\t65535\t", b"\t-2147483648\t", b"\t-294967296\t", b"\t2147483647\tchr1,", b"\t+\t0\t\n", b"\t603\t653\tr1\t37\t+\t2\t\n", b"\t4\t\n",
                  b"\t300\tafter,+1,2M,0;\n", b"\t0\t1AE301\n"):
        assert piece in want_b, piece
    assert b"unreachable" not in want_b and b"behind an unknown" not in want_b and b"\tun\t" not in want_b
    assert b"no terminating NUL" not in want_b                      # a string that runs out of its record reads as empty
    assert b"\t500\t550\tr1\t37\t+\n" in want_b                      # XA behind NM:f: the reference walks into the float and never finds it
    assert max(len(l) for l in want_b.split(b"\n")) > 5000
    assert b"chr1," not in want_v and 0 < want_v.count(b"\n") < want_b.count(b"\n")


def test_a_name_that_runs_out_of_its_record_is_for_the_host(lib):
    rec = bc.record(qname=b"abc", cigar=(), l_qseq=0)
    out = C.create_string_buffer(256)
    assert lib.itxb_line_host(rec, b"chr1", 4, 1, 2, 3, 0, 1, out, 256, 0) == -1
