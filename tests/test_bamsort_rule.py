"""The coordinate order of `filter -b -s` (iteres_amd/csrc/itx_bamsortrule.h, what csrc/itx_bamout_sort.hip, csrc/itx_bamout.hip and host/out_bam.c run) built
for the host (tests/bamsortrule_host.cpp) and held against a Python parse of the record and a Python restatement of the header rule:
1. the key: both strands at one position, pos 0 and 2^31 - 1, tid 0 and 65 535, tid = -1 and pos = -1 reported, the passes over tid;
2. the header text: with and without @HD, SO / GO / SS dropped wherever they stand, trailing NULs and every later line untouched;
3. the header compiles as C;
4. the pieces that take untrusted bytes, as a stand-alone program under -fsanitize=address,undefined over the same inputs;
5. the command: -s without -b is refused while the options are read, and the usage text lists -s once."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import bedcase as bc
from iteres_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bamsortrule_host.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bamsortrule") / "libbamsortrule_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", so, SRC])
    L = C.CDLL(so)
    L.itxs_key.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    L.itxs_high_passes.argtypes = [C.c_uint32]
    L.itxs_high_passes.restype = C.c_uint32
    L.itxs_header_growth.restype = C.c_uint32
    L.itxs_header_text.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    L.itxs_header_text.restype = C.c_size_t
    L.itxs_walk.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    L.itxs_walk.restype = C.c_long
    return L


def test_header_is_valid_c(tmp_path):
    (tmp_path / "t.c").write_text('#include "%s"\nint main(void) { char o[64]; return itx_bamsort_header_text("", 0, o) == 25 && itx_bamsort_high_passes(257) == 2 ? 0 : 1; }\n'
                                  % os.path.join(ROOT, "iteres_amd", "csrc", "itx_bamsortrule.h"))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


# ---- 1. the key

def py_key(rec):
    """(tid, pos, reverse) parsed from the record's bytes with struct alone"""
    bs, tid, pos, l_name, mapq, bn, n_cigar, flag = struct.unpack_from("<IiiBBHHH", rec, 0)
    assert bs + 4 == len(rec)
    return tid, pos, (flag >> 4) & 1


def key(lib, rec):
    out = (C.c_int64 * 5)()
    bad = lib.itxs_key(rec, len(rec), out)
    return bad, tuple(out)


KEY_CASES = [(0, 1000, 0), (0, 1000, 16), (0, 1000, 16 | 1 | 64), (0, 1000, 32), (0, 0, 0), (0, 0, 16), (0, 2**31 - 1, 0), (0, 2**31 - 1, 16), (65535, 5, 16), (65535, 2**31 - 1, 0),
             (7, 123456789, 0x7ef), (7, 123456789, 0xffef)]


@pytest.mark.parametrize("tid,pos,flag", KEY_CASES)
def test_key(lib, tid, pos, flag):
    rec = bc.record(tid=tid, pos=pos, flag=flag, qname=b"name\0", cigar=((0, 30),))
    want = py_key(rec)
    assert want == (tid, pos, (flag >> 4) & 1)
    bad, (t, p, r, low, high) = key(lib, rec)
    assert bad == 0 and (t, p, r) == want
    assert low == (pos << 1 | want[2]) & 0xffffffff == pos * 2 + want[2] and high == tid


def test_both_strands_at_one_position_order_forward_first(lib):
    fwd = key(lib, bc.record(tid=3, pos=77, flag=0))[1]
    rev = key(lib, bc.record(tid=3, pos=77, flag=16))[1]
    nxt = key(lib, bc.record(tid=3, pos=78, flag=0))[1]
    assert (fwd[4], fwd[3]) < (rev[4], rev[3]) < (nxt[4], nxt[3])


@pytest.mark.parametrize("tid,pos", [(-1, 5), (3, -1), (-1, -1), (-2, 0)])
def test_unmapped_keys_are_reported(lib, tid, pos):
    bad, (t, p, r, low, high) = key(lib, bc.record(tid=tid, pos=pos))
    assert bad == 1 and (t, p) == (tid, pos)


def test_a_record_without_a_fixed_part_is_reported(lib):
    short = struct.pack("<I", 31) + bytes(31)
    assert key(lib, short)[0] == 1 and key(lib, struct.pack("<I", 0))[0] == 1
    assert key(lib, struct.pack("<I", 32) + bytes(32))[0] == 0              # tid 0, pos 0


def test_passes_over_tid(lib):
    """ceil(bits(n_ref - 1) / 8)"""
    for n_ref, want in [(0, 0), (1, 0), (2, 1), (256, 1), (257, 2), (65536, 2), (65537, 3), (1 << 24, 3), ((1 << 24) + 1, 4), (2**31 - 1, 4)]:
        assert lib.itxs_high_passes(n_ref) == want == -(-max(n_ref - 1, 0).bit_length() // 8), n_ref


# ---- 2. the header text

def py_header(text):
    """the rule restated: bytes -> bytes"""
    ends = [i for i in (text.find(b"\n"), text.find(b"\0")) if i >= 0]
    eol = min(ends) if ends else len(text)
    line, rest = text[:eol], text[eol:]
    fields = line.split(b"\t")
    if fields[0] != b"@HD":
        return b"@HD\tVN:1.6\tSO:coordinate\n" + text
    kept = [f for f in fields[1:] if f[:3] not in (b"SO:", b"GO:", b"SS:")]
    return b"\t".join([b"@HD"] + kept + [b"SO:coordinate"]) + rest


SQ = b"@SQ\tSN:chr1\tLN:1000\n@PG\tID:bwa\tPN:bwa\n"
HEADER_CASES = {
    "no_hd": (SQ, b"@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    "empty": (b"", b"@HD\tVN:1.6\tSO:coordinate\n"),
    "only_nuls": (b"\0\0\0", b"@HD\tVN:1.6\tSO:coordinate\n\0\0\0"),
    "vn_1_0": (b"@HD\tVN:1.0\n" + SQ, b"@HD\tVN:1.0\tSO:coordinate\n" + SQ),
    "so_in_the_middle": (b"@HD\tVN:1.5\tSO:unsorted\tXY:z\n" + SQ, b"@HD\tVN:1.5\tXY:z\tSO:coordinate\n" + SQ),
    "so_at_the_end": (b"@HD\tVN:1.5\tSO:unsorted\n" + SQ, b"@HD\tVN:1.5\tSO:coordinate\n" + SQ),
    "so_coordinate_already": (b"@HD\tVN:1.6\tSO:coordinate\n" + SQ, b"@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    "go_and_ss": (b"@HD\tVN:1.6\tGO:query\tSS:queryname:natural\tAB:c\n" + SQ, b"@HD\tVN:1.6\tAB:c\tSO:coordinate\n" + SQ),
    "so_go_ss_all": (b"@HD\tSO:queryname\tVN:1.6\tGO:none\tSS:unsorted:x\n", b"@HD\tVN:1.6\tSO:coordinate\n"),
    "hd_only_line": (b"@HD\tVN:1.4\tSO:unknown\n", b"@HD\tVN:1.4\tSO:coordinate\n"),
    "hd_only_line_no_newline": (b"@HD\tVN:1.4\tSO:unknown", b"@HD\tVN:1.4\tSO:coordinate"),
    "bare_hd": (b"@HD\n" + SQ, b"@HD\tSO:coordinate\n" + SQ),
    "trailing_nuls": (b"@HD\tVN:1.6\tSO:unsorted\n" + SQ + b"\0\0\0\0\0", b"@HD\tVN:1.6\tSO:coordinate\n" + SQ + b"\0\0\0\0\0"),
    "nuls_right_behind_hd": (b"@HD\tVN:1.6\0\0", b"@HD\tVN:1.6\tSO:coordinate\0\0"),
    "no_hd_trailing_nuls": (SQ + b"\0\0", b"@HD\tVN:1.6\tSO:coordinate\n" + SQ + b"\0\0"),
    "co_line_with_so": (b"@HD\tVN:1.6\n@CO\tSO:unsorted\tGO:query\n" + SQ, b"@HD\tVN:1.6\tSO:coordinate\n@CO\tSO:unsorted\tGO:query\n" + SQ),
    "co_line_with_so_no_hd": (b"@CO\tSO:unsorted\n" + SQ, b"@HD\tVN:1.6\tSO:coordinate\n@CO\tSO:unsorted\n" + SQ),
    "hdx_is_no_hd": (b"@HDX\tVN:1.6\n", b"@HD\tVN:1.6\tSO:coordinate\n@HDX\tVN:1.6\n"),
    "tag_that_only_starts_like_so": (b"@HD\tVN:1.6\tSOX:1\tSO\n", b"@HD\tVN:1.6\tSOX:1\tSO\tSO:coordinate\n"),
}


def header_text(lib, text):
    out = C.create_string_buffer(len(text) + lib.itxs_header_growth())
    n = lib.itxs_header_text(text, len(text), out)
    assert n == lib.itxs_header_text(text, len(text), None) <= len(text) + lib.itxs_header_growth()
    return out.raw[:n]


@pytest.mark.parametrize("name", list(HEADER_CASES))
def test_header_text(lib, name):
    text, want = HEADER_CASES[name]
    assert py_header(text) == want, "the restatement disagrees with the case"
    assert header_text(lib, text) == want


def test_header_text_is_idempotent(lib):
    for text, want in HEADER_CASES.values():
        assert header_text(lib, want) == want


# ---- 4. the same inputs through the stand-alone program under the sanitizers

def test_untrusted_bytes_under_asan_and_ubsan(lib, tmp_path):
    """exact-size heap blocks for every input and output: the header cases, and record bytes as append_host walks them in sort
    mode: whole records, a ragged end, a block_size that lies, a record shorter than its fixed part"""
    exe = str(tmp_path / "bamsortrule_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DITX_BAMSORT_MAIN", "-o", exe,
                           SRC])
    recs = [bc.record(tid=t, pos=p, flag=f, qname=b"q\0", cigar=((0, 30),)) for t, p, f in KEY_CASES] + [bc.record(tid=-1, pos=-1)]
    whole = b"".join(recs)
    liar = bytearray(recs[0])
    liar[0:4] = struct.pack("<I", 0x40000000)
    record_cases = [whole, whole[:-1], whole + b"\x01\x00", bytes(liar), struct.pack("<I", 20) + bytes(20), struct.pack("<I", 0), b"", whole + struct.pack("<I", 31) + bytes(31)]
    with open(tmp_path / "cases.bin", "wb") as f:
        for text, _ in HEADER_CASES.values():
            f.write(b"H" + struct.pack("<I", len(text)) + text)
        for b in record_cases:
            f.write(b"R" + struct.pack("<I", len(b)) + b)
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stderr.decode().strip() == "%d cases" % (len(HEADER_CASES) + len(record_cases))
    want = b"".join(w for _, w in HEADER_CASES.values())
    for b in record_cases:
        s = C.c_uint64(0)
        n = lib.itxs_walk(b, len(b), C.byref(s))
        want += b"%d %d\n" % (n, s.value)
    assert r.stdout == want
    walked = [int(l.split()[0]) for l in r.stdout[len(b"".join(w for _, w in HEADER_CASES.values())):].splitlines()]
    assert walked == [len(recs), -1, -1, -1, 1, 1, 0, len(recs) + 1]


# ---- 5. the command

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


def test_s_without_b_is_refused_while_the_options_are_read(exe, tmp_path):
    r = subprocess.run([exe, "filter", "-s", "-o", "out", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and "-s" in r.stderr and "without -b" in r.stderr
    assert "Start to parse" not in r.stderr and os.listdir(tmp_path) == []
    r = subprocess.run([exe, "filter", "-s", "-i", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and os.listdir(tmp_path) == []
    for extra, env in ((("-S",), {}), ((), {"ITX_HOST_INFLATE": "1"})):      # -b's own refusals cover -b -s
        r = subprocess.run([exe, "filter", "-s", "-b"] + list(extra) + ["a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120,
                           env=dict(os.environ, **env))
        assert r.returncode == 255 and "-b" in r.stderr and os.listdir(tmp_path) == []


def test_usage_lists_s_once(exe):
    r = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stderr.splitlines() if l.strip().startswith("-s ")]
    assert r.returncode == 1 and len(lines) == 1 and "with -b" in lines[0] and "coordinate" in lines[0]
