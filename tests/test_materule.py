"""The mates rule of `filter -b -s -m` (iteres_amd/csrc/itx_materule.h, what csrc/itx_bamout_mates.hip runs on the device and on the host
route) built for the host (tests/materule_host.cpp) and held against the Python statement (tests/matecase.py):
1. wanted / candidate / whole, the hash and the keys over records with every flag bit of the rule set and cleared one at a time, names of
   1 and 254 bytes, tid = -1, pos = -1, records cut short in the fixed part and inside the name;
2. match over every pair of a set with a name that is a prefix of another, two names of equal h32 (found by a birthday search),
   another tid, another pos, another mtid;
3. the header compiles as C;
4. the walk of itx_bamout_mates_append_host's record check;
5. the same inputs through a stand-alone program under -fsanitize=address,undefined, over exact-size heap blocks;
6. the command: -m without -b, without -s and with -T is refused while the options are read, and the usage text lists -m once."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import pytest

import bedcase as bc
import matecase as mc
from iteres_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "materule_host.cpp")
RULE_BITS = (0x1, 0x4, 0x8, 0x40, 0x100, 0x800)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("materule") / "libmaterule_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", so, SRC])
    L = C.CDLL(so)
    L.itxm_eval.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    L.itxm_eval.restype = None
    L.itxm_match.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.itxm_h32.argtypes = [C.c_char_p, C.c_uint32]
    L.itxm_h32.restype = C.c_uint32
    L.itxm_key_cmp.argtypes = [C.c_void_p, C.c_void_p]
    L.itxm_walk.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.itxm_walk.restype = C.c_long
    return L


def test_header_is_valid_c(tmp_path):
    (tmp_path / "t.c").write_text('#include "%s"\nint main(void) { unsigned char r[40] = {36, 0, 0, 0}; size_t nx = 0; r[12] = 2; r[18] = 0x81; r[36] = 65;\n'
                                  '  return itx_mate_candidate(r, 40) && !itx_mate_wanted(r, 35) && itx_mate_h32(r + 36, 1) == %uu && !itx_mate_next(r, 40, 0, &nx) && nx == 40 ? 0 : 1; }\n'
                                  % (os.path.join(ROOT, "iteres_amd", "csrc", "itx_materule.h"), mc.h32(b"A")))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


# ---- 1. the predicates, the hash, the keys

def rec(flag=0x81, tid=2, pos=700, mtid=2, mpos=300, name=b"pair7", l_qname=None, **kw):
    return bc.record(tid=tid, pos=pos, flag=flag, qname=name + b"\0", mtid=mtid, mpos=mpos, cigar=((0, 30),), l_qname=l_qname, **kw)


def py_eval(r, n=None):
    """what itxm_eval returns, by the Python statement"""
    n = len(r) if n is None else n
    out = [int(mc.fixed(r, n)), int(mc.whole(r, n)), int(mc.wanted(r, n)), int(mc.candidate(r, n)), 0, 0, 0, 0, 0]
    if out[1]:
        kc, kw = mc.key_candidate(r), mc.key_wanted(r)
        out[4:] = [kc[2], kc[0], kc[1], kw[0], kw[1]]
    return out


def c_eval(lib, r, n=None):
    n = len(r) if n is None else n
    out = (C.c_int64 * 9)()
    lib.itxm_eval(bytes(r[:n]), n, out)
    return list(out)


def eval_cases():
    """(record bytes, bytes that are there)"""
    cases = []
    for bit in RULE_BITS:                                                  # every bit of the rule set alone, and cleared alone
        cases.append((rec(flag=bit), None))
        cases.append((rec(flag=0x81 | bit), None))
        cases.append((rec(flag=(0x1 | 0x4 | 0x8 | 0x40 | 0x100 | 0x800) & ~bit), None))
        cases.append((rec(flag=0xffff & ~bit), None))
    cases += [(rec(flag=f), None) for f in (0, 0x1, 0x81, 0x41, 0x83, 0x91, 0xa1, 0x63, 0x10, 0x481, 0x281)]
    cases += [(rec(name=b"x"), None), (rec(name=b"n" * 254), None), (rec(name=b""), None), (rec(name=b"pair"), None), (rec(name=b"pair77"), None)]
    cases += [(rec(tid=-1), None), (rec(pos=-1), None), (rec(tid=-1, pos=-1), None), (rec(mtid=-1, mpos=-1, flag=0x41), None), (rec(tid=0, pos=0), None),
              (rec(tid=65535, pos=2**31 - 1), None)]
    whole = rec(name=b"a_name_of_20_bytes__")
    cases += [(whole, n) for n in (0, 3, 4, 20, 35, 36, 37, 36 + 20, 36 + 21, len(whole) - 1)]        # cut short: fixed part, name
    cases.append((rec(flag=0), 36))
    zero = bytearray(rec())
    zero[12] = 0                                                          # l_read_name = 0
    cases.append((bytes(zero), None))
    long_name = bytearray(rec(name=b"ab"))
    long_name[12] = 255                                                    # a name that runs out of block_size
    cases.append((bytes(long_name), None))
    small_bs = bytearray(whole)
    small_bs[0:4] = struct.pack("<I", 32 + 10)                             # block_size ends inside the name, the bytes go on
    cases.append((bytes(small_bs), None))
    return cases


def test_predicates_hash_and_keys(lib):
    seen = set()
    for r, n in eval_cases():
        want = py_eval(r, n)
        assert c_eval(lib, r, n) == want, (r[:40], n)
        seen.add(tuple(want[:4]))
    # the cases reach: nothing, fixed only, whole only, wanted only, candidate only (a READ2 with a mapped mate is both)
    assert {(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1), (1, 0, 1, 0)} <= seen, seen


@pytest.mark.parametrize("bit", RULE_BITS)
def test_each_flag_bit_decides(lib, bit):
    base_w, base_c = 0x41, 0x81                                            # a READ1 counted as a pair; its READ2
    for flag, fn in ((base_w ^ bit, mc.wanted), (base_c ^ bit, mc.candidate)):
        r = rec(flag=flag)
        out = c_eval(lib, r)
        assert out[2] == int(mc.wanted(r)) and out[3] == int(mc.candidate(r))
    assert mc.wanted(rec(flag=base_w)) and mc.candidate(rec(flag=base_c))
    assert mc.wanted(rec(flag=base_w ^ bit)) == (bit not in (0x1, 0x8))
    assert not mc.candidate(rec(flag=base_c ^ bit))                        # every bit of the rule alone takes a candidate out


def test_hash(lib):
    for nm in (b"", b"a", b"A", b"foobar", b"n" * 254, bytes(range(1, 200))):
        assert lib.itxm_h32(nm, len(nm)) == mc.h32(nm)
    assert mc.h32(b"") == 0x811c9dc5 and mc.h32(b"a") == 0xe40c292c and mc.h32(b"foobar") == 0xbf9cf968    # FNV-1a's published vectors


@pytest.fixture(scope="module")
def collision():
    a, b = mc.collide(b"c")
    assert a != b and len(a) == len(b) and mc.h32(a) == mc.h32(b)
    return a, b


def test_key_order(lib):
    keys = [(0, 5, 9), (0, 5, 10), (0, 6, 0), (1, 0, 0), (0xffffffff, 0, 0), (0, 0xffffffff, 1), (3, 3, 0xffffffff), (3, 3, 0)]
    for a, b in itertools.product(keys, keys):
        ka, kb = (C.c_uint32 * 3)(*a), (C.c_uint32 * 3)(*b)
        assert lib.itxm_key_cmp(ka, kb) == (a > b) - (a < b)


# ---- 2. match

def match_set(collision):
    a, b = collision
    r1 = rec(flag=0x41, tid=2, pos=300, mtid=2, mpos=700, name=b"pair7")
    return [r1, rec(), rec(name=b"pair"), rec(name=b"pair77"), rec(name=b"pair8"), rec(tid=3), rec(pos=701), rec(name=b"x"), rec(name=b"n" * 254),
            rec(flag=0x41, tid=2, pos=300, mtid=3, mpos=700, name=b"pair7"), rec(flag=0x41, tid=0, pos=1, mtid=2, mpos=700, name=a), rec(name=a), rec(name=b),
            rec(flag=0x41, mtid=2, mpos=700, name=b"n" * 254), rec(flag=0x41, mtid=2, mpos=700, name=b"x")]


def test_match(lib, collision):
    s = match_set(collision)
    n_true = 0
    for r, c in itertools.product(s, s):
        want = mc.match(r, c)
        assert lib.itxm_match(r, len(r), c, len(c)) == int(want)
        n_true += want
    a, b = collision
    assert mc.match(s[0], s[1]) and not mc.match(s[0], s[2]) and not mc.match(s[0], s[3]) and not mc.match(s[0], s[5]) and not mc.match(s[0], s[6])
    assert mc.match(s[10], s[11]) and not mc.match(s[10], s[12]) and mc.key_candidate(s[11]) == mc.key_candidate(s[12])     # equal keys, other names
    assert n_true >= 5
    cut = s[1]
    for n in (35, 36, 38, len(cut) - 1):                                   # a candidate cut short in the fixed part or the name never matches
        assert lib.itxm_match(s[0], len(s[0]), cut[:n], n) == int(mc.match(s[0], cut, None, n))
    assert not mc.match(s[0], cut, None, 38) and mc.match(s[0], cut, None, 36 + 6)


# ---- 4. the host route's walk

def walk_cases(collision):
    s = match_set(collision)
    whole = b"".join(s)
    liar = bytearray(s[1])
    liar[0:4] = struct.pack("<I", 0x40000000)
    return [whole, whole[:-1], whole + b"\x01\x00", bytes(liar), struct.pack("<I", 20) + bytes(20), struct.pack("<I", 0), b"", whole + struct.pack("<I", 31) + bytes(31),
            s[1] * 3 + s[0]]


def py_walk(b):
    at, n, nc, ksum = 0, 0, 0, 0
    while at < len(b):
        if len(b) - at < 4:
            return -1, 0, 0
        bs, = struct.unpack_from("<I", b, at)
        if bs >= 0x40000000 or bs > len(b) - at - 4:
            return -1, 0, 0
        r = b[at:at + 4 + bs]
        if mc.candidate(r):
            k = mc.key_candidate(r)
            nc += 1
            ksum = (ksum + k[0] * 1000003 + k[1] * 7 + k[2]) & 0xffffffffffffffff
        at += 4 + bs
        n += 1
    return n, nc, ksum


def test_walk(lib, collision):
    got = []
    for b in walk_cases(collision):
        nc, ks = C.c_uint64(0), C.c_uint64(0)
        n = lib.itxm_walk(b, len(b), C.byref(nc), C.byref(ks))
        want = py_walk(b)
        assert (n, nc.value, ks.value) == want if n >= 0 else n == want[0]
        got.append((n, nc.value))
    assert [g[0] for g in got] == [15, -1, -1, -1, 1, 1, 0, 16, 4] and got[0][1] == 10 and got[-1][1] == 3


# ---- 5. the same inputs under the sanitizers

def test_untrusted_bytes_under_asan_and_ubsan(lib, collision, tmp_path):
    exe = str(tmp_path / "materule_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DITX_MATERULE_MAIN", "-o", exe,
                           SRC])
    s = match_set(collision)
    want = []
    n_cases = 0
    with open(tmp_path / "cases.bin", "wb") as f:
        for r, n in eval_cases():
            n = len(r) if n is None else n
            f.write(b"E" + struct.pack("<I", n) + r[:n])
            want.append("E " + " ".join(str(v) for v in py_eval(r, n)))
            n_cases += 1
        for r, c in itertools.product(s, s):
            f.write(b"M" + struct.pack("<II", 4 + len(r) + len(c), len(r)) + r + c)
            want.append("M %d" % mc.match(r, c))
            n_cases += 1
        for n in (0, 3, 35, 36, 38, 41):                                   # both sides cut short
            f.write(b"M" + struct.pack("<II", 4 + n + n, n) + s[0][:n] + s[1][:n])
            want.append("M %d" % mc.match(s[0], s[1], n, n))
            n_cases += 1
        for b in walk_cases(collision):
            f.write(b"W" + struct.pack("<I", len(b)) + b)
            n, nc, ks = py_walk(b)
            want.append("W %d %d %d" % (n, nc, ks) if n >= 0 else None)
            n_cases += 1
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stderr.decode().strip() == "%d cases" % n_cases
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(want)
    for got, w in zip(lines, want):
        assert got == w if w is not None else got.startswith("W -1 ")


# ---- 6. the command

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


@pytest.mark.parametrize("opts,words", [(("-m",), ("-m", "without -b")), (("-m", "-s"), ("without -b",)), (("-m", "-b"), ("-m", "without -s")),
                                        (("-m", "-b", "-i"), ("-m", "without -s")), (("-m", "-b", "-s", "-T"), ("-m", "-T"))])
def test_m_is_refused_while_the_options_are_read(exe, tmp_path, opts, words):
    r = subprocess.run([exe, "filter"] + list(opts) + ["-o", "out", "a", "b", "c", "d"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 255 and all(w in r.stderr for w in words), r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
    assert "Start to parse" not in r.stderr and os.listdir(tmp_path) == []


def test_usage_lists_m_once(exe):
    r = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stderr.splitlines() if l.strip().startswith("-m ")]
    assert r.returncode == 1 and len(lines) == 1 and "with -b -s" in lines[0] and "extension" in lines[0]
    assert not {"-l", "-i", "-a"} & set(lines[0].split())
