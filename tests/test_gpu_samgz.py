"""GPU: SAM text that arrives as BGZF, inflated and parsed on the device (include/iteres_amd.h itx_samtext_parse_begin_bgzf, _bgzf_info,
_text, _strings; csrc/itx_samtext.hip, the decoder: csrc/itx_inflate.hip).
1. the ABI: every chunk against the plain entry (itx_samtext_parse_begin) on the same text in the other slot, record array by record array, and
   against the text itself read back; the carry between two chunks; the header skipped; the strings gathered on the device against slices of
   the text; a damaged member; argument and state checks;
2. the command: a BGZF file through the three routes (the host's reader; the device's parser on text the host inflated; inflated on the device),
   byte-identical outputs; hard lines; the hand-over to the host's zlib reader for what is not BGZF; plain gzip."""
import ctypes as C
import filecmp
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import goldencase as gc
import refio
from iteres_amd import build, engine as eng, synth
from test_samline import XA1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
NAMES = [b"chr1", b"chr2", b"chrX", b"chr2"]
MAX_CHUNK = 8 << 20
ARRAYS = ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize", "line_off", "qname_len", "xa_off", "xa_len", "nm", "xa_mark")


@pytest.fixture(scope="module")
def sam():
    x = eng.SamText(NAMES, MAX_CHUNK)
    yield x
    x.close()


def line(i, seq_len=36, opt=(), flag="0", name=None):
    f = [name or f"q{i}", flag, "chr1" if i % 3 else "chr2", str(1000 + i), "37", f"{seq_len}M", "=", str(2000 + i), str(-i), "A" * seq_len, "I" * seq_len] + list(opt)
    return ("\t".join(f) + "\n").encode()


def line_of(i, total):
    """a plain line of exactly `total` bytes, newline included"""
    base = len(line(i, 30, opt=("ZZ:Z:",)))
    assert total >= base
    out = line(i, 30, opt=("ZZ:Z:" + "z" * (total - base),))
    assert len(out) == total
    return out


def members(text: bytes, payload: int, level: int = 6):
    return [synth.bgzf_block(text[i:i + payload], level) for i in range(0, len(text), payload)]


def body(n, first=0):
    return b"".join(line(i, 30 + i % 40, opt=("NM:i:1", XA1) if i % 4 == 0 else (), flag=("0", "16", "99", "147")[i % 4]) for i in range(first, first + n))


def snapshot(sam, slot, res):
    a = sam.fetch(slot, 0, res["n_rec"])
    return {k: a[k].copy() for k in ARRAYS}


def same_as_plain(sam, slot, text, final, res, arrays):
    """the plain entry on the same text in `slot`: every result field but the times, every record array"""
    want = sam.parse(text, final, slot)
    for k in ("n_lines", "n_rec", "consumed", "n_hard", "first_hard_line", "flags"):
        assert res[k] == want[k], (k, res, want)
    b = sam.fetch(slot, 0, want["n_rec"])
    for k in ARRAYS:
        assert np.array_equal(arrays[k], b[k]), k


def check(sam, comp, text, final=True, slot=0, skip=0, n_members=None):
    """one chunk of a stream of its own: inflated on the device, held against the text and against the plain entry in the other slot"""
    res, info = sam.parse_bgzf(comp, final, slot, skip)
    if n_members is not None:
        assert len(eng.index_bgzf(comp)) == n_members
    assert (info["n_bad"], info["carry_len"], info["text_len"]) == (0, 0, len(text)), info
    assert sam.text(slot) == text
    assert info["tail_len"] == len(text) - res["consumed"]
    a = snapshot(sam, slot, res)
    same_as_plain(sam, 1 - slot, text, final, res, a)
    if not final:
        sam.parse(b"", True, slot)                       # ends the stream: the next chunk has no carry
    return res, info, a


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------------------

TEXT = body(1500)


# (65 536 stored bytes and the 31 bytes around them are more than a member's 16-bit size field holds: that member does not exist)
@pytest.mark.parametrize("payload,level", [(p, l) for p in (1, 100, 0xff00, 65536) for l in (0, 1, 6, 9) if (p, l) != (65536, 0)])
def test_members_of_every_size_and_level(payload, level, sam):
    text = TEXT[:TEXT.find(b"\n", 290) + 1] if payload == 1 else TEXT
    res, _, _ = check(sam, b"".join(members(text, payload, level)), text, slot=level & 1)
    assert res["n_hard"] == 0 and res["n_rec"] == text.count(b"\n")


def test_member_counts_and_odd_members(sam):
    three = line_of(1, 100) + line_of(2, 100) + line_of(3, 100)
    check(sam, b"".join(members(three, 1)), three, n_members=300)
    check(sam, synth.bgzf_block(TEXT[:60000]), TEXT[:60000], final=False, n_members=1)
    tiny = line_of(4, 100) + line_of(5, 100)
    ms = members(tiny, 10)
    assert all(m[18] & 6 == 2 for m in ms)                                # fixed Huffman codes
    check(sam, b"".join(ms), tiny, n_members=20)
    k = 40_000
    comp = b"".join(members(TEXT[:k], 7000)) + synth.bgzf_block(b"") + b"".join(members(TEXT[k:], 7000)) + synth.BGZF_EOF
    res, _, _ = check(sam, comp, TEXT, slot=1)
    assert res["n_rec"] == 1500


def test_lines_against_members(sam):
    p = TEXT.find(b"\n", 50_000)
    for cut in (p + 1, p):                                                # the newline a member's last byte; the next one's first byte
        comp = synth.bgzf_block(TEXT[:cut]) + synth.bgzf_block(TEXT[cut:cut + 60_000]) + b"".join(members(TEXT[cut + 60_000:], 0xff00))
        check(sam, comp, TEXT)
    over3 = body(20) + line_of(20, 2600) + body(20, 21)
    at = over3.find(b"ZZ:Z:")
    comp = synth.bgzf_block(over3[:at + 100]) + synth.bgzf_block(over3[at + 100:at + 1100]) + synth.bgzf_block(over3[at + 1100:])
    assert over3.find(b"\n", at) > at + 1100
    check(sam, comp, over3)
    long_read = body(100) + line(100, 70_000, opt=("NM:i:3", XA1), flag="83") + body(50, 101)
    res, _, a = check(sam, b"".join(members(long_read, 0xff00, 1)), long_read, slot=1)
    assert int(a["tmpend"][100]) == 1100 - 1 + 70_000 and int(a["xa_len"][100]) == len(XA1) - 5


@pytest.mark.parametrize("tail", [0, 1, 15, 16, 17, 70_000])
def test_carry_between_two_chunks(tail, sam):
    first, last = body(400), body(300, 401)
    mid = line(400, 70_000, opt=(XA1,)) if tail > 1000 else line(400, 50)
    text = first + mid + last
    cut = len(first) + tail
    for s0 in (0, 1):
        r0, i0 = sam.parse_bgzf(b"".join(members(text[:cut], 0xff00, 1)), False, s0)
        a0 = snapshot(sam, s0, r0)
        t0 = sam.text(s0)
        r1, i1 = sam.parse_bgzf(b"".join(members(text[cut:], 5000)) + synth.BGZF_EOF, True, 1 - s0)
        a1 = snapshot(sam, 1 - s0, r1)
        t1 = sam.text(1 - s0)
        assert (i0["n_bad"], i1["n_bad"]) == (0, 0)
        assert t0 == text[:cut] and (r0["consumed"], i0["tail_len"], i0["carry_len"]) == (len(first), tail, 0)
        assert t1 == text[len(first):] and (i1["carry_len"], i1["text_len"], i1["tail_len"]) == (tail, len(mid) + len(last), 0)
        assert r0["consumed"] + r1["consumed"] == len(text) and r0["n_rec"] + r1["n_rec"] == 701
        assert int(a1["line_off"][0]) == 0 and int(a1["qname_len"][0]) == 4 and int(a1["line_off"][1]) == len(mid)      # the completed line
        same_as_plain(sam, s0, text[:cut], False, r0, a0)
        same_as_plain(sam, s0, text[len(first):], True, r1, a1)


def test_skip_takes_the_header_off(sam):
    text = body(600)
    for payload, skip in ((1000, 0), (1000, 1), (1000, 15), (1000, 16), (1000, 1000), (1000, 1234), (0xff00, 70_000)):
        whole = b"@" * skip + text
        check(sam, b"".join(members(whole, payload)), text, skip=skip, slot=skip & 1)
    # 3 366 @SQ lines: the body begins inside the second member
    header = b"".join(b"@SQ\tSN:contig%d\tLN:%d\n" % (i, 1000 + i) for i in range(3366))
    assert 0xff00 < len(header) < 2 * 0xff00
    check(sam, b"".join(members(header + text, 0xff00, 1)), text, skip=len(header))
    # a header longer than the first chunk: that chunk's text is empty, the next one skips what is left of the header
    ms = members(header + text, 20_000)
    r0, i0 = sam.parse_bgzf(b"".join(ms[:3]), False, 0, skip=len(header))
    assert (r0["n_lines"], r0["n_rec"], r0["consumed"], i0["text_len"], i0["tail_len"], i0["n_bad"]) == (0, 0, 0, 0, 0, 0)
    r1, i1 = sam.parse_bgzf(b"".join(ms[3:]), True, 1, skip=len(header) - 60_000)
    assert (i1["carry_len"], i1["text_len"]) == (0, len(text)) and sam.text(1) == text
    same_as_plain(sam, 0, text, True, r1, snapshot(sam, 1, r1))


def expect_strings(text, a, first, n, want):
    out, qat, xat = [], [], []
    at = 0
    for i in range(first, first + n):
        q, x = eng.SAMTEXT_NO_STRING, eng.SAMTEXT_NO_STRING
        if want & 1:
            lo = int(a["line_off"][i])
            out.append(text[lo:lo + int(a["qname_len"][i])] + b"\0")
            q, at = at, at + len(out[-1])
        if want & 2 and a["xa_mark"][i]:
            lo = int(a["xa_off"][i])
            out.append(text[lo:lo + int(a["xa_len"][i])] + b"\0")
            x, at = at, at + len(out[-1])
        qat.append(q)
        xat.append(x)
    return b"".join(out), np.array(qat, np.uint32), np.array(xat, np.uint32)


def check_strings(x, slot, text, a, first, n, want):
    packed, qat, xat, guard = x.strings(slot, first, n, want)
    e_packed, e_qat, e_xat = expect_strings(text, a, first, n, want)
    assert packed == e_packed, (first, n, want)
    assert np.array_equal(qat, e_qat) and np.array_equal(xat, e_xat)
    assert guard == b"\xa5" * 16                                          # the bytes behind the text: nobody's


def test_strings_gathered_on_the_device():
    x = eng.SamText(NAMES, MAX_CHUNK)                                       # an object of its own: its buffers start small
    big_xa = "XA:Z:" + "chr1,+5,50M,1;" * 2857 + "ab"
    assert len(big_xa) == 40_005
    parts = []
    for i in range(70_001):
        name = "n" if i % 1000 == 7 else "N" * 254 if i % 1000 == 8 else None
        opt = (big_xa,) if i == 300 else ("XA:Z:",) if i % 500 == 9 else ("NM:i:2", XA1) if i % 4 == 1 else ()
        parts.append(line(i, 10 + i % 9, opt=opt, name=name))
    text = b"".join(parts)
    assert len(text) <= MAX_CHUNK
    res, info = x.parse_bgzf(b"".join(members(text, 0xff00, 1)), True, 1)
    assert (res["n_rec"], res["n_hard"], info["n_bad"]) == (70_001, 0, 0)
    a = snapshot(x, 1, res)
    assert int(a["xa_len"][300]) == 40_000 and a["xa_mark"][9] and int(a["xa_len"][9]) == 0
    check_strings(x, 1, text, a, 5, 1, 3)                                   # the first call: a few bytes
    for want in (1, 2, 3):
        for first, n in ((0, 255), (0, 256), (1, 257), (290, 20), (777, 1), (0, 70_001), (69_000, 1001)):
            check_strings(x, 1, text, a, first, n, want)
    check_strings(x, 1, text, a, 2, 2, 2)                                   # no record marked: an empty text
    assert x.strings(1, 2, 2, 2)[0] == b""
    every = b"".join(line(i, 25, opt=(f"XA:Z:chr2,-{i},25M,0;",)) for i in range(600))
    res = x.parse(every, True, 0)                                           # a chunk begun the plain way serves strings as well
    check_strings(x, 0, every, snapshot(x, 0, res), 3, 597, 3)
    check_strings(x, 0, every, snapshot(x, 0, res), 0, 600, 2)
    x.close()


def test_lifecycle_and_buffers_that_regrow():
    """made and destroyed with no call between; then, twice in one process: made, a BGZF chunk of three lines in a few members, then
    one of 1500 lines in members of 100 bytes in the same slot: its compressed bytes, block lists, status bytes, the decoder's scratch
    and the string gather's buffers are all far beyond need + need / 4 + 64 of the first and are taken anew under one object; text,
    records and strings as for every chunk here; destroyed"""
    eng.SamText(NAMES, 1 << 16).close()
    few = body(3)
    room = lambda need: need + need // 4 + 64                              # what a buffer made for `need` elements holds
    chunks = [(text, members(text, 100)) for text in (few, TEXT)]
    (_, m0), (_, m1) = chunks
    assert len(m1) > 3 * room(len(m0) + 1) and len(b"".join(m1)) > 3 * room(len(b"".join(m0)) + 64) and 2 * 1500 > 3 * room(2 * 3)
    for _ in range(2):
        x = eng.SamText(NAMES, 1 << 20)
        for text, ms in chunks:
            res, _, a = check(x, b"".join(ms), text, slot=0)
            assert res["n_rec"] == text.count(b"\n")
            check_strings(x, 0, text, a, 0, res["n_rec"], 3)
        x.close()


def test_damaged_member(sam):
    ms = [bytearray(m) for m in members(TEXT, 9000)]
    ms[5][18] |= 6                                                          # one byte of its deflate data: a block type that does not exist
    res, info = sam.parse_bgzf(b"".join(bytes(m) for m in ms), False, 0)
    assert (info["n_bad"], info["first_bad"], res["n_rec"]) == (1, 5, 0)
    check(sam, b"".join(members(TEXT, 9000)), TEXT, slot=0)                 # the stream ended there: the slot takes a new one


def test_argument_and_state_checks(sam):
    L = eng.load()
    t30 = TEXT[:TEXT.find(b"\n", 30_000) + 1]
    comp = b"".join(members(t30, 4000))
    blocks = eng.index_bgzf(comp)
    buf = np.frombuffer(comp + b"\0", np.uint8).copy()
    begin = lambda h, slot, n_comp, blk, skip=0, final=1: L.itx_samtext_parse_begin_bgzf(h, slot, eng._p(buf), n_comp, eng._p(blk), len(blk), skip, final)
    assert begin(None, 0, len(comp), blocks) == -1 and begin(sam._h, 2, len(comp), blocks) == -1
    assert L.itx_samtext_parse_begin_bgzf(sam._h, 0, None, len(comp), eng._p(blocks), len(blocks), 0, 1) == -1
    assert L.itx_samtext_parse_begin_bgzf(sam._h, 0, eng._p(buf), len(comp), None, len(blocks), 0, 1) == -1
    assert begin(sam._h, 0, len(comp) - 1, blocks) == -1                   # the last member ends behind the bytes
    for field, value in (("uoff", 1), ("usize", 65537), ("csize", 25)):
        bad = blocks.copy()
        bad[field][2] = value
        assert begin(sam._h, 0, len(comp), bad) == -1, field
    small = eng.SamText(NAMES, 1 << 16)
    info, out = eng.SamTextBgzfInfo(), eng.SamTextStrings()
    assert begin(small._h, 0, len(comp), blocks[:3], skip=0, final=0) == 0
    assert begin(small._h, 0, len(comp), blocks[:3]) == -5                 # begun twice
    assert L.itx_samtext_strings(small._h, 0, 0, 1, 3, C.byref(out)) == -5 # not ended yet
    assert L.itx_samtext_bgzf_info(small._h, 0, C.byref(info)) == -5
    assert L.itx_samtext_text(small._h, 0, 0, eng._p(buf), 1) == -5
    res = small.end(0)
    assert res["n_rec"] >= 50
    assert begin(small._h, 0, len(comp), blocks[:3]) == -5                 # the stream's previous chunk lies in this slot
    assert L.itx_samtext_strings(small._h, 0, res["n_rec"], 1, 3, C.byref(out)) == -1        # first + n out of range
    assert L.itx_samtext_strings(small._h, 0, 0, res["n_rec"] + 1, 3, C.byref(out)) == -1
    assert L.itx_samtext_strings(small._h, 0, 0, 1, 0, C.byref(out)) == -1 and L.itx_samtext_strings(small._h, 0, 0, 1, 3, None) == -1
    assert L.itx_samtext_strings(small._h, 1, 0, 1, 3, C.byref(out)) == -5 # the other slot is empty
    assert L.itx_samtext_text(small._h, 0, 12_000, eng._p(buf), 1) == -1 and L.itx_samtext_bgzf_info(small._h, 0, None) == -1
    assert L.itx_samtext_strings(small._h, 0, 0, 0, 3, C.byref(out)) == 0 and out.text_len == 0
    wide = b"".join(members(TEXT[:140_000], 0xff00))
    wbuf = np.frombuffer(wide + b"\0", np.uint8).copy()
    wb = eng.index_bgzf(wide)
    assert L.itx_samtext_parse_begin_bgzf(small._h, 1, eng._p(wbuf), len(wide), eng._p(wb), len(wb), 0, 1) == -6      # more than the object holds
    assert L.itx_samtext_parse_begin_bgzf(small._h, 1, eng._p(wbuf), len(wide), eng._p(wb[:2]), 2, 0, 1) == -6        # inflates into its room, the text does not fit
    small.parse(b"", True, 0)
    assert small.parse_bgzf(comp, True, 1)[0]["n_rec"] == t30.count(b"\n")                               # and the object still works
    res = small.parse(TEXT[:5000], True, 0)
    assert L.itx_samtext_bgzf_info(small._h, 0, C.byref(info)) == -5       # a chunk begun the plain way
    assert small.text(0, 10, 90) == TEXT[10:100]
    small.close()


# ---- 2. the command -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


def bgzf_file(text: bytes, payload: int, eof: bool = True) -> bytes:
    return b"".join(members(text, payload)) + (synth.BGZF_EOF if eof else b"")


@pytest.fixture(scope="module")
def pile(tmp_path_factory):
    """the `pile` of tests/test_gpu_samtext.py (every mapped read has a CIGAR, XA on a quarter, 6 000 reads), and the same text as BGZF"""
    d = tmp_path_factory.mktemp("samgz_pile")
    chroms = [("chr1", 2_000_000), ("chr2", 700_000)]
    t = synth.make_table(91, chroms, 3000, n_names=60, n_fams=9, n_clas=4, overlap_frac=0.05)
    synth.write_sizes(str(d / "chrom.sizes"), chroms)
    synth.write_sizes(str(d / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(d / "rmsk.txt"), t)
    r = synth.make_reads(92, chroms, 6000, read_len=(40, 120), paired_frac=0.3, nocigar_frac=0.0)
    rng = np.random.default_rng(93)
    r.aux = [[f"NM:i:{i % 3}", f"XA:Z:chr1,+{1 + int(rng.integers(1_900_000))},50M,1;"] if i % 4 == 0 else [] for i in range(len(r))]
    synth.write_sam(str(d / "reads.sam"), r)
    text = (d / "reads.sam").read_bytes()
    (d / "reads.sam.gz").write_bytes(bgzf_file(text, 4000))
    return d, text


ROUTES = {"host": {"ITX_HOST_SAM": "1"}, "host_inflate": {"ITX_HOST_SAM": "0", "ITX_HOST_SAM_INFLATE": "1", "ITX_SAM_CHUNK": "65536"},
          "device_4096": {"ITX_HOST_SAM": "0", "ITX_SAM_CHUNK": "4096"}, "device_1M": {"ITX_HOST_SAM": "0", "ITX_SAM_CHUNK": str(1 << 20)}}
SIDE = ("chrom.sizes", "rep.sizes", "rmsk.txt")


def _run(exe, cmd, opts, d, out, aln, env, prefix="out", ref=False):
    os.makedirs(out)
    keep = {k: v for k, v in os.environ.items() if k not in ("ITX_HOST_SAM", "ITX_HOST_SAM_INFLATE", "ITX_SAM_CHUNK")}
    pr = subprocess.run([exe, cmd, "-S"] + opts + ["-o", prefix] + [str(d / n) for n in SIDE] + [str(aln)], cwd=out, capture_output=True, text=True, timeout=600,
                        env=keep if ref else dict(keep, ITX_TIMING="1", **env))
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr.stderr.replace(str(aln), "<the alignment file>")


def _gz_line(err):
    """-> (chunks inflated on the device, compressed bytes, inflated bytes, chunks by the host, the reason), or None for `not compressed`"""
    lines = [l for l in err.split("\n") if l.startswith("[itx timing] sam gz:")]
    assert len(lines) == 1, err[-1500:]
    if lines[0] == "[itx timing] sam gz: not compressed":
        return None
    m = re.fullmatch(r"\[itx timing\] sam gz: (\d+) chunks inflated on the device \((\d+) -> (\d+) bytes, [0-9.]+ ms in the decoder, [0-9.]+ ms gathering strings\), "
                     r"(\d+) by the host \((.*)\)", lines[0])
    assert m, lines[0]
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)


def _user_stderr(err):
    return "\n".join(l for l in err.replace("\r", "\n").split("\n") if not l.startswith("[itx timing]") and "time used" not in l)


def _same_dirs(a, b, but=()):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b))
    for fn in names:
        if not fn.endswith(tuple(but)):
            assert filecmp.cmp(os.path.join(a, fn), os.path.join(b, fn), shallow=False), fn


@pytest.mark.parametrize("opts", [["-w"], ["-w", "-x", "-B", "-V", "-R"]], ids=["w", "wxBVR"])
def test_three_routes_write_the_same_files(opts, pile, exe, tmp_path):
    d, text = pile
    size = os.path.getsize(d / "reads.sam.gz")
    plain = _run(exe, "stat", opts, d, tmp_path / "plain", d / "reads.sam", ROUTES["host"])
    assert _gz_line(plain) is None
    for name, env in ROUTES.items():
        err = _run(exe, "stat", opts, d, tmp_path / name, d / "reads.sam.gz", env)
        _same_dirs(tmp_path / name, tmp_path / "plain")
        assert _user_stderr(err) == _user_stderr(plain), name
        n_dev, n_comp, n_infl, n_host, why = _gz_line(err)
        print(name, opts, n_dev, n_comp, n_infl, n_host, why)
        if name.startswith("device"):
            assert n_dev >= 1 and n_host == 0 and why == "none" and (n_comp, n_infl) == (size, len(text))
            assert n_dev >= len(text) // (int(env["ITX_SAM_CHUNK"]) + 65536)
            m = re.search(r"\[itx timing\] sam: (\d+) chunks parsed on the device \(\d+ bytes, .*\), (\d+) by the host", err)
            assert m and int(m.group(1)) >= 1 and int(m.group(2)) == 0
        else:
            assert n_dev == 0
            assert (n_host, why) == (0, "read line by line") if name == "host" else (n_host >= 1 and why == "ITX_HOST_SAM_INFLATE=1")


def test_filter_names_through_the_gather(pile, exe, tmp_path):
    d, text = pile
    plain = _run(exe, "filter", ["-r"], d, tmp_path / "plain", d / "reads.sam", ROUTES["host"])
    loci = (tmp_path / "plain" / "out_ALL.iteres.loci").read_bytes()
    body_lines = [l for l in text.split(b"\n") if l and not l.startswith(b"@")]
    assert sum(l.split(b"\t")[0] in loci for l in body_lines[:500]) >= 10      # the lists hold read names
    for name, env in ROUTES.items():
        err = _run(exe, "filter", ["-r"], d, tmp_path / name, d / "reads.sam.gz", env)
        _same_dirs(tmp_path / name, tmp_path / "plain")
        assert _user_stderr(err) == _user_stderr(plain), name
        n_dev, _, _, n_host, _ = _gz_line(err)
        assert (n_dev >= 1 and n_host == 0) if name.startswith("device") else n_dev == 0


def test_golden_with_a_hard_line_as_bgzf(exe, tmp_path):
    """quirks/in/reads.sam holds lines the device does not model: their chunk is the host's, which fetches the text from the device"""
    run = gc.manifest_run("quirks", "stat_default_sam")
    src = os.path.join(gc.GOLDEN, "quirks", "in")
    for n in SIDE:
        refio.materialise(src, n, str(tmp_path))
    (tmp_path / "reads.sam.gz").write_bytes(bgzf_file(refio.read_bytes(os.path.join(src, "reads.sam")), 1000))
    for chunk in ("1000", str(1 << 20)):
        out = tmp_path / f"out{chunk}"
        err = _run(exe, "stat", [o for o in run["opts"] if o != "-S"], tmp_path, out, tmp_path / "reads.sam.gz", {"ITX_HOST_SAM": "0", "ITX_SAM_CHUNK": chunk}, prefix=run["prefix"])
        for fn in run["files"]:
            assert (out / fn).read_bytes() == refio.read_bytes(os.path.join(gc.GOLDEN, "quirks", "stat_default_sam", fn)), fn
        n_dev, _, _, n_host, why = _gz_line(err)
        assert n_dev >= 1 and n_host == 0 and why == "none"                 # inflated on the device, all of it ...
        m = re.search(r"\[itx timing\] sam: (\d+) chunks parsed on the device \(\d+ bytes, .*\), (\d+) by the host \(line \d+ is spelt", err)
        assert m and int(m.group(2)) >= 1, err[-1500:]                      # ... and a chunk parsed by the host


def _inflate_what_is_there(data: bytes) -> bytes:
    out, off = [], 0
    while off < len(data):
        z = zlib.decompressobj(31)
        try:
            out.append(z.decompress(data[off:]))
        except zlib.error:
            break
        if not z.eof:
            break
        off = len(data) - len(z.unused_data)
    return b"".join(out)


@pytest.mark.parametrize("kind", ["bgzf_then_gzip", "truncated", "damaged_member"])
def test_hand_over_to_the_hosts_reader(kind, pile, exe, tmp_path):
    d, text = pile
    whole = bgzf_file(text, 4000)
    if kind == "bgzf_then_gzip":
        half = len(text) // 2 + 17                                          # in mid-line: the carry goes in front of the gzip member's text
        data, same_as = bgzf_file(text[:half], 4000, eof=False) + gzip.compress(text[half:]), text
    elif kind == "truncated":
        data = whole[: len(whole) * 3 // 5]
        same_as = _inflate_what_is_there(data)
        assert 0 < len(same_as) < len(text) and not same_as.endswith(b"\n")
    else:
        # A block type that does not exist. What gzread hands out in front of a data error depends on the sizes it is asked for, so the
        # routes need not agree on such a file (nor with the reference): the hand-over itself is what is checked.
        ms = [bytearray(m) for m in members(text, 4000)]
        ms[len(ms) // 2][18] |= 6
        (d / f"{kind}.sam.gz").write_bytes(b"".join(bytes(m) for m in ms))
        for name in ("device_4096", "device_1M"):
            err = _run(exe, "stat", ["-w"], d, tmp_path / name, d / f"{kind}.sam.gz", ROUTES[name])
            n_dev, _, _, n_host, why = _gz_line(err)
            print(kind, name, n_dev, n_host, why)
            assert why.startswith("handed over at byte ") and "does not inflate on the device" in why, why
            assert (n_dev >= 10) if name == "device_4096" else n_dev == 0
        return
    (d / f"{kind}.sam.gz").write_bytes(data)
    (d / f"{kind}.sam").write_bytes(same_as)
    opts = ["-w", "-x", "-B"]
    plain = _run(exe, "stat", opts, d, tmp_path / "plain", d / f"{kind}.sam", ROUTES["host"])
    host = _run(exe, "stat", opts, d, tmp_path / "host", d / f"{kind}.sam.gz", ROUTES["host"])
    _same_dirs(tmp_path / "host", tmp_path / "plain")
    for name in ("device_4096", "device_1M"):
        err = _run(exe, "stat", opts, d, tmp_path / name, d / f"{kind}.sam.gz", ROUTES[name])
        _same_dirs(tmp_path / name, tmp_path / "host")
        assert _user_stderr(err) == _user_stderr(host)
        n_dev, _, _, n_host, why = _gz_line(err)
        print(kind, name, n_dev, n_host, why)
        assert n_host >= 1 and why.startswith("handed over at byte "), why
        if name == "device_4096":
            assert n_dev >= 10
    if os.path.exists(REF):
        _run(REF, "stat", opts, d, tmp_path / "ref", d / f"{kind}.sam.gz", {}, ref=True)
        _same_dirs(tmp_path / "ref", tmp_path / "device_4096", but=(".bigWig",))


def test_plain_gzip_is_inflated_by_the_host_and_parsed_on_the_device(pile, exe, tmp_path):
    d, text = pile
    (d / "plain_gzip.sam.gz").write_bytes(gzip.compress(text, 6))
    plain = _run(exe, "stat", ["-w"], d, tmp_path / "plain", d / "reads.sam", ROUTES["host"])
    err = _run(exe, "stat", ["-w"], d, tmp_path / "dev", d / "plain_gzip.sam.gz", {"ITX_HOST_SAM": "0", "ITX_SAM_CHUNK": "65536"})
    _same_dirs(tmp_path / "dev", tmp_path / "plain")
    assert _user_stderr(err) == _user_stderr(plain)
    n_dev, _, _, n_host, why = _gz_line(err)
    assert n_dev == 0 and n_host >= len(text) // 65536 and why == "plain gzip is one stream"
    m = re.search(r"\[itx timing\] sam: (\d+) chunks parsed on the device \(\d+ bytes, .*\), (\d+) by the host", err)
    assert m and int(m.group(1)) == n_host and int(m.group(2)) == 0
