"""CPU: the levels of the BAM's members (`filter -b -l`; csrc/itx_bgzflevels.h over csrc/itx_deflate_fast.h) in their host build
(tests/bgzflevels_host.cpp), held to zlib: every member of levels 0 and 1 inflates to its payload with nothing unused, every field
of the frame is BGZF's, no member exceeds payload + 31 bytes and a level-0 member is exactly that; 1, 3 and 64 lanes write the
same bytes; level 6 through the level call is itx_bgzf_member's member. The payloads sit on the fast encoder's slice edges (128
positions): matches that cross them, runs cut at two of them, distances of many slices. The same payloads run through a stand-alone
build under AddressSanitizer and UndefinedBehaviorSanitizer with exact-size heap blocks. And the command's refusals of -l, which
need no GPU."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzflevelshost as bl
import bgzfmemberhost as bm
import refio
from iteres_amd import build, synth

LEVELS = (0, 1)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return bl.LevelRule(tmp_path_factory.mktemp("bgzflevels"))


@pytest.fixture(scope="module")
def bam_bytes(tmp_path_factory):
    """the inflated bytes of a synth.write_bam file"""
    d = tmp_path_factory.mktemp("bgzflevels_bam")
    header = [("chr1", 2_000_000), ("chr2", 900_000)]
    synth.write_bam(str(d / "r.bam"), synth.make_reads(5, header, 1500, paired_frac=0.3))
    return refio.bgzf_decompress((d / "r.bam").read_bytes())


def sizes(P):
    return [0, 1, 2, 3, 127, 128, 129, 255, 256, 257, P - 1, P]


def contents(kind, n, bam):
    if kind == "zeros":
        return bytes(n)
    if kind == "period4":
        return (b"\x01\x80\x00\xff" * (n // 4 + 1))[:n]
    if kind == "period129":                                              # every match crosses a slice edge
        return (bytes((i * 37 + 11) & 255 for i in range(129)) * (n // 129 + 1))[:n]
    if kind == "random":
        return np.random.default_rng(n + 1).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert kind == "bam" and len(bam) >= n
    return bam[:n]


KINDS = ["zeros", "period4", "period129", "random", "bam"]


def specials(P):
    rng = np.random.default_rng(77)
    noise = rng.integers(0, 256, P, dtype=np.uint8).tobytes()
    run = bytearray(noise[:1000])
    run[100:400] = b"\x5a" * 300                                          # a run of 300 equal bytes from 100 on: cut at 128, 256 and 384
    half = rng.integers(0, 256, 4000, dtype=np.uint8).tobytes()
    return {"run300": bytes(run), "twice4000": half + half}               # distances of 4000: more than 31 slices back


def mixtures(P, bam, count=200):
    rng = np.random.default_rng(20241)
    for _ in range(count):
        n = int(rng.integers(0, P + 1))
        parts, left = [], n
        while left:
            m = min(left, int(rng.integers(1, 2000)))
            what = int(rng.integers(0, 4))
            if what == 0:
                parts.append(bytes([int(rng.integers(0, 256))]) * m)
            elif what == 1:
                parts.append(rng.integers(0, 256, m, dtype=np.uint8).tobytes())
            elif what == 2:
                at = int(rng.integers(0, len(bam) - m))
                parts.append(bam[at:at + m])
            else:
                unit = rng.integers(0, 4, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
                parts.append((unit * (m // len(unit) + 1))[:m])
            left -= m
        b = b"".join(parts)
        assert len(b) == n
        yield b


def all_payloads(P, bam):
    out = [contents(k, n, bam) for k in KINDS for n in sizes(P)]
    out += list(specials(P).values())
    out += list(mixtures(P, bam))
    return out


def check(m, payload, level):
    """the issue's member checks"""
    assert zlib.decompress(m, 31) == payload
    bm.check_member(m, payload)                                           # header bytes, BSIZE, CRC-32, ISIZE, nothing unused
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    assert crc == zlib.crc32(payload) and isize == len(payload)
    assert len(m) <= len(payload) + 31
    if level == 0:
        assert len(m) == len(payload) + 31
        assert m[18:23] == b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) and m[23:-8] == payload


def test_constants(rule):
    assert rule.payload == 8192 and rule.slice == 128


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_members_of_every_size(rule, bam_bytes, kind, level):
    for n in sizes(rule.payload):
        b = contents(kind, n, bam_bytes)
        m = rule.member(b, level)
        check(m, b, level)
        assert m == rule.member(b, level)                                 # a pure function of the payload
        if level == 1 and kind == "random" and n >= 128:
            assert len(m) == n + 31                                       # the stored fallback
        if level == 1 and kind in ("zeros", "period4") and n >= 255:
            assert len(m) < n // 2 + 64, (kind, n, len(m))                # the Huffman block was written
        if level == 1 and kind == "period129" and n >= 255:
            assert len(m) < n + 31 - (n - 129) // 2, (n, len(m))          # the first period is literals, the rest matches that cross slice edges


@pytest.mark.parametrize("level", LEVELS)
def test_slice_edge_cases(rule, level):
    for name, b in specials(rule.payload).items():
        m = rule.member(b, level)
        check(m, b, level)
        if level == 1 and name == "run300":
            assert len(m) < len(b) + 31 - 200                             # the run is matches, cut or not
        if level == 1 and name == "twice4000":
            # random bytes alone would be stored: what makes the Huffman block smaller is matches that reach back 4000 bytes (the
            # finder keeps one candidate per hash head, so it finds some of them, not all: no figure is asserted)
            assert len(m) < len(b) + 31


@pytest.mark.parametrize("level", LEVELS)
def test_random_mixtures(rule, bam_bytes, level):
    for b in mixtures(rule.payload, bam_bytes):
        check(rule.member(b, level), b, level)


@pytest.mark.parametrize("level", LEVELS)
def test_concatenated_members(rule, bam_bytes, level):
    P = rule.payload
    data = bam_bytes[:3 * P + 1234]
    ms = rule.members(data, level)
    assert len(ms) == 4 and [len(bm.check_member(m)) for m in ms] == [P, P, P, 1234]
    blob = b"".join(ms) + bm.EOF_MARKER
    assert refio.bgzf_decompress(blob) == data
    assert bm.split_members(blob) == ms + [bm.EOF_MARKER]
    assert refio.bgzf_decompress(rule.member(b"", level) + blob) == data
    assert rule.members(data[:2 * P], level) == ms[:2] and rule.members(data, level, tail=False) == ms[:3]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("lanes", [3, 64])
def test_lanes_agree(rule, bam_bytes, level, lanes):
    P = rule.payload
    cases = [contents(k, n, bam_bytes) for k in KINDS for n in sizes(P) if n < 1000 or k in ("bam", "period129")]
    cases += list(specials(P).values()) + list(mixtures(P, bam_bytes, 6))
    for b in cases:
        assert rule.member(b, level, lanes) == rule.member(b, level, 1), (len(b), lanes)


def test_level_6_is_the_member_rule(rule, bam_bytes, tmp_path):
    old = bm.MemberRule(tmp_path)                                         # tests/bgzfmember_host.cpp: today's hooks, today's bytes
    P = rule.payload
    cases = [contents(k, n, bam_bytes) for k in KINDS for n in sizes(P)] + list(specials(P).values()) + list(mixtures(P, bam_bytes, 20))
    for b in cases:
        m = rule.member(b, 6)
        assert m == rule.plain(b) == old.member(b), len(b)


def test_bam_content_is_smaller_at_level_1(rule, bam_bytes):
    """repeated names and constant qualities: the fast encoder's members are, in total, smaller than the stored ones"""
    P = rule.payload
    data = bam_bytes[:8 * P]
    assert len(data) == 8 * P
    z0 = sum(len(m) for m in rule.members(data, 0))
    z1 = sum(len(m) for m in rule.members(data, 1))
    assert z0 == 8 * (P + 31) and z1 < z0
    print(f"level 0: {z0} bytes, level 1: {z1}, level 6: {sum(len(rule.member(data[i:i + P], 6)) for i in range(0, 8 * P, P))}")


def test_sanitized_program(rule, bam_bytes, tmp_path):
    """the same payloads through the stand-alone build under AddressSanitizer and UndefinedBehaviorSanitizer, payloads and members in
    exact-size heap blocks; what it writes is what the library build writes"""
    exe = bl.build_sanitized(tmp_path)
    payloads = all_payloads(rule.payload, bam_bytes)
    feed = b"".join(struct.pack("<I", len(b)) + b for b in payloads)
    r = subprocess.run([exe], input=feed, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr
    assert r.stderr.decode().strip().endswith(f"{len(payloads)} payloads")
    off, seen = 0, 0
    for b in payloads:
        for level, lanes in ((0, 1), (0, 3), (1, 1), (1, 3), (6, 1)):
            lv, nl, n, size = struct.unpack_from("<4I", r.stdout, off)
            assert (lv, nl, n) == (level, lanes, len(b))
            m = r.stdout[off + 16:off + 16 + size]
            off += 16 + size
            assert m == rule.member(b, level), (level, lanes, len(b))
            seen += 1
    assert off == len(r.stdout) and seen == 5 * len(payloads)


# ---- the command's refusals: decided while the options are read, before any GPU call

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


def _inputs(d):
    (d / "c.sizes").write_text("chr1\t1000\n")
    (d / "r.sizes").write_text("AluY\t311\n")
    (d / "rmsk.txt").write_text("585\t1\t0\t0\t0\tchr1\t10\t200\t-800\t+\tAluY\tSINE\tAlu\t1\t190\t-121\t1\n")
    synth.write_bam(str(d / "x.bam"), synth.make_reads(3, [("chr1", 1000)], 20, read_len=(20, 30)))


@pytest.mark.parametrize("opts", [("-l", "1"), ("-l", "2", "-b"), ("-l", "x", "-b"), ("-b", "-l", "9"), ("-b", "-l", "1x"), ("-b", "-l", "-1")],
                         ids=["l1_without_b", "l2", "lx", "l9_after_b", "l1x", "minus1"])
def test_l_is_refused(exe, tmp_path, opts):
    _inputs(tmp_path)
    before = sorted(p.name for p in tmp_path.iterdir())
    r = subprocess.run([exe, "filter", *opts, "c.sizes", "r.sizes", "rmsk.txt", "x.bam"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255, r.stderr
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and "-l" in lines[0], r.stderr
    assert "Start to parse" not in r.stderr and "no usable" not in r.stderr          # refused before any input is read or any GPU call made
    assert sorted(p.name for p in tmp_path.iterdir()) == before                        # no file


def test_usage_lists_l_once(exe):
    r = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    line = [ln for ln in r.stderr.splitlines() if ln.strip().startswith("-l ")]
    assert len(line) == 1 and "with -b" in line[0] and all(v in line[0] for v in ("0", "1", "6"))
    assert sum("-l" in ln.split() for ln in r.stderr.splitlines()) == 1
    # no other usage line changed
    others = [ln for ln in r.stderr.splitlines() if not ln.strip().startswith("-l ")]
    assert any(ln.strip().startswith("-b ") and ".iteres.bam" in ln for ln in others)
    assert any(ln.strip().startswith("-s ") and "with -b" in ln for ln in others) and any(ln.strip().startswith("-i ") and "with -b" in ln for ln in others)
