"""CPU: the BGZF member rule of `filter -b` (csrc/itx_bgzfmember.h) in its host build (tests/bgzfmember_host.cpp), held to zlib:
every member inflates to its payload with nothing unused, every header field is BGZF's, CRC-32 and ISIZE are the payload's;
concatenated members and the EOF marker read back through refio.bgzf_decompress; the lane-parallel CRC with 64 host "lanes".
And the command's refusals of -b, which need no GPU."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzfmemberhost as bm
import refio
from iteres_amd import build, synth


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return bm.MemberRule(tmp_path_factory.mktemp("bgzfmember"))


@pytest.fixture(scope="module")
def bam_bytes(tmp_path_factory):
    """the inflated bytes of a synth.write_bam file"""
    d = tmp_path_factory.mktemp("bgzfmember_bam")
    header = [("chr1", 2_000_000), ("chr2", 900_000)]
    synth.write_bam(str(d / "r.bam"), synth.make_reads(5, header, 1500, paired_frac=0.3))
    return refio.bgzf_decompress((d / "r.bam").read_bytes())


def lengths(P):
    return [0, 1, 2, 3, 63, 64, 65, P - 1, P]


def contents(kind, n, bam):
    if kind == "zeros":
        return bytes(n)
    if kind == "period4":
        return (b"\x01\x80\x00\xff" * (n // 4 + 1))[:n]
    if kind == "random":
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert len(bam) >= n
    return bam[:n]


def test_payload_constant(rule):
    assert rule.payload % 16 == 0 and 0 < rule.payload <= 32768


@pytest.mark.parametrize("kind", ["zeros", "period4", "random", "bam"])
def test_members_of_every_length(rule, bam_bytes, kind):
    for n in lengths(rule.payload):
        b = contents(kind, n, bam_bytes)
        m = rule.member(b)
        bm.check_member(m, b)
        if kind == "random" and n >= 64:
            assert len(m) == n + 5 + 26                                  # the stored path: 5 bytes of block header
        if kind == "zeros" and n >= 64:
            assert len(m) < n // 8 + 64
        assert m == rule.member(b)                                        # a pure function of the payload


def test_random_mixtures(rule, bam_bytes):
    rng = np.random.default_rng(20240)
    P = rule.payload
    for k in range(200):
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
                at = int(rng.integers(0, len(bam_bytes) - m))
                parts.append(bam_bytes[at:at + m])
            else:
                unit = rng.integers(0, 4, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
                parts.append((unit * (m // len(unit) + 1))[:m])
            left -= m
        b = b"".join(parts)
        assert len(b) == n
        bm.check_member(rule.member(b), b)


def test_concatenated_members_and_eof(rule, bam_bytes):
    P = rule.payload
    data = bam_bytes[:3 * P + 1234]
    ms = rule.members(data)
    assert len(ms) == 4 and [len(bm.check_member(m)) for m in ms] == [P, P, P, 1234]
    blob = b"".join(ms) + bm.EOF_MARKER
    assert refio.bgzf_decompress(blob) == data
    assert bm.split_members(blob) == ms + [bm.EOF_MARKER]
    # an empty payload is a member too (the marker itself is samtools' 28 bytes, written by the host)
    assert refio.bgzf_decompress(rule.member(b"") + blob) == data
    assert rule.members(data[:2 * P]) == ms[:2] and rule.members(data, tail=False) == ms[:3]


@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_lane_parallel_crc(rule, bam_bytes, lanes):
    rng = np.random.default_rng(7)
    P = rule.payload
    for n in [0, 1, 2, 3, 5, 63, 64, 65, 66, 127, 129, 255, 1001, 4097, P - 3, P - 1, P, 32767, 32768]:
        for b in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n), b"\xff" * n, (bam_bytes * 2)[:n]):
            assert rule.crc_lanes(b, lanes) == zlib.crc32(b), (n, lanes)


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
    (d / "x.sam").write_text("@SQ\tSN:chr1\tLN:1000\nr0\t0\tchr1\t20\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n")
    synth.write_bam(str(d / "x.bam"), synth.make_reads(3, [("chr1", 1000)], 20, read_len=(20, 30)))


def test_b_with_sam_text_is_refused(exe, tmp_path):
    _inputs(tmp_path)
    r = subprocess.run([exe, "filter", "-b", "-S", "c.sizes", "r.sizes", "rmsk.txt", "x.sam"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255, r.stderr
    assert "-b" in r.stderr and "-S" in r.stderr and "SAM" in r.stderr
    assert "Start to parse" not in r.stderr and "no usable" not in r.stderr      # refused before any input is read or any GPU call made
    assert not [p.name for p in tmp_path.iterdir() if p.name.endswith(".bam") and p.name != "x.bam"]
    assert not [p.name for p in tmp_path.iterdir() if ".iteres." in p.name]


def test_b_with_the_host_decoder_is_refused(exe, tmp_path):
    _inputs(tmp_path)
    r = subprocess.run([exe, "filter", "-b", "c.sizes", "r.sizes", "rmsk.txt", "x.bam"], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ITX_HOST_INFLATE="1"))
    assert r.returncode == 255, r.stderr
    assert "-b" in r.stderr and "ITX_HOST_INFLATE" in r.stderr
    assert "Start to parse" not in r.stderr and "no usable" not in r.stderr
    assert not [p.name for p in tmp_path.iterdir() if ".iteres." in p.name]


def test_usage_lists_b(exe):
    r = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    line = [ln for ln in r.stderr.splitlines() if ln.strip().startswith("-b ")]
    assert len(line) == 1 and ".iteres.bam" in line[0] and "extension" in line[0]
    assert "-t" in r.stderr and "whatever -t" in r.stderr
