"""The device DEFLATE encoder (iteres_amd/csrc/itx_deflate_core.h, what csrc/itx_bigwig.hip deflates the bigWig blocks with)
built for the host with a one-lane wave (tests/deflate_host.cpp) and checked against zlib: every stream inflates to its
input, two encodings of one input are the same bytes, incompressible input takes a stored block, and on bigWig-like blocks
the compressed size stays within 1.25x of zlib level 6."""
import gzip
import os
import zlib

import numpy as np
import pytest

import deflatehost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return deflatehost.build_encoder(tmp_path_factory.mktemp("deflate"))


def _coverage(rng, n):
    v = np.zeros(n, np.float32)
    i = 0
    while i < n:
        r = int(rng.integers(1, 200))
        v[i:i + r] = float(rng.integers(0, 60)) if rng.random() < 0.6 else 0.0
        i += r
    return v


def _section(chrom, start, vals):
    hdr = np.array([chrom, start, start + len(vals), 1, 1, 3 | len(vals) << 16], np.uint32)
    return hdr.tobytes() + np.asarray(vals, np.float32).tobytes()


def _zoom(rng, n=1024, red=35):
    recs = np.zeros((n, 8), np.uint32)
    st = np.arange(n, dtype=np.uint32) * red
    recs[:, 0] = 7
    recs[:, 1] = st
    recs[:, 2] = st + red
    recs[:, 3] = red
    recs[:, 4:] = _coverage(rng, 4 * n).reshape(n, 4).view(np.uint32)
    return recs.tobytes()


def _golden_wig_values():
    """per-base values of the golden runs' wigs, as the bigWig stores them"""
    out = []
    for case, run in (("mid", "stat_default"), ("cfg1_chr22", "stat_default")):
        p = os.path.join(GOLDEN, case, run, "out.iteres.wig.gz")
        cur = []
        for ln in gzip.open(p, "rt"):
            if ln.startswith("fixedStep"):
                if cur:
                    out.append(np.array(cur, np.float32))
                cur = []
            elif ln.strip():
                cur.append(float(ln))
        if cur:
            out.append(np.array(cur, np.float32))
    return out


def _check(enc, b):
    c = enc(b)
    assert zlib.decompress(c) == b
    assert enc(b) == c
    return c


def test_edge_inputs(enc):
    rng = np.random.default_rng(3)
    for b in (b"", b"a", b"ab", b"abc", bytes(32768), bytes(range(256)) * 128, _section(0, 0, []), _section(4, 1024, [5.0]),
              _section(1, 0, [1.0, 2.0, 3.0]), np.zeros(1024, np.float32).tobytes(), np.full(1024, 7.0, np.float32).tobytes(),
              _zoom(rng, 1), _zoom(rng, 1024)):
        _check(enc, b)


def test_random_bytes_take_the_stored_block(enc):
    rng = np.random.default_rng(4)
    for n in (1, 7, 100, 4120, 32768):
        b = rng.bytes(n)
        c = _check(enc, b)
        assert c[2] & 7 == 1 and len(c) == n + 11        # BFINAL, BTYPE 00: 2 + 1 + 4 + n + 4


def test_fuzz_lengths_and_content(enc):
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(0, 32769))
        kind = rng.integers(0, 4)
        if kind == 0:
            b = rng.bytes(n)
        elif kind == 1:
            b = bytes(rng.integers(0, 3, n, dtype=np.uint8))
        elif kind == 2:
            b = _coverage(rng, (n + 3) // 4).tobytes()[:n]
        else:
            pat = rng.bytes(int(rng.integers(1, 40)))
            b = (pat * (n // len(pat) + 1))[:n]
        _check(enc, b)


def test_ratio_against_zlib_level6(enc):
    rng = np.random.default_rng(6)
    secs, zooms = [], []
    for vals in _golden_wig_values():
        for s in range(0, len(vals), 1024):
            secs.append(_section(len(secs) % 97, s, vals[s:s + 1024]))
    for _ in range(100):
        secs.append(_section(3, 0, _coverage(rng, int(rng.integers(1, 1025)))))
    for _ in range(20):
        zooms.append(_zoom(rng))
    for blocks in (secs, zooms):
        ours = sum(len(_check(enc, b)) for b in blocks)
        z6 = sum(len(zlib.compress(b, 6)) for b in blocks)
        assert ours <= 1.25 * z6, (ours, z6, ours / z6)
