"""The hand-made DEFLATE streams of tests/deflatecraft.py before any of them reaches a GPU: the writer against zlib and against the
plain replay of the same token list (two oracles that share no code), then every case through the host build of the decoder
(tests/inflate_host.cpp, a one-lane wave: it pins the bytes, the region and the buffers, and says nothing about where a 64-lane
step ends — that is tests/test_gpu_inflate_crafted.py), and the refusals."""
import ctypes as C
import re
import time
import zlib

import pytest

import deflatecraft as dc
from test_inflate_core import run

@pytest.fixture(scope="module", params=[[], ["-DITXI_SIMPLE_IN"]], ids=["fifo", "word_ahead"])
def lib(request, tmp_path_factory):
    return dc.host_lib(str(tmp_path_factory.mktemp("craft") / "libinflate_host.so"), request.param)


def test_the_constants_are_the_header_s():
    text = open(dc.CORE_H).read()
    assert re.search(r"#define ITXI_NEAR \(ITXI_RING - 320u\)", text) and dc.NEAR == dc.RING - 320
    assert "lit_total <= ITXI_LSTAGE - 16u" in text and dc.STAGED == dc.LSTAGE - 16
    assert dc.RING % dc.STRIPE == 0 and dc.LAG + dc.STRIPE + 258 < dc.NEAR - 258


def test_replay_by_hand():
    blocks = [dc.stored(b"xy"), dc.fixed([("L", b"ab"), ("M", 5, 2), ("M", 3, 1), ("M", 4, 12)])]
    assert dc.replay(blocks) == b"xy" + b"ab" + b"ababa" + b"aaa" + b"xyab"
    with pytest.raises(ValueError):
        dc.replay([dc.fixed([("L", b"ab"), ("M", 3, 3)])])


def test_generation_stays_quick():
    t0 = time.perf_counter()
    n = sum(1 for name in "ABCDEF" for _ in dc.FAMILIES[name]())
    took = time.perf_counter() - t0
    print("deflatecraft: %d cases in %.2f s" % (n, took))
    assert took < 15.0


def test_every_family_has_what_it_is_for():
    a = dc.cases("A")
    assert 3000 < len(a) < 10000 and 1_000_000 < sum(len(w) for _, _, w in a) < 3_000_000
    assert len({label for label, _, _ in dc.crafted_cases()}) == len(dc.crafted_cases())
    assert sum(1 for label, _, _ in dc.cases("B") if " lag " in label and label.endswith("fast")) >= 64
    assert [len(w) for _, _, w in dc.cases("D")] == [65536, 1 + 3 * 21800 + 3 + 3, 65536]
    assert max(len(w) for _, _, w in dc.cases("E")) == 65280
    # the code-length repeats do cross from the literal/length lengths into the distance lengths
    for ll, dl, sym in ((dc.E_CROSS16_LIT, dc.E_CROSS16_DIST, 16), (dc.E_CROSS18_LIT, dc.E_CROSS18_DIST, 18)):
        assert any(s == sym and at < len(ll) < at + n for at, s, _, _, n in dc.rle(ll + dl))


def test_writer_against_zlib_and_replay():
    """zlib.decompress(raw) == replay(blocks) (the cases' expected bytes are the replay's; D's literal members and E's corpus are zlib's own)"""
    n = 0
    for name in "ABCDE":
        for label, raw, want in dc.cases(name):
            assert zlib.decompress(raw, -15) == want, label
            m = dc.member(raw, want)
            assert len(m) == len(raw) + 26
            n += 1
    assert n > 6000


def test_tokens_as_pass_one_hands_them_over(lib):
    """pass2_tokens, by which the families count batches, against the host build's own count"""
    import numpy as np
    rnd = dc._Rnd(1)
    for blocks in (dc.fullest_region_blocks(), [dc.stored(rnd(300)), dc.fixed([("M", 3, 1), ("L", rnd(255)), ("M", 4, 2), ("L", rnd(256)), ("M", 4, 2), ("L", rnd(9))])],
                   dc._fill_batch([dc.stored(rnd(5000))]), dc._fill_batch([dc.fixed([("L", rnd(5)), ("M", 3, 1)])])):
        raw, want = dc.deflate(blocks), dc.replay(blocks)
        buf = np.zeros(len(raw) // 4 + 8, np.uint32)
        buf.view(np.uint8)[:len(raw)] = np.frombuffer(raw, np.uint8)
        out = np.zeros(len(want) + 64, np.uint8)
        n_lit, n_tok = C.c_uint32(), C.c_uint32()
        assert lib.itx_inflate_host(buf.ctypes.data, 0, len(raw), out.ctypes.data, 0, len(want), C.byref(n_lit), C.byref(n_tok)) == 0
        toks, lits = dc.pass2_tokens(blocks)
        assert (n_tok.value, n_lit.value) == (len(toks), lits)
    assert len(dc.pass2_tokens(dc.fullest_region_blocks())[0]) == 21801


def test_host_build_every_case(lib):
    n = 0
    for name in "ABCDE":
        for label, raw, want in dc.cases(name):
            rc, got = run(lib, raw, len(want), n % 4, (0, 3, 255, 256, 70001)[n % 5])
            assert rc == 0, (label, rc)
            assert got == want, label
            n += 1


def test_refusals(lib):
    seen = []
    for label, raw, data, status in dc.cases("F"):
        rc, got = run(lib, raw, len(data), 1, 3)
        assert rc == status, (label, rc)
        seen.append(status)
        z = zlib.decompressobj(-15)
        if status == 0:
            assert got == data and z.decompress(raw) == data and z.eof
        elif status == 7:
            with pytest.raises(zlib.error):                      # "invalid distance too far back"
                z.decompress(raw)
        else:
            # a well-formed stream of one byte more than the member's trailer promises: zlib cannot end it inside usize bytes
            z.decompress(raw, len(data))
            assert status == 2 and not z.eof and len(zlib.decompress(raw, -15)) == len(data) + 1
    assert seen == [0, 7, 0, 7, 0, 2, 0]
