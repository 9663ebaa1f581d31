"""Hand-made DEFLATE streams for pass 2 of the device decoder (iteres_amd/csrc/itx_inflate_core.h, itxi_resolve), which replays
64 tokens "a wave of bytes at a time": a token-level writer (stored, fixed and dynamic blocks from a list of literal runs and
(length, distance) matches), an independent replay of the same token list in plain Python, BGZF framing, and the case families
that put chosen distances on chosen lanes of a step, chosen token ends on the bitmap's and the literal stage's limits, and the
fullest scratch regions side by side. zlib writes none of these on purpose: which distance lands on which lane is left to its
hash chains, it never writes a distance above 32 506, and its literal runs are what its input makes them.

The limits come from the #defines of itx_inflate_core.h (read here with a regex), so the cases follow the constants.

What the step loop does with a case is worked out from the token list pass 1 hands over (pass2_tokens: literal runs merge
across DEFLATE blocks, a run above 255 gets a token of its own): a batch is 64 of THOSE tokens, it is replayed in steps only
when its literals fit the stage (LSTAGE - 16), and a token is taken by the steps only when it ends inside the bitmap (BMAP).
A stored prefix of several KB is therefore a run token that sends its whole batch the long way round: the families that aim at
the steps fill that batch up with (3, 1) matches (`fast`), and keep the unfilled form as well, which pins the one-token path.

Family A as the steps see it: r0 < 64 puts the first match's source into the step that starts with the block, so the step ends
in front of the match and the match starts the next one (at the step's base); r0 = 64 starts it at a base without a cut; r0 in
{65, 66, 130} starts it one or two lanes into a step whose base lies behind its source for d >= 2 (inside the step), and
r0 in {71, 95, 127}, added to the grid for that, 7, 31 and 63 lanes into it.

What the families cannot show, by the code's own slack: reading the ring for a distance in (NEAR, RING] gives the same bytes as
reading what was written back (a step reads before it writes, and only active lanes store, so the ring holds a full RING bytes
behind a step's base), and taking byte k of a self-overlapping match from k - distance instead of k % distance is LZ77's own
definition, with the step cut in front of the first such lane. So the near/far limit is pinned nowhere in (NEAR, RING]. A limit
above RING changes bytes: RING + 1 read from the ring is the byte just written (family B's RING + 1 cases).

Generation of all families (9 790 cases, 6.2 MB of expected bytes) takes 1.0 s, about 2 s with zlib's check of every
case (test_deflatecraft.py prints the figure and holds it below 15 s)."""
import bisect
import functools
import heapq
import os
import re
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE_H = os.path.join(ROOT, "iteres_amd", "csrc", "itx_inflate_core.h")


def _defines():
    text = open(CORE_H).read()
    got = {}
    for name in ("RING", "STRIPE", "LAG", "BMAP", "LSTAGE"):
        m = re.search(r"^[ \t]*#[ \t]*define[ \t]+ITXI_%s[ \t]+(\d+)u?\b" % name, text, re.M)
        assert m, "ITXI_%s: no numeric #define in %s" % (name, CORE_H)
        got[name] = int(m.group(1))
    return got


_D = _defines()
RING, STRIPE, LAG, BMAP, LSTAGE = (_D[k] for k in ("RING", "STRIPE", "LAG", "BMAP", "LSTAGE"))
NEAR = RING - 320            # ITXI_NEAR: matches up to this distance read the ring
STAGED = LSTAGE - 16         # a batch whose literals sum to at most this is staged in one piece
WAVE = 64                    # tokens per batch, bytes per step


class _Bits:
    """DEFLATE's bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def field(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.field(int(format(c, f"0{n}b")[::-1], 2), n)

    def fixed_sym(self, s):                                      # RFC 1951 3.2.6
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xC0 + s - 280, 8)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


# ------------------------------------------------------------------------------------------------------------- the writer

# RFC 1951 3.2.5
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def stored(data):
    return ("S", bytes(data))


def fixed(tokens):
    return ("F", list(tokens))


def dynamic(lit_lengths, dist_lengths, tokens):
    return ("D", list(lit_lengths), list(dist_lengths), list(tokens))


def _kraft(lengths):
    """the code space the lengths take, in units of 2^-15"""
    return sum(1 << (15 - l) for l in lengths if l)


def _canonical(lengths):
    """symbol -> (the code's bits in stream order as a field value, its length): RFC 1951 3.2.2"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[s] = (int(format(nxt[l], f"0{l}b")[::-1], 2), l)
            nxt[l] += 1
    return table


_FIXED_LIT = _canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _canonical([5] * 30)


def _check_tokens(tokens):
    for t in tokens:
        if t[0] == "L":
            assert isinstance(t[1], (bytes, bytearray))
        else:
            assert t[0] == "M" and 3 <= t[1] <= 258 and 1 <= t[2] <= 32768, t


def _put_tokens(b, lt, dt, tokens):
    field = b.field
    for t in tokens:
        if t[0] == "L":
            for ch in t[1]:
                field(*lt[ch])
        else:
            _, length, dist = t
            i = bisect.bisect_right(_LBASE, length) - 1
            field(*lt[257 + i])
            if _LEXTRA[i]:
                field(length - _LBASE[i], _LEXTRA[i])
            j = bisect.bisect_right(_DBASE, dist) - 1
            field(*dt[j])
            if _DEXTRA[j]:
                field(dist - _DBASE[j], _DEXTRA[j])
    field(*lt[256])


def rle(seq):
    """the code-length sequence as (position, symbol, extra value, extra bits, entries covered): zero runs as 17 / 18, repeats
    of a length as 16; the literal/length and the distance lengths are ONE sequence, so a run may cross from one into the other"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        n = j - i
        if v == 0:
            while n >= 11:
                r = min(n, 138)
                ops.append((j - n, 18, r - 11, 7, r))
                n -= r
            if n >= 3:
                ops.append((j - n, 17, n - 3, 3, n))
                n = 0
        else:
            ops.append((j - n, v, 0, 0, 1))
            n -= 1
            while n >= 3:
                r = min(n, 6)
                ops.append((j - n, 16, r - 3, 2, r))
                n -= r
        for k in range(n):
            ops.append((j - n + k, v, 0, 0, 1))
        i = j
    return ops


def _code_length_code(freq):
    """lengths (at most 7 bits) of a COMPLETE code for the code-length symbols in use: Huffman's, or a balanced one where that
    would be deeper; a lone symbol gets a partner so that the code is complete"""
    used = [s for s in range(19) if freq[s]]
    if len(used) == 1:
        used.append(1 if used[0] == 0 else 0)
    depth = dict.fromkeys(used, 0)
    heap = [(freq[s], k, [s]) for k, s in enumerate(used)]
    heapq.heapify(heap)
    tie = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
        tie += 1
    if max(depth.values()) > 7:
        n = len(used)
        k = (n - 1).bit_length()
        short = (1 << k) - n
        for rank, s in enumerate(sorted(used, key=lambda s: -freq[s])):
            depth[s] = k - 1 if rank < short else k
    lengths = [depth.get(s, 0) for s in range(19)]
    assert _kraft(lengths) == 1 << 15
    return lengths


def _put_dynamic_header(b, ll, dl):
    nl, nd = len(ll), len(dl)
    assert 257 <= nl <= 286 and 1 <= nd <= 30 and all(0 <= l <= 15 for l in ll + dl)
    assert ll[256], "no end-of-block code"
    assert _kraft(ll) == 1 << 15, "the literal/length code must be complete"
    assert _kraft(dl) == 1 << 15 or [l for l in dl if l] == [1], "the distance code must be complete, or one code of length 1"
    ops = rle(ll + dl)
    freq = [0] * 19
    for _, sym, _, _, _ in ops:
        freq[sym] += 1
    cl = _code_length_code(freq)
    nc = max(4, 1 + max(k for k in range(19) if cl[_CLORDER[k]]))
    b.field(nl - 257, 5)
    b.field(nd - 1, 5)
    b.field(nc - 4, 4)
    for k in range(nc):
        b.field(cl[_CLORDER[k]], 3)
    ct = _canonical(cl)
    for _, sym, extra, bits, _ in ops:
        b.field(*ct[sym])
        if bits:
            b.field(extra, bits)


def deflate(blocks):
    """the raw DEFLATE stream of a list of blocks; the last one carries BFINAL"""
    assert blocks
    b = _Bits()
    for k, blk in enumerate(blocks):
        last = k == len(blocks) - 1
        if blk[0] == "S":
            data = blk[1]
            chunks = [data[at:at + 65535] for at in range(0, len(data), 65535)] or [b""]
            for c, chunk in enumerate(chunks):
                b.field(1 if last and c == len(chunks) - 1 else 0, 1)
                b.field(0, 2)
                if b.n:
                    b.field(0, 8 - b.n)
                b.field(len(chunk), 16)
                b.field(len(chunk) ^ 0xFFFF, 16)
                b.out += chunk                   # (on a byte boundary: nothing is held back)
        elif blk[0] == "F":
            _check_tokens(blk[1])
            b.field(1 if last else 0, 1)
            b.field(1, 2)
            _put_tokens(b, _FIXED_LIT, _FIXED_DIST, blk[1])
        else:
            _, ll, dl, tokens = blk
            _check_tokens(tokens)
            b.field(1 if last else 0, 1)
            b.field(2, 2)
            _put_dynamic_header(b, ll, dl)
            _put_tokens(b, _canonical(ll), _canonical(dl), tokens)
    return b.done()


def replay(blocks):
    """what the blocks stand for: LZ77 byte by byte, no zlib, no project code"""
    out = bytearray()
    for blk in blocks:
        if blk[0] == "S":
            out += blk[1]
            continue
        for t in blk[-1]:
            if t[0] == "L":
                out += t[1]
            else:
                _, n, d = t
                if not 1 <= d <= len(out):
                    raise ValueError("distance %d with %d bytes produced" % (d, len(out)))
                for _ in range(n):
                    out.append(out[-d])
    return bytes(out)


def pass2_tokens(blocks):
    """(tokens, literals) as pass 1 hands them to pass 2: (run, length, distance) per match with run <= 255, a longer run as a token
    (run, 0, 0) in front of its match; literals: all literal bytes of the stream, those behind the last match included"""
    toks, run, n_lit = [], 0, 0
    for blk in blocks:
        if blk[0] == "S":
            run += len(blk[1])
            n_lit += len(blk[1])
            continue
        for t in blk[-1]:
            if t[0] == "L":
                run += len(t[1])
                n_lit += len(t[1])
            else:
                if run > 255:
                    toks.append((run, 0, 0))
                    run = 0
                toks.append((run, t[1], t[2]))
                run = 0
    return toks, n_lit


def frame(raw, crc, isize):
    assert len(raw) + 26 <= 65536 and isize <= 65536, (len(raw), isize)
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(raw) + 25) + raw + struct.pack("<II", crc, isize)


def member(raw, data):
    """one BGZF member around a raw DEFLATE stream of our making; data: what it inflates to (a refused stream: as many bytes
    as its trailer is to promise)"""
    return frame(raw, zlib.crc32(data) & 0xFFFFFFFF, len(data))


# ------------------------------------------------------------------------------- zlib's own streams, and the host build

def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15, memlevel=8):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, memlevel, strategy)
    return co.compress(data) + co.flush()


def corpus(rng):
    yield b""
    yield b"a"
    yield b"abc" * 5
    yield bytes(70000 % 65280)
    yield bytes(rng.integers(0, 256, 65280, dtype=np.uint8))                      # incompressible: stored blocks at level >= 1
    yield bytes(rng.integers(0, 4, 65280, dtype=np.uint8))                        # tiny alphabet: short codes, long matches
    yield (b"ACGT" * 7 + b"N") * 2200
    yield bytes(rng.integers(65, 91, 40000, dtype=np.uint8)) + bytes(25000)
    # BAM-like records: little-endian ints, names, 4-bit sequence, quality runs
    rec = bytearray()
    for i in range(400):
        rec += int(rng.integers(0, 1 << 28)).to_bytes(4, "little") * 3 + f"read{i}".encode() + b"\0" + bytes(rng.integers(0, 256, 50, dtype=np.uint8)) + bytes([40]) * 100
    yield bytes(rec)
    # far matches: a random kilobyte repeated at distances up to the 32 KiB window
    base = bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
    # ... (7000 to 8200: around the near/far limit of an 8 KiB ring; the last five: around ITXI_NEAR and ITXI_RING as they are)
    for gap in (7000, 7800, 7900, 8200, 20000, 31700, NEAR - 76, NEAR, NEAR + 1, RING, RING + 104):
        yield base + bytes(rng.integers(0, 256, gap - 1000, dtype=np.uint8)) + base + bytes(rng.integers(0, 256, 500, dtype=np.uint8)) + base[:300]
    # self-overlapping matches of every small distance
    for d in (1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 100, 257, 258, 259):
        yield bytes(rng.integers(0, 256, d, dtype=np.uint8)) * (3000 // d + 2)


def host_lib(so, flags=()):
    """the decoder's host build (tests/inflate_host.cpp, a one-lane wave) compiled to `so` with the flags, loaded"""
    import ctypes as C
    subprocess.check_call(["g++", "-O2", "-g", "-shared", "-fPIC", "-Wno-unknown-pragmas"] + list(flags) + ["-o", so, os.path.join(ROOT, "tests", "inflate_host.cpp")])
    L = C.CDLL(so)
    L.itx_inflate_host.restype = C.c_int
    L.itx_inflate_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


# ------------------------------------------------------------------------------------------------------------ the families

class _Rnd:
    """random literal bytes by the slice"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.buf, self.at = b"", 0

    def __call__(self, n):
        if self.at + n > len(self.buf):
            self.buf, self.at = bytes(self.rng.integers(0, 256, max(1 << 16, n), dtype=np.uint8)), 0
        self.at += n
        return self.buf[self.at - n:self.at]


def _case(label, blocks):
    return label, deflate(blocks), replay(blocks)


def _fill_batch(blocks):
    """(3, 1) matches behind `blocks` until the tokens so far are whole batches: what follows opens a batch of its own"""
    fill = []
    while True:
        filled = blocks + [fixed(fill)] if fill else blocks
        n = len(pass2_tokens(filled)[0])                 # (the first filler takes a long run along: two tokens)
        if n and n % WAVE == 0:
            return filled
        fill.append(("M", 3, 1))


def _produced(blocks):
    return len(replay(blocks))


A_R0 = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 66, 130)
A_R0_DEEP = (71, 95, 127)            # the first match starts 7, 31 and 63 lanes into a step: its source lies before the step's base for d above that


def family_a():
    """step grid: r0 literals, a match (l, d), two literals, a match that reads bytes written in its own step, a match whose
    source is the first match's output"""
    rnd, n = _Rnd(101), 0
    for r0 in A_R0 + A_R0_DEEP:
        for d in range(1, min(r0, 70) + 1):
            for l in sorted({min(258, max(3, l)) for l in (3, 4, 5, d - 1, d, d + 1, 2 * d, 63, 64, 65, 127, 128, 129, 257, 258)}):
                l2, d2 = ((3, 1), (4, 2))[n % 2]
                n += 1
                toks = [("L", rnd(r0)), ("M", l, d), ("L", rnd(2)), ("M", l2, d2), ("M", l, l + 2 + l2)]
                yield _case("A r0=%d d=%d l=%d then (%d,%d)" % (r0, d, l, l2, d2), [fixed(toks)])


def _with_seps(rnd, matches, first_sep=0):
    toks = []
    for k, (l, d) in enumerate(matches):
        if (k + first_sep) % 4:
            toks.append(("L", rnd((k + first_sep) % 4)))
        toks.append(("M", l, d))
    return toks


def family_b():
    """near, far and the ring; every block in two forms: `fast`, the matches in a staged batch of their own (the steps), and `slow`,
    right behind the stored prefix's run token (one token at a time)"""
    rnd = _Rnd(202)
    rng = np.random.default_rng(203)
    ds = (NEAR - 1, NEAR, NEAR + 1, NEAR + 2, RING - 1, RING, RING + 1)
    grid = [(l, d) for d in ds for l in (3, 64, 258)]

    def both(label, head, tail_of):
        for form in ("fast", "slow"):
            blocks = _fill_batch(head) if form == "fast" else head
            yield _case("B %s %s" % (label, form), blocks + [fixed(tail_of(_produced(blocks)))])

    # far lanes, near lanes and literal lanes in one step
    for k in range(4):
        order = [grid[i] for i in rng.permutation(len(grid))]
        yield from both("mixed shuffle %d" % k, [stored(rnd(RING + 400))], lambda _, order=order, k=k: _with_seps(rnd, order, k) + [("L", rnd(5))])
    dense = [(3, ds[i % 7]) for i in range(42)]
    yield from both("dense length 3", [stored(rnd(RING + 400))], lambda _: _with_seps(rnd, dense))
    # the far match's source as recent as the write-back lag allows
    for i, k in enumerate(range(0, LAG + STRIPE, 17)):
        l = (3, 64, 258)[i % 3]
        yield from both("lag k=%d l=%d" % (k, l), [stored(rnd(RING + 400))], lambda _, k=k, l=l: ([("L", rnd(k))] if k else []) + [("M", l, NEAR + 1), ("L", rnd(1 + k % 3))])
    # the source is the block's first bytes
    for l in (3, 64, 258):
        yield from both("whole block back l=%d" % l, [stored(rnd(RING + 400))], lambda n, l=l: [("M", l, n), ("L", rnd(2))])
    # distances zlib never writes
    big = [(l, d) for d in (32507, 32700, 32767, 32768) for l in (3, 258)]
    yield from both("window's end", [stored(rnd(32768))], lambda _: _with_seps(rnd, big) + [("L", rnd(3))])


def _prefixed(rnd, n, tokens):
    """n literals in front of the tokens: a stored block when they are many (the same run for pass 2, cheaper to write)"""
    return [stored(rnd(n)), fixed(tokens)] if n > 300 else [fixed([("L", rnd(n))] + tokens)]


def _runs(total, n=WAVE):
    q, r = divmod(total, n)
    return [q + 1] * r + [q] * (n - r)


def family_c():
    """batch, bitmap and stage limits"""
    rnd = _Rnd(303)
    # blocks of exactly n tokens
    for n in (0, 1, 63, 64, 65, 128, 129):
        toks = [("L", rnd(7))]
        for i in range(n):
            if i % 4:
                toks.append(("L", rnd(i % 4)))
            toks.append(("M", 3 + i % 5, 1 + i % 7))
        toks.append(("L", rnd(5)))
        assert len(pass2_tokens([fixed(toks)])[0]) == n
        yield _case("C %d tokens" % n, [fixed(toks)])
    # 64 tokens (run 0, length L) in a batch of their own: the batch's bytes end at, before and behind the bitmap's reach
    first = [t for _ in range(WAVE) for t in (("L", rnd(5)), ("M", 4, 3))]
    for L in sorted({(BMAP - 64) // WAVE, BMAP // WAVE, (BMAP + 64) // WAVE}):
        for shift in (-1, 0, 1):
            lens = [L] * WAVE
            if shift < 0:
                lens[-1] -= 1
            toks = [("L", rnd(1))] if shift > 0 else []
            toks += [("M", lens[i], (1, 2, L, 64, 300, 575)[i % 6]) for i in range(WAVE)]
            blocks = [fixed(first + toks + [("L", rnd(3))])]
            assert len(pass2_tokens(blocks)[0]) == 2 * WAVE
            yield _case("C bitmap 64 x %d %+d" % (L, shift), blocks)
    # a batch whose literals just fit, fit exactly, and do not fit the stage; first in the block and behind a batch that leaves
    # the literal cursor at 0 and at 15 mod 16
    for total in (STAGED - 1, STAGED, STAGED + 1):
        for lead in (None, 0, 15):
            toks = []
            if lead is not None:
                toks = [t for i in range(WAVE) for t in (("L", rnd(4 + (lead if i == 0 else 0))), ("M", 3, 1))]
            for i, r in enumerate(_runs(total)):
                toks += [("L", rnd(r)), ("M", 3, (1, 5, 33, 200)[i % 4] if i >= 8 else 1 + i)]
            toks.append(("L", rnd(2)))
            t2, _ = pass2_tokens([fixed(toks)])
            assert len(t2) == (WAVE if lead is None else 2 * WAVE) and sum(t[0] for t in t2[-WAVE:]) == total
            yield _case("C stage literals %d lead %s" % (total, lead), [fixed(toks)])
    # literal runs around the 8 bits a match's token has for them
    for n in (255, 256, 257, 511, 512):
        blocks = _prefixed(rnd, n, [("M", 10, n), ("L", rnd(3)), ("M", 5, 2)])
        assert len(pass2_tokens(blocks)[0]) == (2 if n <= 255 else 3)
        yield _case("C run %d" % n, blocks)
    # a run of LSTAGE literals inside a batch: not staged; the batch behind it is staged again
    head = [("L", rnd(9))] + [t for _ in range(20) for t in (("L", rnd(2)), ("M", 4, 3))]
    tail = [("M", 6, 100)] + [t for i in range(110) for t in (("L", rnd(1 + i % 3)), ("M", 3 + i % 4, 7))]
    yield _case("C run of LSTAGE inside a batch", [fixed(head), stored(rnd(LSTAGE)), fixed(tail + [("L", rnd(4))])])
    # a run token as the 64th token of a batch, its match first in the next
    toks = [t for _ in range(WAVE - 1) for t in (("L", rnd(2)), ("M", 3, 2))] + [("L", rnd(300)), ("M", 20, 150)]
    toks += [t for i in range(10) for t in (("L", rnd(i % 3)), ("M", 4, 301))]
    t2, _ = pass2_tokens([fixed(toks)])
    assert t2[WAVE - 1] == (300, 0, 0) and t2[WAVE] == (0, 20, 150)
    yield _case("C run token closes a batch", [fixed(toks)])
    # more than two stages of literals over three batches, the literal cursor odd at every refill
    toks = [("L", rnd(8)), ("M", 3, 1)] + [t for i in range(3 * WAVE - 1) for t in (("L", rnd(23)), ("M", 3 + i % 4, 1 + i % 23))] + [("L", rnd(9))]
    t2, n_lit = pass2_tokens([fixed(toks)])
    assert len(t2) == 3 * WAVE and n_lit > 2 * LSTAGE and sum(t[0] for t in t2[:WAVE]) % 16 == 1
    yield _case("C three batches of literals", [fixed(toks)])


def fullest_region_blocks():
    """stream (a) of test_code_lengths_staged_in_the_fullest_scratch_region: 21 801 tokens, 87 KB of them, and a second block"""
    return [fixed([("L", b"a")] + [("M", 3, 1)] * 21800), fixed([("L", b"bcd"), ("M", 3, 1)])]


def family_d():
    """the fullest scratch regions side by side: 65 536 literals, 21 801 tokens, 65 536 literals"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    aaaa = co.compress(b"A" * 65536) + co.flush()
    yield "D 65536 literals, first", aaaa, b"A" * 65536
    yield _case("D 21801 tokens", fullest_region_blocks())
    yield "D 65536 literals, second", aaaa, b"A" * 65536


# code-length sets for family E
E_DEEP_SYMS = [101, 32, 116, 97, 111, 110, 105, 115, 114, 104, 108, 100, 117, 257, 256, 258]      # lengths 1, 2, .. 15, 15
E_ALL_LIT = [8] * 226 + [9] * 60                                   # all 286 symbols
E_CROSS16_LIT = [0] * 97 + [3, 3, 4, 4, 4, 4] + [0] * 153 + [3, 3, 3, 3]      # 'a'..'f', then 256..259 at 3 bits: the threes run on into ...
E_CROSS16_DIST = [3] * 8                                           # ... eight distance codes of 3 bits
E_CROSS18_LIT = [8] * 242 + [9] * 28 + [0] * 16                    # sixteen zeros at the end run on into ...
E_CROSS18_DIST = [0, 0, 0, 2, 2, 2, 2]                             # ... three zeros


def family_e(with_corpus=True):
    """pass 1's code shapes: hand-made dynamic blocks (15-bit literal codes, a single distance code, code-length repeats that
    cross from the literal lengths into the distance lengths) between zlib's own of the corpus, uncut up to 65 280 bytes"""
    rnd = _Rnd(404)
    rng = np.random.default_rng(405)
    made = []
    for v in range(8):
        # 15-bit codes: which symbol is how deep turns with v
        syms = E_DEEP_SYMS[v:] + E_DEEP_SYMS[:v]
        ll = [0] * 259
        for k, s in enumerate(syms):
            ll[s] = min(k + 1, 15)
        lits = [s for s in syms if s < 256]
        toks = [("L", bytes(lits))]
        for _ in range(120):
            toks.append(("L", bytes(lits[int(i)] for i in rng.integers(0, len(lits), int(rng.integers(1, 6))))))
            toks.append(("M", 3 + int(rng.integers(0, 2)), 1 + int(rng.integers(0, 4))))
        made.append(_case("E 15-bit codes, turn %d" % v, [dynamic(ll, [2, 2, 2, 2], toks)]))
        # a single distance code
        k = (0, 4, 10)[v % 3]
        toks = [("L", rnd(60))]
        for _ in range(80):
            toks += [("M", 3 + int(rng.integers(0, 256)), _DBASE[k] + int(rng.integers(0, 1 << _DEXTRA[k]))), ("L", rnd(int(rng.integers(0, 4))))]
        made.append(_case("E single distance code %d, %d" % (k, v), [dynamic(E_ALL_LIT, [0] * k + [1], toks)]))
        # a repeat of a length (16) and of zeros (18) across the two codes
        toks = [("L", b"abcdef")]
        for _ in range(100):
            toks += [("L", bytes(97 + int(i) for i in rng.integers(0, 6, int(rng.integers(0, 5))))), ("M", 3 + int(rng.integers(0, 3)), 1 + int(rng.integers(0, 6)))]
        made.append(_case("E 16 crosses, %d" % v, [dynamic(E_CROSS16_LIT, E_CROSS16_DIST, toks)]))
        toks = [("L", rnd(40))]
        for _ in range(100):
            toks += [("L", rnd(int(rng.integers(0, 5)))), ("M", 3 + int(rng.integers(0, 20)), 4 + int(rng.integers(0, 9)))]
        made.append(_case("E 18 crosses, %d" % v, [dynamic(E_CROSS18_LIT, E_CROSS18_DIST, toks)]))
    if not with_corpus:
        yield from made
        return
    theirs = []
    for n, data in enumerate(corpus(np.random.default_rng(406))):
        data = data[:65280]
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)):
            raw = raw_deflate(data, level, strategy)
            if len(raw) + 26 <= 65536:               # (random bytes in the fixed code: no BGZF member holds them)
                theirs.append(("E zlib corpus %d level %d strategy %d" % (n, level, strategy), raw, data))
    # in turn, so that the lanes of one pass-1 wave hold blocks of every kind
    for k in range(max(len(made), len(theirs))):
        if k < len(theirs):
            yield theirs[k]
        if k < len(made):
            yield made[k]


def family_f():
    """refusals between good members: (label, raw, data, status); data of a refused member: zeros, as many as its trailer promises"""
    rnd = _Rnd(505)
    good = [("L", rnd(20)), ("M", 5, 7), ("L", rnd(3))]
    yield ("F good 0",) + _case("", [fixed(good)])[1:] + (0,)
    yield "F distance = produced + 1", deflate([fixed([("L", rnd(10)), ("M", 5, 11)])]), bytes(15), 7
    yield ("F good 1",) + _case("", [fixed(good + [("M", 40, 1)])])[1:] + (0,)
    toks = [("L", rnd(4))] + [("M", 3, 1)] * 70
    yield "F distance = produced + 1 in the second batch", deflate([fixed(toks + [("M", 3, 4 + 210 + 1)])]), bytes(4 + 210 + 3), 7
    yield ("F good 2",) + _case("", [fixed(good + [("M", 9, 2)])])[1:] + (0,)
    yield "F one byte past usize", deflate([fixed([("L", rnd(10)), ("M", 5, 3)])]), bytes(14), 2
    yield ("F good 3",) + _case("", [fixed(good + [("M", 258, 28)])])[1:] + (0,)


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f}


@functools.lru_cache(maxsize=None)
def cases(name):
    """the cases of one family, made once per process"""
    return tuple(FAMILIES[name]())


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """every hand-made well-formed case (A - D and E's own blocks)"""
    return cases("A") + cases("B") + cases("C") + cases("D") + tuple(family_e(with_corpus=False))


B_PHASES = (0, 1, 3, 255)


def phased(family, phases=B_PHASES):
    """(label, member, expected) of a family with every member at g0 % 256 == phase, for each phase in turn: a filler member in
    front of each brings the output offset there (1, 3 and 255 bytes in front of the first; 0 bytes: none)"""
    rnd = _Rnd(606)
    out, at = [], 0
    for phase in phases:
        for label, raw, want in family:
            fill = (phase - at) % 256
            if fill:
                data = rnd(fill)
                out.append(("filler of %d" % fill, member(deflate([stored(data)]), data), data))
                at += fill
            out.append(("%s @%d" % (label, phase), member(raw, want), want))
            at += len(want)
    return out
