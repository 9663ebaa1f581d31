"""One scenario of tests/test_gpu_inflate_fused.py, run in a process of its own (ITX_FUSE / ITX_GROUP are read once per process):
pushes of small BGZF blocks through itx_bamwin_push_begin / push_copied / push_end on up to 12 slots, every window's bytes compared
with zlib here, and one JSON line for the parent: the status bytes of every push and a digest of every window.
    python tests/fusedcase.py <scenario>"""
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iteres_amd import engine as eng  # noqa: E402

SLOTS = 12                       # ITX_BAMWIN_LANES_DEFAULT: the slots an inflater sets up
WINDOWS = 16                     # the ring the command rotates its pushes through (slots + 4)
SIZES = (1, 63, 64, 65, 129, 0)  # blocks per push, in turn
E_BTYPE, E_DIST = 3, 7           # itx_inflate_core.h


def content(rng, kind, n):
    """n bytes that look like BAM records of mkbam's three contents: names, packed bases, and qualities that are wide and
    noisy (legacy), 40 values on a slowly falling level (hiseq) or four bins in runs (novaseq)"""
    out = bytearray()
    i = int(rng.integers(0, 1 << 20))
    while len(out) < n:
        name = b"read.%d\0" % i
        i += 1
        bases = bytes(rng.integers(0, 256, 50, dtype=np.uint8) & 0x77 | 0x11)
        if kind == "legacy":
            qual = bytes(rng.integers(0, 42, 100, dtype=np.uint8))
        elif kind == "hiseq":
            level = 41 - np.arange(100) // 8
            qual = bytes(np.clip(level - rng.integers(0, 6, 100), 2, 41).astype(np.uint8))
        else:
            qual = bytes(np.repeat(np.array([2, 12, 23, 37], np.uint8)[rng.integers(0, 4, 10)], 10))
        core = struct.pack("<iiIIiiii", int(rng.integers(0, 24)), int(rng.integers(0, 1 << 27)), len(name) | 30 << 8, 1 | 16 << 16, 100, -1, -1, 0)
        rec = core + name + struct.pack("<I", 100 << 4) + bases + qual
        out += struct.pack("<I", len(rec)) + rec
    return bytes(out[:n])


def member(data, kind):
    """one BGZF block whose deflate stream is stored, fixed-Huffman or dynamic"""
    level, strategy = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "dynamic": (6, zlib.Z_DEFAULT_STRATEGY)}[kind]
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return frame(co.compress(data) + co.flush(), zlib.crc32(data) & 0xFFFFFFFF, len(data))


def frame(deflated, crc, isize):
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(deflated) + 25) + deflated + struct.pack("<II", crc, isize)


def far_match_member():
    """a fixed-Huffman block whose first token is a match of length 3 at distance 1: it reaches before the start of the block.
    Bits, in stream order: BFINAL 1, BTYPE 01 (sent low bit first: 1 0), length symbol 257 = 0000001, distance symbol 0 = 00000, end
    of block = 0000000"""
    bits = [1, 1, 0] + [0, 0, 0, 0, 0, 0, 1] + [0] * 5 + [0] * 7
    bits += [0] * (-len(bits) % 8)
    raw = bytes(sum(b << k for k, b in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))
    try:
        zlib.decompress(raw, -15)
    except zlib.error:
        return frame(raw, 0, 3)
    raise AssertionError("zlib takes the block with the far match")


def make_push(rng, n_blocks, at, btype3=None, far=None):
    """(compressed bytes, block list, expected bytes per block): n_blocks blocks of 1 .. 6000 bytes; the three block types and the
    three contents in turn (`at` shifts the turn from push to push); block btype3 gets block type 3, block far a far match"""
    parts, want = [], []
    for i in range(n_blocks):
        data = content(rng, ("legacy", "hiseq", "novaseq")[(i // 3 + at) % 3], int(rng.integers(1, 6000)))
        m = bytearray(member(data, ("stored", "fixed", "dynamic")[(i + at) % 3]))
        if btype3 == i:
            m[18] |= 0x06                      # block type 3: no decoder may accept it
        if far == i:
            m, data = bytearray(far_match_member()), b"\0\0\0"
        parts.append(bytes(m))
        want.append(data)
    comp = b"".join(parts)
    blocks = eng.index_bgzf(comp) if n_blocks else np.zeros(0, eng.BGZF_BLOCK)
    assert len(blocks) == n_blocks
    return comp, blocks, want


class Pipe:
    def __init__(self):
        L = self.L = eng.load()
        L.itx_bamwin_push_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.itx_bamwin_push_copied.argtypes = [C.c_void_p, C.c_int]
        L.itx_bamwin_push_end.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
        self.inf = eng.Inflater()
        self.h = self.inf._h
        self.keep = []                     # the callers' buffers stay alive to the end
        self.result = {}

    def begin(self, k, push):
        comp, blocks = push[0], push[1]
        cbuf = np.zeros(len(comp) + 16, np.uint8)
        cbuf[:len(comp)] = np.frombuffer(comp, np.uint8)
        blocks = np.ascontiguousarray(blocks, eng.BGZF_BLOCK)
        self.keep += [cbuf, blocks]
        eng._chk(self.L.itx_bamwin_push_begin(self.h, k % WINDOWS, k % SLOTS, eng._p(cbuf), len(comp), eng._p(blocks), len(blocks)), "push_begin")

    def copied(self, k):
        eng._chk(self.L.itx_bamwin_push_copied(self.h, k % SLOTS), "push_copied")

    def end(self, k, push, hurt=()):
        """status and window of push k; every block but those of `hurt` ({block: status}) must be clean and equal to zlib's bytes"""
        hurt = dict(hurt)
        blocks, want = push[1], push[2]
        name = (lambda i: push[3][i]) if len(push) > 3 else (lambda i: "")        # a crafted block's label, for the messages
        status = np.full(len(blocks) + 1, 255, np.uint8)
        n_new = C.c_size_t()
        eng._chk(self.L.itx_bamwin_push_end(self.h, k % SLOTS, eng._p(status), C.byref(n_new)), "push_end")
        assert status[len(blocks)] == 255
        status = status[:len(blocks)]
        assert n_new.value == sum(len(d) for d in want), (k, n_new.value)
        raw = np.zeros(n_new.value + 1, np.uint8)
        if n_new.value:
            eng._chk(self.L.itx_bamwin_peek(self.h, k % WINDOWS, 0, eng._p(raw), n_new.value), "peek")
        at = 0
        for i, d in enumerate(want):
            got = raw[at:at + len(d)].tobytes()
            at += len(d)
            if i in hurt:
                assert status[i] == hurt[i], (k, i, int(status[i]))
                raw[at - len(d):at] = 0               # whatever lies behind a flagged block is not part of the digest
            else:
                assert status[i] == 0, (k, i, name(i), int(status[i]))
                assert got == zlib.decompress(push[0][int(blocks["coff"][i]) + 18:int(blocks["coff"][i]) + int(blocks["csize"][i]) - 8], -15) == d, (k, i, name(i))
        self.result[k] = {"status": [int(x) for x in status], "window": hashlib.sha256(raw[:n_new.value].tobytes()).hexdigest()}

    def close(self):
        self.inf.close()


def in_order(pipe, pushes, hurt=None):
    """what the reader's producer does: begin while a slot is free, else end the oldest"""
    begun = ended = 0
    while ended < len(pushes):
        if begun < len(pushes) and begun - ended < SLOTS:
            pipe.begin(begun, pushes[begun])
            begun += 1
        else:
            pipe.end(ended, pushes[ended], (hurt or {}).get(ended, ()))
            ended += 1


def crafted_pushes():
    """the hand-made members of tests/deflatecraft.py (families B, C and D: the ring's, the bitmap's and the stage's limits, the fullest
    scratch regions) as pushes of 64, 65 and 3 blocks in turn; then the three fullest regions as the last blocks of one push and
    the first of the next, cut behind the second and behind the first. In the fused launch four replaying waves share one LDS
    block and a group's scratch regions abut: what one overruns, a neighbour loses."""
    import deflatecraft as dc
    ms = [(dc.member(raw, want), want, label) for name in "BCD" for label, raw, want in dc.cases(name)]
    d0, d1, d2 = ms[-3:]
    small = ms[len(dc.cases("B")):-3]                  # family C
    sets, at, k = [], 0, 0
    while at < len(ms):
        n = (64, 65, 3)[k % 3]
        sets.append(ms[at:at + n])
        at += n
        k += 1
    sets += [(small * 2)[:62] + [d0, d1], [d2] + (small * 2)[:64], [small[0], small[1], d0], [d1, d2] + (small * 2)[:62]]
    pushes = []
    for members in sets:
        comp = b"".join(m for m, _, _ in members)
        blocks = eng.index_bgzf(comp)
        assert len(blocks) == len(members)
        pushes.append((comp, blocks, [w for _, w, _ in members], [label for _, _, label in members]))
    return pushes


def sized(rng, n_pushes, first=0):
    return [make_push(rng, SIZES[(first + k) % len(SIZES)], k) for k in range(n_pushes)]


def main():
    scenario = sys.argv[1]
    assert int(os.environ.get("ITX_GROUP", "4")) == 4 and int(os.environ.get("ITX_LANES", "1")) == 1
    rng = np.random.default_rng(2026)
    pipe = Pipe()
    if scenario.startswith("flush"):
        # one group only, of 1, 2 or 4 slots: its pass 2 has no later launch to go with
        pushes = [make_push(rng, n, k) for k, n in enumerate((65, 129, 1, 64)[:int(scenario[5:])])]
        in_order(pipe, pushes)
    elif scenario.startswith("groups"):
        # 2, 3 or 5 groups back to back, slots of 1, 63, 64, 65, 129 and 0 blocks in turn, the last group partial: 4 (g - 1) + 3
        # pushes with blocks and the empty ones between them (5 groups: 19 pushes, so slots, windows' groups and both scratch
        # buffers are used again)
        g = int(scenario[6:])
        n = 0
        while sum(1 for k in range(n) if SIZES[k % len(SIZES)]) < 4 * (g - 1) + 3:
            n += 1
        in_order(pipe, sized(rng, n))
    elif scenario == "newest_first":
        # two full groups and two members of a third; the newest push is ended first: the open group is launched short and flushed;
        # then the older ones, newest to oldest
        pushes = [make_push(rng, n, k) for k, n in enumerate((64, 1, 129, 63, 65, 65, 2, 130, 64, 33))]
        for k, p in enumerate(pushes):
            pipe.begin(k, p)
        for k in reversed(range(len(pushes))):
            pipe.end(k, pushes[k])
    elif scenario == "all12":
        # every slot in flight before the first push_end
        pushes = [make_push(rng, SIZES[k % 5], k) for k in range(SLOTS)]
        for k, p in enumerate(pushes):
            pipe.begin(k, p)
        for k in range(SLOTS):
            pipe.copied(k)
        for k, p in enumerate(pushes):
            pipe.end(k, p)
    elif scenario == "damaged":
        # three groups; in the second, a block of type 3 in one slot and a match that reaches before its block in another: their
        # pass 2 runs in the third group's launch
        sizes = (64, 65, 1, 63, 40, 65, 33, 64, 65, 129, 1)
        pushes = [make_push(rng, n, k, btype3=17 if k == 5 else None, far=5 if k == 6 else None) for k, n in enumerate(sizes)]
        in_order(pipe, pushes, hurt={5: {17: E_BTYPE}, 6: {5: E_DIST}})
    elif scenario == "crafted":
        in_order(pipe, crafted_pushes())
    else:
        raise SystemExit("unknown scenario " + scenario)
    pipe.close()
    print("RESULT " + json.dumps({"scenario": scenario, "fuse": os.environ.get("ITX_FUSE", ""), "pushes": [pipe.result[k] for k in sorted(pipe.result)]}), flush=True)


if __name__ == "__main__":
    main()
