"""One scenario of tests/test_gpu_inflate_groups.py, run in a process of its own (ITX_GROUP / ITX_LANES are read once per
process): pushes of small BGZF blocks through itx_bamwin_push_begin / push_copied / push_end, every window's bytes compared
with zlib here, and one JSON line for the parent: the status bytes of every push and a digest of every window.
    python tests/groupcase.py <scenario>"""
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

IN_FLIGHT = 8                    # ITX_BAMWIN_LANES_DEFAULT: the slots an inflater sets up


def member(data, kind):
    """one BGZF block whose deflate stream is stored, fixed-Huffman or dynamic"""
    level, strategy = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "dynamic": (6, zlib.Z_DEFAULT_STRATEGY)}[kind]
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    comp = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def make_push(rng, n_blocks, damage=None):
    """(compressed bytes, block list, expected bytes per block): n_blocks blocks of 1 .. 3000 bytes, the three block types in turn"""
    parts, want = [], []
    for i in range(n_blocks):
        n = int(rng.integers(1, 3000))
        data = bytes(rng.integers(0, int(rng.choice([4, 40, 256])), n, dtype=np.uint8))
        kind = ("stored", "fixed", "dynamic")[i % 3]
        m = bytearray(member(data, kind))
        if damage == i:
            m[18] |= 0x06                      # block type 3: no decoder may accept it
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
        self.result = []

    def begin(self, k, push):
        comp, blocks, _ = push
        cbuf = np.zeros(len(comp) + 16, np.uint8)
        cbuf[:len(comp)] = np.frombuffer(comp, np.uint8)
        blocks = np.ascontiguousarray(blocks, eng.BGZF_BLOCK)
        self.keep += [cbuf, blocks]
        eng._chk(self.L.itx_bamwin_push_begin(self.h, k % IN_FLIGHT, k % IN_FLIGHT, eng._p(cbuf), len(comp), eng._p(blocks), len(blocks)), "push_begin")

    def copied(self, k):
        eng._chk(self.L.itx_bamwin_push_copied(self.h, k % IN_FLIGHT), "push_copied")

    def end(self, k, push, hurt=None):
        """status and window of push k; every block but `hurt` must be clean and equal to zlib's bytes"""
        _, blocks, want = push
        status = np.full(len(blocks) + 1, 255, np.uint8)
        n_new = C.c_size_t()
        eng._chk(self.L.itx_bamwin_push_end(self.h, k % IN_FLIGHT, eng._p(status), C.byref(n_new)), "push_end")
        status = status[:len(blocks)]
        assert n_new.value == sum(len(d) for d in want), (k, n_new.value)
        raw = np.zeros(n_new.value + 1, np.uint8)
        if n_new.value:
            eng._chk(self.L.itx_bamwin_peek(self.h, k % IN_FLIGHT, 0, eng._p(raw), n_new.value), "peek")
        at = 0
        for i, d in enumerate(want):
            got = raw[at:at + len(d)].tobytes()
            at += len(d)
            if i == hurt:
                assert status[i] == 3, (k, i, int(status[i]))
                raw[at - len(d):at] = 0               # whatever lies behind a flagged block is not part of the digest
            else:
                assert status[i] == 0, (k, i, int(status[i]))
                assert got == zlib.decompress(push[0][int(blocks["coff"][i]) + 18:int(blocks["coff"][i]) + int(blocks["csize"][i]) - 8], -15) == d, (k, i)
        self.result.append({"status": [int(x) for x in status], "window": hashlib.sha256(raw[:n_new.value].tobytes()).hexdigest()})

    def close(self):
        self.inf.close()


def in_order(pipe, pushes, hurt_push=None, hurt_block=None):
    """what the reader's producer does: begin while a slot is free, else end the oldest"""
    begun = ended = 0
    while ended < len(pushes):
        if begun < len(pushes) and begun - ended < IN_FLIGHT:
            pipe.begin(begun, pushes[begun])
            begun += 1
        else:
            pipe.end(ended, pushes[ended], hurt_block if ended == hurt_push else None)
            ended += 1


def main():
    scenario = sys.argv[1]
    G, Ln = int(os.environ.get("ITX_GROUP", "1")), int(os.environ.get("ITX_LANES", "4"))
    rng = np.random.default_rng(2024)
    pipe = Pipe()
    if scenario == "sizes":
        # slots of 1, 63, 64, 65 and 129 blocks and one without any, begun back to back: groups of G, the last one partial
        pushes = [make_push(rng, n) for n in (1, 63, 0, 64, 65, 129, 129, 1)]
        in_order(pipe, pushes)
    elif scenario == "partial":
        # G - 1 begins, the copies waited for, then the first push_end has to launch the group
        pushes = [make_push(rng, n) for n in (65, 1, 64, 63)[:max(G - 1, 1)]]
        for k, p in enumerate(pushes):
            pipe.begin(k, p)
        for k in range(len(pushes)):
            pipe.copied(k)
        for k, p in enumerate(pushes):
            pipe.end(k, p)
    elif scenario == "damaged":
        # one block of type 3 in the third of four slots
        pushes = [make_push(rng, n, damage=17 if k == 2 else None) for k, n in enumerate((40, 65, 33, 64))]
        in_order(pipe, pushes, hurt_push=2, hurt_block=17)
    elif scenario == "reuse":
        # 2 G L + 1 pushes: every lane's scratch is used again by a later group
        pushes = [make_push(rng, int(rng.integers(20, 70))) for _ in range(2 * G * Ln + 1)]
        in_order(pipe, pushes)
    else:
        raise SystemExit("unknown scenario " + scenario)
    pipe.close()
    print("RESULT " + json.dumps({"scenario": scenario, "group": G, "lanes": Ln, "pushes": pipe.result}), flush=True)


if __name__ == "__main__":
    main()
