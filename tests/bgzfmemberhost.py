"""The one-lane host build of the BGZF member rule (tests/bgzfmember_host.cpp around csrc/itx_bgzfmember.h), compiled once per
directory and shared by the tests that hold the rule to zlib (test_bgzf_member.py) and the device build to the host build
(test_gpu_bamout.py)."""
import ctypes as C
import os
import struct
import subprocess
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class MemberRule:
    def __init__(self, directory):
        so = os.path.join(str(directory), "libbgzfmember_host.so")
        subprocess.check_call(["g++", "-O2", "-g", "-shared", "-fPIC", "-Wall", "-o", so, os.path.join(ROOT, "tests", "bgzfmember_host.cpp")])
        L = self.L = C.CDLL(so)
        L.itx_bgzf_member_host.restype = C.c_uint32
        L.itx_bgzf_member_host.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
        L.itx_crc32_lanes_host.restype = C.c_uint32
        L.itx_crc32_lanes_host.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
        L.itx_bamout_payload_host.restype = C.c_uint32
        L.itx_bgzf_member_cap_host.restype = C.c_uint32
        L.itx_bgzf_member_cap_host.argtypes = [C.c_uint32]
        self.payload = int(L.itx_bamout_payload_host())

    def member(self, b):
        """the member the rule makes of the payload b"""
        cap = int(self.L.itx_bgzf_member_cap_host(len(b)))
        out = C.create_string_buffer(b"\xa5" * (cap + 64), cap + 64)
        n = self.L.itx_bgzf_member_host(bytes(b), len(b), out)
        assert 0 < n <= cap
        assert out.raw[cap:] == b"\xa5" * 64, "wrote past its room"
        return out.raw[:n]

    def members(self, data, tail=True):
        """the members of successive payload-sized slices of data (tail: and of the short rest, when there is one)"""
        P = self.payload
        out = [self.member(data[i:i + P]) for i in range(0, len(data) - P + 1, P)]
        if tail and len(data) % P:
            out.append(self.member(data[len(data) - len(data) % P:]))
        return out

    def crc_lanes(self, b, lanes=64):
        return int(self.L.itx_crc32_lanes_host(bytes(b), len(b), lanes))


def split_members(data):
    """the BGZF members of data, by their BSIZE"""
    out, off = [], 0
    while off < len(data):
        assert len(data) - off >= 26, "a member's frame is cut short"
        size = struct.unpack_from("<H", data, off + 16)[0] + 1
        assert off + size <= len(data), "BSIZE runs past the end"
        out.append(data[off:off + size])
        off += size
    return out


def check_member(m, payload=None):
    """every field of the frame; returns the payload it inflates to"""
    assert m[:16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b"BC" + bytes([2, 0])
    assert struct.unpack_from("<H", m, 16)[0] == len(m) - 1 and len(m) - 1 < 65536
    d = zlib.decompressobj(31)
    got = d.decompress(m)
    assert d.eof and d.unused_data == b""
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    assert crc == zlib.crc32(got) and isize == len(got)
    assert zlib.decompress(m[18:-8], -15) == got                          # raw DEFLATE between the frame's two parts
    if payload is not None:
        assert got == bytes(payload)
    return got
