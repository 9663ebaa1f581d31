"""The host build of the member levels (tests/bgzflevels_host.cpp around csrc/itx_bgzflevels.h), compiled once per directory and
shared by the tests that hold the levels to zlib (test_bgzf_levels.py) and the device build to the host build
(test_gpu_bamout_levels.py). A "wave" of several lanes is as many threads that meet at a barrier where the device has one."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bgzflevels_host.cpp")


class LevelRule:
    def __init__(self, directory):
        so = os.path.join(str(directory), "libbgzflevels_host.so")
        subprocess.check_call(["g++", "-O2", "-g", "-shared", "-fPIC", "-Wall", "-pthread", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.itx_bgzf_member_level_host.restype = C.c_uint32
        L.itx_bgzf_member_level_host.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        L.itx_bgzf_member_plain_host.restype = C.c_uint32
        L.itx_bgzf_member_plain_host.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
        L.itx_bgzf_levels_payload_host.restype = C.c_uint32
        L.itx_bgzf_levels_slice_host.restype = C.c_uint32
        L.itx_bgzf_levels_cap_host.restype = C.c_uint32
        L.itx_bgzf_levels_cap_host.argtypes = [C.c_uint32]
        self.payload = int(L.itx_bgzf_levels_payload_host())
        self.slice = int(L.itx_bgzf_levels_slice_host())

    def _call(self, b, fn):
        cap = int(self.L.itx_bgzf_levels_cap_host(len(b)))
        out = C.create_string_buffer(b"\xa5" * (cap + 64), cap + 64)
        assert C.addressof(out) % 4 == 0
        n = fn(bytes(b), len(b), out)
        assert 0 < n <= cap
        assert out.raw[cap:] == b"\xa5" * 64, "wrote past its room"
        return out.raw[:n]

    def member(self, b, level, lanes=1):
        """the member of `level` the rule makes of the payload b with `lanes` lanes"""
        return self._call(b, lambda src, n, out: self.L.itx_bgzf_member_level_host(src, n, out, level, lanes))

    def plain(self, b):
        """itx_bgzf_member itself (csrc/itx_bgzfmember.h), not through the level call"""
        return self._call(b, self.L.itx_bgzf_member_plain_host)

    def members(self, data, level, tail=True):
        """the members of successive payload-sized slices of data (tail: and of the short rest, when there is one)"""
        P = self.payload
        out = [self.member(data[i:i + P], level) for i in range(0, len(data) - P + 1, P)]
        if tail and len(data) % P:
            out.append(self.member(data[len(data) - len(data) % P:], level))
        return out


def build_sanitized(directory):
    """the stand-alone program of the same source under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = os.path.join(str(directory), "bgzflevels_san")
    r = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBGZFLEVELS_MAIN",
                        "-Wall", "-pthread", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
