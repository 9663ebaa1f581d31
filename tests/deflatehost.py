"""The one-lane host build of the device DEFLATE encoder (tests/deflate_host.cpp around csrc/itx_deflate_core.h), compiled
once per directory and shared by the tests that hold the encoder to zlib and the device build to the host build."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_encoder(directory):
    """compiles the host encoder into `directory`; returns run(bytes) -> the zlib stream it makes of them"""
    so = os.path.join(str(directory), "libdeflate_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-shared", "-fPIC", "-Wall", "-o", so, os.path.join(ROOT, "tests", "deflate_host.cpp")])
    L = C.CDLL(so)
    L.itxd_deflate_host.restype = C.c_uint32
    L.itxd_deflate_host.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]

    def run(b):
        cap = ((len(b) + 16) + 3) & ~3
        out = C.create_string_buffer(cap + 64)
        n = L.itxd_deflate_host(b, len(b), out)
        assert 0 < n <= cap
        assert out.raw[cap:] == bytes(64), "wrote past its room"
        return out.raw[:n]
    return run
