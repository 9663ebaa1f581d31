"""The host program's alignment reader as a CPU-only test tool: the reader's sources and the one compile line that links
them, each a translation unit of its own as in the product, behind a small main of iteres_amd/host/test/ (reader_dump.c,
split_dump.c, share_dump.c). ALN_SEPARATE_UNITS tells the main that it is built this way (test/reader_units.h)."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iteres_amd", "host")
READER_SOURCES = ("bgzf.c", "bamio.c", "bamdev.c", "samio.c", "tables.c")


def build(exe, main_c, extra=()):
    """compiles iteres_amd/host/test/<main_c> with the reader (and the host sources named in `extra`) into exe"""
    subprocess.check_call(["gcc", "-O2", "-g", "-fopenmp", "-std=gnu11", "-DALN_SEPARATE_UNITS", "-o", exe, os.path.join(HOST, "test", main_c)]
                          + [os.path.join(HOST, s) for s in tuple(extra) + READER_SOURCES] + ["-lz", "-ldl"])
    return exe
