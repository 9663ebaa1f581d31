"""Where a push's blocks lie among the indices of a grouped launch of the device decoder (iteres_amd/csrc/itx_inflate_group.h):
the header built into a stand-alone host program (tests/inflate_group_main.cpp), with the address and undefined-behaviour
sanitizers, which checks every index of every group of one to four slots with 0, 1, 63, 64, 65 or 129 blocks against a literal
loop."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_index_of_every_small_group(tmp_path):
    exe = str(tmp_path / "inflate_group_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "inflate_group_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 6 + 36 + 216 + 1296 groups
    assert r.stdout.startswith("ok 1554 groups "), r.stdout
