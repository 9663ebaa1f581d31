"""Which workgroup and wave of a fused decoder launch does what (iteres_amd/csrc/itx_decode_roles.h): the header built into a
stand-alone host program (tests/decode_roles_main.cpp), with the address and undefined-behaviour sanitizers, which checks every
workgroup, wave and lane for every pair of spans from {0, 1, 63, 64, 65, 129, 257} against a literal loop: one role each, one
block index or none, every block of both groups exactly once, no index beyond a span."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_wave_of_every_small_launch(tmp_path):
    exe = str(tmp_path / "decode_roles_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "decode_roles_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 7 x 7 pairs of spans
    assert r.stdout.startswith("ok 49 pairs "), r.stdout
