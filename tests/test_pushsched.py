"""The schedule of the device decoder's push pipeline (iteres_amd/csrc/itx_pushsched.h: which group a push joins, when a group is
launched, on which lane and scratch buffer, whose pass 2 a launch carries, when a flush is needed): the header built into a
stand-alone host program (tests/pushsched_main.cpp), once plain and once with the address and undefined-behaviour sanitizers. It
walks every legal order of begins and ends of up to 6 pushes for 36 configurations against a model of the caller — no refusal, each
pass of every group exactly once and on one lane, no scratch buffer reused before it was read, a wait only for what is resolved,
nothing left at the end — replays the slot sequences of tests/fusedcase.py with the launch and flush counts that
tests/test_gpu_inflate_fused.py asserts on the device, and makes the three illegal calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_every_order_of_a_few_pushes(tmp_path, sanitize):
    exe = str(tmp_path / "pushsched_main")
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-o", exe, os.path.join(ROOT, "tests", "pushsched_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # slots {1, 2, 4, 6} x group size {1, 2, 4} x (lanes, fused) {(1, 0), (2, 0), (1, 1)}
    assert r.stdout.startswith("ok 36 configurations "), r.stdout


def test_the_header_is_plain_cxx17_for_the_host(tmp_path):
    """on its own, no HIP: g++ -Wall -Werror"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "%s"\nint main() { itxp_sched s; itxp_init(&s, 1, 1, 1, 0); return s.open_grp + 1; }\n' % os.path.join(ROOT, "iteres_amd", "csrc", "itx_pushsched.h"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(tmp_path / "only"), str(src)])
    assert subprocess.run([str(tmp_path / "only")]).returncode == 0
