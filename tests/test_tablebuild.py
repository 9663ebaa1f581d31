"""The rules the device build of the repeat table shares with the host build (iteres_amd/csrc/itx_tablebuild.h: level and bin of a
row, the sort key of binKeeperFind's return order, the running maximum of the ends as joinable summaries): the header built into a
stand-alone host program (tests/tablebuild_main.cpp), once plain and once with the address and undefined-behaviour sanitizers, which
checks each rule against the loop the host build runs, on random and boundary rows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_rules_against_the_host_builds_loops(tmp_path, sanitize):
    exe = str(tmp_path / "tablebuild_main")
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-o", exe, os.path.join(ROOT, "tests", "tablebuild_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
