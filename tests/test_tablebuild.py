"""The repeat table's build without a GPU: tests/tablebuild_main.cpp, a stand-alone host program built by g++ alone, once plain and once
with the address and undefined-behaviour sanitizers. It checks the rules both builds call (iteres_amd/csrc/itx_tablebuild.h: level and bin
of a row, the sort key of binKeeperFind's return order, the running maximum of the ends as joinable summaries) each against a loop written
out there, on random and boundary rows; and the host build as a whole (tb_host_arrays of iteres_amd/csrc/itx_tablehost.h, what
ITX_TABLE_HOST=1 uploads and tests/test_gpu_table_device.py takes for the truth) against a model of the table in the plainest form, every
array and scalar element by element: the unit cases, no rows, 300 chromosomes, ties in both orders, all six bin levels, a table of more
than 2 x 65 536 rows that the build cuts into slices, and the bad rows with their code and message. The program reports how many rows and
bins it compared."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_rules_against_the_host_builds_loops(tmp_path, sanitize):
    exe = str(tmp_path / "tablebuild_main")
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-o", exe, os.path.join(ROOT, "tests", "tablebuild_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "host build against the model: " in r.stdout, r.stdout
