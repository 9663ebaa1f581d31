"""The bigWig files of `iteres stat` built on the device (csrc/itx_bigwig.hip, the default) against the host's zlib writer
(ITX_BW_HOST=1): the same decoded content (refio.bigwig_digest, the reference's digest where the manifest has one), and
the device's bytes the same from run to run."""
import os
import subprocess

import pytest

import goldencase as gc
import refio
from iteres_amd import build

pytestmark = pytest.mark.gpu

STAT_RUNS = [(c, r) for c, r in gc.list_runs("stat") if gc.manifest_run(c, r).get("bigwig_sha256") and gc.manifest_run(c, r)["rc"] == 0]


@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


def _run(exe, run, paths, work, env):
    work.mkdir()
    pr = subprocess.run([exe, run["cmd"]] + run["opts"] + ["-o", run["prefix"]] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, ITX_TIMING="1", **env))
    assert pr.returncode == run["rc"], pr.stderr[-2000:]
    return {fn: (work / fn).read_bytes() for fn in run["bigwig_sha256"]}, pr.stderr


@pytest.mark.parametrize("case,run_name", STAT_RUNS)
def test_device_bigwig_equals_host_writer(case, run_name, exe, tmp_path):
    run = gc.manifest_run(case, run_name)
    src = os.path.join(gc.GOLDEN, case, "in")
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", run["aln"]]]
    dev, err = _run(exe, run, paths, tmp_path / "dev", {})
    assert "bigWig: device build" in err, err[-1500:]
    again, _ = _run(exe, run, paths, tmp_path / "dev2", {})
    host, err_h = _run(exe, run, paths, tmp_path / "host", {"ITX_BW_HOST": "1"})
    assert "bigWig: device build" not in err_h
    for fn, want in run["bigwig_sha256"].items():
        assert refio.bigwig_digest(dev[fn]) == want, f"{fn}: device build differs from the reference's"
        assert refio.bigwig_digest(host[fn]) == want
        assert refio.bigwig_decode(dev[fn]) == refio.bigwig_decode(host[fn])
        assert again[fn] == dev[fn], f"{fn}: two device builds gave different bytes"
