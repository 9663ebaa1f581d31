"""GPU: `iteres filter -W`, the command, on the inputs of tests/gcovcase.py make_inputs. The two bigWig files decode to what the
model of tests/bwsparse.py gives for the run's own bedGraph text (which tests/test_gpu_gcov_cli.py compares with the reference's
counted reads), and, where oracle/_ref/libcuskent.a and gcc exist, to what the reference's converter makes of that text."""
import filecmp
import os
import re
import subprocess

import pytest

import bwsparse as bs
import gcovcase as gv
from iteres_amd import build

pytestmark = pytest.mark.gpu

GRAPHS = ["out_ALL.iteres.bedGraph", "out_ALL.iteres.unique.bedGraph"]
BIGWIGS = ["out_ALL.iteres.bigWig", "out_ALL.iteres.unique.bigWig"]


@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gcov_bw_cli") / "in")
    gv.make_inputs(d)
    return d


def run_filter(exe, d, out, opts, aln="reads.bam", env=None):
    os.makedirs(out, exist_ok=True)
    pr = subprocess.run([exe, "filter"] + list(opts) + ["-o", "out", os.path.join(d, "chrom.sizes"), os.path.join(d, "rep.sizes"), os.path.join(d, "rmsk.txt"),
                         os.path.join(d, aln)], cwd=out, capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, ITX_TIMING="1", ITX_BGZF_CHUNK="40000", **(env or {})))
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr


def decoded(out):
    return [bs.decode(open(os.path.join(out, fn), "rb").read()) for fn in BIGWIGS]


@pytest.fixture(scope="module")
def both(inputs, exe, tmp_path_factory):
    """-G -W: the four files; the bigWigs are the model's (and the reference's) conversion of the run's own text"""
    out = str(tmp_path_factory.mktemp("gw"))
    pr = run_filter(exe, inputs, out, ("-G", "-W"))
    return out, decoded(out), pr.stderr


def test_bigwigs_are_the_conversion_of_the_runs_own_text(both, inputs, tmp_path):
    out, dec, err = both
    sizes = dict(gv.CHROMS)
    for w in (0, 1):
        text = open(os.path.join(out, GRAPHS[w])).read()
        assert text.count("\n") > 100                                        # (the run has data on several chromosomes; the count itself is not a claim)
        m = bs.model(bs.parse_bedgraph(text), sizes)
        bs.check_against_model(dec[w], m)
        assert len(dec[w]["chroms"]) >= 3 and dec[w]["index"][3] == 1 and all(z[1][3] == 1024 for z in dec[w]["zooms"])
        if bs.have_reference():
            ref = str(tmp_path / f"ref{w}.bw")
            pr = bs.reference_bigwig(str(tmp_path), os.path.join(out, GRAPHS[w]), os.path.join(inputs, "chrom.sizes"), ref)
            assert pr.returncode == 0, pr.stderr
            assert bs.decode(open(ref, "rb").read()) == dec[w]
    assert re.search(r"\[itx timing\] genome coverage bigWigs: \d+ \+ \d+ items", err)


def test_w_alone_writes_the_same_bigwigs_and_no_text(both, inputs, exe, tmp_path):
    pr = run_filter(exe, inputs, str(tmp_path / "w"), ("-W",))
    run_filter(exe, inputs, str(tmp_path / "plain"), ())
    assert sorted(os.listdir(tmp_path / "w")) == sorted(os.listdir(tmp_path / "plain") + BIGWIGS)
    assert decoded(tmp_path / "w") == both[1]
    m = re.search(r"(\d+) \+ (\d+) lines, (\d+) \+ (\d+) bytes in (\d+) \+ (\d+) rounds", pr.stderr)
    assert m and set(m.groups()) == {"0"}                                   # no text round ran


def test_host_build_gives_the_same_content(both, inputs, exe, tmp_path):
    run_filter(exe, inputs, str(tmp_path / "h"), ("-W",), env={"ITX_BW_HOST": "1"})
    assert decoded(tmp_path / "h") == both[1]
    if bs.have_reference():                                                 # host zlib: the reference's bytes
        for w in (0, 1):
            ref = str(tmp_path / f"ref{w}.bw")
            assert bs.reference_bigwig(str(tmp_path), os.path.join(both[0], GRAPHS[w]), os.path.join(inputs, "chrom.sizes"), ref).returncode == 0
            assert filecmp.cmp(ref, tmp_path / "h" / BIGWIGS[w], shallow=False)


def test_g_alone_writes_what_it_wrote_and_no_bigwig(both, inputs, exe, tmp_path):
    run_filter(exe, inputs, str(tmp_path / "g"), ("-G",))
    run_filter(exe, inputs, str(tmp_path / "plain"), ())
    assert sorted(os.listdir(tmp_path / "g")) == sorted(os.listdir(tmp_path / "plain") + GRAPHS)
    for fn in GRAPHS:
        assert filecmp.cmp(tmp_path / "g" / fn, os.path.join(both[0], fn), shallow=False)


def test_no_counted_reads_no_bigwig(inputs, exe, tmp_path):
    with open(os.path.join(inputs, "none.sam"), "w") as f:
        f.write("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{s}\n" for n, s in gv.CHROMS) + "q1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n")
    out = tmp_path / "n"
    os.makedirs(out)
    (out / BIGWIGS[0]).write_bytes(b"left by an earlier run")
    pr = run_filter(exe, inputs, str(out), ("-W", "-S"), "none.sam")
    assert not any(os.path.exists(out / fn) for fn in BIGWIGS + GRAPHS)
    for fn in BIGWIGS:
        assert pr.stderr.count(f"* {fn} is not written: the coverage has no data\n") == 1


@pytest.mark.parametrize("opts,aln", [(("-W", "-S"), "reads.sam"), (("-W", "-b", "-s"), "reads.bam")], ids=["S", "bs"])
def test_with_sam_input_and_with_the_sorted_bam(opts, aln, both, inputs, exe, tmp_path):
    run_filter(exe, inputs, str(tmp_path / "w"), opts, aln)
    assert decoded(tmp_path / "w") == both[1]


def test_usage_names_the_option(exe):
    pr = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True)
    assert re.search(r"^\s+-W\s+output that genome coverage as bigWig", pr.stderr, re.M)
