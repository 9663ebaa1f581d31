"""GPU: `iteres filter -G`, the command. The two bedGraph files are compared byte for byte with the model of tests/gcovcase.py over
the counted reads the REFERENCE names for the same options (its `filter -r` lists joined with its `stat -B` bed lines; recorded under
tests/golden/gcov/ and held against a fresh run of the reference by tests/test_gcov_model.py); the other outputs with a run
without -G. Every input format and route gives the same two files."""
import filecmp
import os
import re
import subprocess

import pytest

import gcovcase as gv
from iteres_amd import build, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gcov_cli") / "in")
    t, r, big, name, fam = gv.make_inputs(d)
    assert gv.input_digest(d) == gv.recorded_counted("ALL")[1]              # the recordings were made for exactly these inputs
    with open(os.path.join(d, "reads.sam"), "rb") as f:
        with open(os.path.join(d, "reads.sam.gz"), "wb") as g:
            data = f.read()
            g.write(b"".join(synth.bgzf_block(data[k:k + 30000], 6) for k in range(0, len(data), 30000)) + synth.BGZF_EOF)
    return d, big, name, fam


def run_filter(exe, d, out, opts, aln, env=None):
    os.makedirs(out, exist_ok=True)
    pr = subprocess.run([exe, "filter"] + list(opts) + ["-o", "out", os.path.join(d, "chrom.sizes"), os.path.join(d, "rep.sizes"), os.path.join(d, "rmsk.txt"),
                         os.path.join(d, aln)], cwd=out, capture_output=True, text=True, timeout=600,
                        env=dict(os.environ, ITX_TIMING="1", ITX_BGZF_CHUNK="40000", **(env or {})))
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr


def graphs(out, sub="ALL"):
    return tuple(open(os.path.join(out, f"out_{sub}.iteres{u}.bedGraph"), "rb").read() for u in ("", ".unique"))


def timing(err):
    m = re.search(r"\[itx timing\] genome coverage: (\d+) records added \((\d+) with MAPQ >= -Q, (\d+) out of range\), (\d+) batches on the device, (\d+) by the host route; "
                  r"(\d+) \+ (\d+) change points, (\d+) \+ (\d+) lines, (\d+) \+ (\d+) bytes in (\d+) \+ (\d+) rounds", err)
    assert m, err[-1500:]
    return dict(zip(("records", "uniq", "oor", "dev", "host", "p0", "p1", "l0", "l1", "b0", "b1", "r0", "r1"), map(int, m.groups())))


def same_other_outputs(with_g, plain, sub="ALL"):
    """every file of the run without -G is there, byte for byte, and -G adds exactly its two"""
    extra = [f"out_{sub}.iteres.bedGraph", f"out_{sub}.iteres.unique.bedGraph"]
    assert sorted(os.listdir(with_g)) == sorted(os.listdir(plain) + extra)
    for fn in os.listdir(plain):
        assert filecmp.cmp(os.path.join(with_g, fn), os.path.join(plain, fn), shallow=False), fn


@pytest.mark.parametrize("key", list(gv.OPTSETS))
def test_command_against_the_reference(key, case, exe, tmp_path):
    d, big, name, fam = case
    aln, opts = gv.OPTSETS[key]
    opts = gv.fill(opts, big, name, fam)
    sub = gv.subfam(opts)
    pr = run_filter(exe, d, str(tmp_path / "g"), ("-G",) + opts, aln)
    run_filter(exe, d, str(tmp_path / "plain"), opts, aln)
    same_other_outputs(tmp_path / "g", tmp_path / "plain", sub)
    counted, _ = gv.recorded_counted(key)
    want = gv.both(counted)
    got = graphs(tmp_path / "g", sub)
    assert got[0] == want[0] and got[1] == want[1]
    tm = timing(pr.stderr)
    assert tm["records"] == len(counted) and tm["uniq"] == sum(c[3] >= gv.MAPQ_MIN for c in counted) and tm["oor"] == 0
    assert (tm["l0"], tm["l1"]) == (want[0].count(b"\n"), want[1].count(b"\n")) and (tm["b0"], tm["b1"]) == (len(want[0]), len(want[1]))
    assert len({l.split(b"\t")[0] for l in got[0].splitlines()}) >= (3 if sub == "ALL" else 1)
    # (chrU, which the size file lacks, sends its windows down the host route: both routes add into one file)
    assert (tm["dev"] >= 1 or aln.endswith(".sam")) and tm["host"] >= 1 and pr.stderr.count("will be discarded") == 1


@pytest.fixture(scope="module")
def bam_run(case, exe, tmp_path_factory):
    d = case[0]
    out = str(tmp_path_factory.mktemp("gcov_bam"))
    pr = run_filter(exe, d, out, ("-G",), "reads.bam")
    return out, graphs(out), timing(pr.stderr)


@pytest.mark.parametrize("which", ["sam_host", "sam_device", "samgz_device", "samgz_host", "bam_host_inflate"])
def test_every_input_format_gives_the_same_files(which, case, exe, bam_run, tmp_path):
    d = case[0]
    aln, opts, env = {"sam_host": ("reads.sam", ("-S",), {}), "sam_device": ("reads.sam", ("-S",), {"ITX_HOST_SAM": "0"}),
                      "samgz_device": ("reads.sam.gz", ("-S",), {"ITX_HOST_SAM": "0"}), "samgz_host": ("reads.sam.gz", ("-S",), {}),
                      "bam_host_inflate": ("reads.bam", (), {"ITX_HOST_INFLATE": "1"})}[which]
    pr = run_filter(exe, d, str(tmp_path / "g"), ("-G",) + opts, aln, env)
    run_filter(exe, d, str(tmp_path / "plain"), opts, aln, env)
    same_other_outputs(tmp_path / "g", tmp_path / "plain")
    assert graphs(tmp_path / "g") == bam_run[1] == gv.both(gv.recorded_counted("ALL")[0])
    tm = timing(pr.stderr)
    assert tm["dev"] == 0 and tm["host"] >= 1 and tm["records"] == bam_run[2]["records"]


def test_windows_of_both_routes_in_one_file(case, bam_run):
    """reads.bam holds mapped records on chrU, which the size file lacks, in the middle of the sorted file: their windows take the
    host route (the warning is per record), the windows before and after stay on the device, and all of them add into one coverage"""
    tm = bam_run[2]
    assert tm["dev"] >= 2 and tm["host"] >= 1 and tm["records"] == len(gv.recorded_counted("ALL")[0])


@pytest.mark.parametrize("extra", [("-r",), ("-b", "-s", "-i", "-a"), ("-r", "-b")], ids=["r", "bsia", "rb"])
def test_with_the_read_lists_and_the_bam(extra, case, exe, bam_run, tmp_path):
    d = case[0]
    env = {"ITX_HOST_NAMES": "0"}                                           # the lists are gathered on the device: one classification for all takers
    run_filter(exe, d, str(tmp_path / "g"), ("-G",) + extra, "reads.bam", env)
    run_filter(exe, d, str(tmp_path / "plain"), extra, "reads.bam", env)
    same_other_outputs(tmp_path / "g", tmp_path / "plain")
    assert graphs(tmp_path / "g") == bam_run[1]
    if extra == ("-r",):                                                    # ... and on the host
        run_filter(exe, d, str(tmp_path / "gh"), ("-G",) + extra, "reads.bam")
        assert graphs(tmp_path / "gh") == bam_run[1]
        same_other_outputs(tmp_path / "gh", tmp_path / "plain")
    if extra == ("-r", "-b"):
        # the lists own the batch's rows and the BAM reads them: the BAM is the one -b alone writes from rows of its own, and the lists'
        # files are the ones -r alone writes
        run_filter(exe, d, str(tmp_path / "r"), ("-r",), "reads.bam", env)
        run_filter(exe, d, str(tmp_path / "b"), ("-b",), "reads.bam", env)
        bams = [fn for fn in os.listdir(tmp_path / "b") if fn.endswith(".bam")]
        assert len(bams) == 1 and os.path.getsize(tmp_path / "b" / bams[0]) > 28
        assert filecmp.cmp(tmp_path / "plain" / bams[0], tmp_path / "b" / bams[0], shallow=False)
        assert os.listdir(tmp_path / "r") and set(os.listdir(tmp_path / "r")) <= set(os.listdir(tmp_path / "plain"))
        for fn in os.listdir(tmp_path / "r"):
            assert filecmp.cmp(tmp_path / "plain" / fn, tmp_path / "r" / fn, shallow=False), fn


def test_threshold_does_not_change_the_coverage(case, exe, bam_run, tmp_path):
    d = case[0]
    run_filter(exe, d, str(tmp_path / "t5"), ("-G", "-t", "5"), "reads.bam")
    run_filter(exe, d, str(tmp_path / "t5_plain"), ("-t", "5"), "reads.bam")
    same_other_outputs(tmp_path / "t5", tmp_path / "t5_plain")
    assert graphs(tmp_path / "t5") == bam_run[1]
    assert not filecmp.cmp(tmp_path / "t5" / "out_ALL.iteres.loci", os.path.join(bam_run[0], "out_ALL.iteres.loci"), shallow=False)


def test_many_rounds_write_the_same_files(case, exe, bam_run, tmp_path):
    d = case[0]
    pr = run_filter(exe, d, str(tmp_path / "g"), ("-G",), "reads.bam", {"ITX_GCOV_ROUND_BYTES": "4000"})
    assert graphs(tmp_path / "g") == bam_run[1]
    tm = timing(pr.stderr)
    assert tm["r0"] >= 10 and tm["r1"] >= 5 and bam_run[2]["r0"] == 1


def test_no_counted_reads_gives_two_empty_files(case, exe, tmp_path):
    d = case[0]
    with open(os.path.join(d, "none.sam"), "w") as f:
        f.write("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{s}\n" for n, s in gv.CHROMS) + "q1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n")
    run_filter(exe, d, str(tmp_path / "g"), ("-G", "-S"), "none.sam")
    assert graphs(tmp_path / "g") == (b"", b"")


def test_usage_names_the_option(exe):
    pr = subprocess.run([exe, "filter", "-h"], capture_output=True, text=True)
    assert re.search(r"^\s+-G\s+output the genome coverage", pr.stderr, re.M)
