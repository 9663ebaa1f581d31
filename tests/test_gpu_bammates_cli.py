"""GPU: the command `iteres filter -c <class> -b -s -m` on files of tools/mkbam with paired=1, about 20 000 records: sorted, shuffled,
and with a chromosome the size file lacks in the middle (its windows take the host route).
The expectation is tests/matecase.py over the input's records and the rows oracle/liboracle.so chooses. Every test first asserts that
this expectation holds at least 100 counted pairs with both signs of isize and mates on either side of their READ1, then compares the
emitted records with it, .loci and .reportloci with a run without -m, and runs the variants with -i, -a, -r, -R, -D and -l.
Where oracle/_ref is present the reference reads the emitted file: its counts do not move, every pair is complete in bamcheck view, and
bamcheck index agrees with the written .bai."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import baicase as bai
import bgzfmemberhost as bm
import matecase as mc
import refbam
import reptagcase as rt
from iteres_amd import synth
from test_gpu_bamout import BAM_HEADER, CHROMS, REF, exe, loci_total, oracle_rows, pile, raw_records, routes, run_filter   # noqa: F401  (fixtures too)
from test_gpu_bamsort import header_parts, key_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_READS = 20_000
BAM = "out_%s.iteres.bam"


@pytest.fixture(scope="module")
def inputs(pile, tmp_path_factory):
    """<pile>/mates_sorted.bam, mates_shuffled.bam (the header of the size file) and mates_mixed.bam (chrU in the middle)"""
    root, d, big, name = pile
    w = tmp_path_factory.mktemp("mkbam_mates")
    mk = str(w / "mkbam")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-Wall", "-o", mk, os.path.join(ROOT, "tools", "mkbam.c"), "-lz", "-ldl"])
    synth.write_sizes(str(w / "with_u.sizes"), BAM_HEADER)
    for fn, sizes, extra in (("mates_sorted.bam", d / "chrom.sizes", ()), ("mates_shuffled.bam", d / "chrom.sizes", ("order=shuffled",)),
                             ("mates_mixed.bam", w / "with_u.sizes", ())):
        subprocess.check_call([mk, str(sizes), str(N_READS), str(d / fn), "100", "7", "0", "paired=1"] + list(extra), env=dict(os.environ, OMP_NUM_THREADS="4"),
                              stderr=subprocess.DEVNULL)
    return root, d, big


def mates_line(err):
    m = re.search(r"; sort: [^;]*; mates: (\d+) candidates held \((\d+) bytes\), (\d+) wanted, (\d+) found, [0-9.]+ ms in the candidate gathers, [0-9.]+ ms in the join", err)
    assert m, err[-1500:]
    return dict(zip(("candidates", "bytes", "wanted", "found"), map(int, m.groups())))


def expectation(root, d, aln, sel, big):
    """(the expected records, the counted records, wanted, found) and the assertion that the case shows something"""
    hit_row, _ = oracle_rows(root, aln, ("-c", big) + tuple(sel))
    head, recs = raw_records(d / aln)
    counted = [r for r, h in zip(recs, hit_row) if h >= 0]
    want, n_wanted, n_found = mc.expected(counted, recs)
    chosen = mc.choose(counted, recs)[0]
    at = {bytes(r): i for i, r in enumerate(recs)}
    assert len(at) == len(recs)
    before = sum(at[bytes(c)] < at[bytes(counted[i])] for c, i in chosen)
    signs = {mc.fields(counted[i])["tlen"] > 0 for c, i in chosen}
    assert len(chosen) >= 100 and signs == {True, False} and before >= 1 and len(chosen) - before >= 1, (len(chosen), signs, before)
    return want, counted, n_wanted, n_found


def run_pair(exe, d, tmp_path, aln, big, opts, env=None):
    """-c big -b -s -m with opts, and the same without -m; every file but the BAM (and its index) is the same"""
    env = dict({"ITX_HOST_NAMES": "0"}, **(env or {}))
    with_m = run_filter(exe, d, str(tmp_path / "m"), ("-c", big, "-b", "-s", "-m") + tuple(opts), d / aln, env)
    run_filter(exe, d, str(tmp_path / "s"), ("-c", big, "-b", "-s") + tuple(opts), d / aln, env)
    assert sorted(os.listdir(tmp_path / "m")) == sorted(os.listdir(tmp_path / "s"))
    for fn in os.listdir(tmp_path / "s"):
        if not fn.endswith((".bam", ".bai")):
            assert filecmp.cmp(tmp_path / "m" / fn, tmp_path / "s" / fn, shallow=False), fn
    assert {f"out_{big}.iteres.loci", f"out_{big}.iteres.reportloci"} <= set(os.listdir(tmp_path / "m"))
    return with_m


def check_file(tmp_path, big, want, with_index):
    path = tmp_path / "m" / (BAM % big)
    data = open(path, "rb").read()
    assert data.endswith(bm.EOF_MARKER)
    head, got = raw_records(path)
    assert got == want
    assert b"SO:coordinate" in header_parts(head)[0].split(b"\n")[0]
    if with_index:
        status, idx = bai.expected_for_file(data)
        assert status == bai.OK and open(str(path) + ".bai", "rb").read() == idx
    return path, data


def check_reference(exe, d, tmp_path, aln, big, path, with_index):
    if not os.path.exists(REF) or not refbam.present:
        return
    run_filter(exe, d, str(tmp_path / "ref_in"), ("-c", big), d / aln, binary=REF)
    run_filter(exe, d, str(tmp_path / "ref_out"), ("-c", big), path, binary=REF)
    assert loci_total(tmp_path / "ref_in" / f"out_{big}.iteres.loci")[1] == loci_total(tmp_path / "ref_out" / f"out_{big}.iteres.loci")[1]
    head, lines = refbam.view(path)
    by_name = {}
    for ln in lines:
        f = ln.split(b"\t")
        by_name.setdefault(f[0], []).append((int(f[1]), int(f[3]), int(f[7])))
    n_pairs = 0
    for name, rs in by_name.items():
        for flag, pos, mpos in rs:
            if flag & 0x1 and not flag & 0x8:
                partners = [r for r in rs if (r[0] & 0xc0) == (flag & 0xc0) ^ 0xc0 and r[1] == mpos]
                assert len(partners) == 1, (name, rs)
                n_pairs += 1
    assert n_pairs >= 200
    if with_index:
        ours = open(str(path) + ".bai", "rb").read()
        refbam.check_index(path, ours)
        with open(str(path) + ".bai", "wb") as f:                          # (the library wrote its own beside the file)
            f.write(ours)


@pytest.mark.parametrize("aln", ["mates_sorted.bam", "mates_shuffled.bam"])
def test_command(aln, inputs, exe, tmp_path):
    root, d, big = inputs
    want, counted, n_wanted, n_found = expectation(root, d, aln, (), big)
    with_m = run_pair(exe, d, tmp_path, aln, big, ("-i",))
    path, data = check_file(tmp_path, big, want, True)
    ml = mates_line(with_m.stderr)
    assert (ml["wanted"], ml["found"]) == (n_wanted, n_found) and n_wanted == n_found and "have no mate in the input" not in with_m.stderr
    head, recs = raw_records(d / aln)
    assert ml["candidates"] == sum(mc.candidate(r) for r in recs) and routes(with_m.stderr)["records"] == len(counted)
    assert routes(with_m.stderr)["dev"] >= 3 and routes(with_m.stderr)["host"] == 0
    check_reference(exe, d, tmp_path, aln, big, path, True)


def test_command_host_route_in_the_middle(inputs, exe, tmp_path):
    root, d, big = inputs
    aln = "mates_mixed.bam"
    want, counted, n_wanted, n_found = expectation(root, d, aln, (), big)
    with_m = run_pair(exe, d, tmp_path, aln, big, ("-i",))
    path, data = check_file(tmp_path, big, want, True)
    rt_ = routes(with_m.stderr)
    assert rt_["dev"] >= 2 and rt_["host"] >= 1, rt_
    head, recs = raw_records(d / aln)
    assert mates_line(with_m.stderr)["candidates"] == sum(mc.candidate(r) for r in recs)      # the host route's windows feed the store too
    u = [i for i, r in enumerate(recs) if key_of(r)[0] == 1]
    assert sum(mc.candidate(r) for r in recs[u[0]:u[-1] + 1]) > 100


@pytest.mark.parametrize("which", ["R", "D", "r", "l0", "l1"])
def test_command_options(which, inputs, exe, tmp_path):
    root, d, big = inputs
    aln = "mates_mixed.bam" if which in ("R", "r") else "mates_sorted.bam"
    opts = {"R": ("-R",), "D": ("-D",), "r": ("-r",), "l0": ("-l", "0"), "l1": ("-l", "1")}[which]
    sel = tuple(o for o in opts if o in ("-R", "-D"))
    want, counted, n_wanted, n_found = expectation(root, d, aln, sel, big)
    with_m = run_pair(exe, d, tmp_path, aln, big, opts)
    check_file(tmp_path, big, want, False)
    assert mates_line(with_m.stderr)["found"] == n_found
    if which in ("l0", "l1"):
        assert with_m.stderr.rstrip().splitlines()[-1] != "" and ", level %s" % opts[1] in with_m.stderr


@pytest.mark.parametrize("aln", ["mates_sorted.bam", "mates_mixed.bam"])
def test_command_annotated(aln, inputs, exe, tmp_path):
    """-a: with the tags taken off the file is the one without -a, and a mate carries the tags of its READ1"""
    root, d, big = inputs
    want, counted, n_wanted, n_found = expectation(root, d, aln, (), big)
    run_pair(exe, d, tmp_path, aln, big, ("-a", "-i"))
    path = tmp_path / "m" / (BAM % big)
    head, got = raw_records(path)
    stripped = [rt.strip(r) for r in got]
    assert [s[0] for s in stripped] == want
    status, idx = bai.expected_for_file(open(path, "rb").read())
    assert status == bai.OK and open(str(path) + ".bai", "rb").read() == idx
    tags_of = {}
    for c, i in mc.choose(counted, raw_records(d / aln)[1])[0]:
        tags_of[bytes(c)] = bytes(counted[i])
    by_rec = {bytes(s[0]): s[1] for s in stripped}
    assert len(tags_of) >= 100
    for mate, read1 in tags_of.items():
        assert by_rec[mate] == by_rec[read1]
    assert len({v for v in by_rec.values()}) > 10                          # many rows


def test_pairs_without_a_mate_are_reported(inputs, exe, tmp_path):
    """every fifth READ2 taken out of the input: the READ1s are still written, one line gives the count, the exit status is 0"""
    root, d, big = inputs
    head, recs = raw_records(d / "mates_sorted.bam")
    k = 0
    kept = []
    for r in recs:
        if mc.candidate(r):
            k += 1
            if k % 5 == 0:
                continue
        kept.append(r)
    buf = head + b"".join(kept)
    with open(d / "mates_fewer.bam", "wb") as f:
        f.write(b"".join(synth.bgzf_block(buf[i:i + 6000]) for i in range(0, len(buf), 6000)) + synth.BGZF_EOF)
    want, counted, n_wanted, n_found = expectation(root, d, "mates_fewer.bam", (), big)
    assert n_wanted - n_found >= 20
    with_m = run_pair(exe, d, tmp_path, "mates_fewer.bam", big, ())
    check_file(tmp_path, big, want, False)
    assert with_m.stderr.count("[iteres] %d counted pairs have no mate in the input\n" % (n_wanted - n_found)) == 1
    ml = mates_line(with_m.stderr)
    assert (ml["wanted"], ml["found"]) == (n_wanted, n_found)
    assert np.all([r in want for r in counted[:50]])
