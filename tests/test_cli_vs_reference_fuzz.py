"""Differential test on the GPU box: the drop-in `iteres` (iteres_amd/host + the HIP engine) against the reference
binary itself (oracle/_ref/iteres, built from /root/reference by oracle/Makefile; it travels to the GPU box as a built
file) on seeded random tables, reads and OPTION SETS — every file either program writes must be byte-identical
(bigWig: same decoded content, tests/refio.py). The committed golden cases pin chosen corners; this sweeps the
combinations nobody chose. Skipped where the reference binary is absent."""
import os
import subprocess

import numpy as np
import pytest

import refio
from iteres_amd import build, engine as eng, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/iteres not built (make -C oracle ref)")
    lib, exe = build.build_all()
    assert exe and os.path.exists(exe)
    return exe


def _xa_aux(rng, r, t, chroms, frac):
    names = [nm for nm, _ in chroms]
    aux = [[] for _ in range(len(r))]
    for i in np.flatnonzero(rng.random(len(r)) < frac):
        alts = []
        for _ in range(int(rng.integers(1, 4))):
            if rng.random() < 0.7:
                row = int(rng.integers(0, len(t.start)))
                c, p0 = names[int(t.chrom[row])], int(t.start[row]) + int(rng.integers(-20, 40))
            else:
                ci = int(rng.integers(0, len(chroms)))
                c, p0 = names[ci], int(rng.integers(1, chroms[ci][1]))
            alts.append(f"{c},{'+' if rng.random() < 0.5 else '-'}{max(p0, 1)},{int(r.l_qseq[i])}M,{int(rng.integers(0, 4))}")
        fields = [f"XA:Z:{';'.join(alts)};"]
        if rng.random() < 0.9:
            fields.insert(0, f"NM:i:{int(rng.integers(0, 4))}")
        aux[i] = fields
    return aux


def _random_case(seed):
    rng = np.random.default_rng(seed)
    chroms = [("chr1", int(rng.integers(300_000, 3_000_000))), ("chr2", int(rng.integers(150_000, 900_000))), ("chrM", 16_571)][: int(rng.integers(1, 4))]
    t = synth.make_table(seed * 3 + 1, chroms, int(rng.integers(300, 6000)), n_names=int(rng.integers(5, 300)), n_fams=int(rng.integers(2, 30)),
                         n_clas=int(rng.integers(1, 9)), overlap_frac=float(rng.choice([0.0, 0.03, 0.3])), shuffle_frac=float(rng.choice([0.0, 0.05, 1.0])),
                         inconsistent_frac=float(rng.choice([0.0, 0.05])), median_len=float(rng.choice([60.0, 200.0, 900.0])))
    header = list(chroms) + ([("chrUn", 40_000)] if rng.random() < 0.5 else [])
    r = synth.make_reads(seed * 3 + 2, header, int(rng.integers(200, 30_000)), read_len=(20, int(rng.integers(40, 260))),
                         paired_frac=float(rng.choice([0.0, 0.3, 1.0])), unmapped_frac=float(rng.choice([0.0, 0.05])),
                         odd_cigar_frac=float(rng.choice([0.0, 0.2])), sorted_=bool(rng.random() < 0.7))
    if rng.random() < 0.5:
        r.aux = _xa_aux(rng, r, t, chroms, float(rng.choice([0.02, 0.4])))
    if rng.random() < 0.5:                       # exact duplicates for -R
        for i in rng.choice(np.arange(1, len(r)), max(len(r) // 8, 1), replace=False):
            for arr in (r.tid, r.pos, r.flag, r.l_qseq, r.mtid, r.mpos, r.isize):
                arr[i] = arr[i - 1]
            r.cigars[i] = list(r.cigars[i - 1])
    r.mapq[:4] = 60                              # -R reads its key buffer before writing it otherwise (uninitialised in the reference)
    r.flag[:4] &= ~np.uint16(4)
    return rng, chroms, t, r


def _random_opts(rng, t):
    pick = lambda *a: a[int(rng.integers(0, len(a)))]
    common = []
    if rng.random() < 0.5:
        common += ["-Q", str(pick(0, 1, 20, 37, 61))]
    if rng.random() < 0.3:
        common += ["-R"]
    if rng.random() < 0.3:
        common += ["-T"]
    if rng.random() < 0.3:
        common += ["-D"]
    if rng.random() < 0.5:
        common += ["-E", str(pick(0, 1, 50, 150, 400))]
    if rng.random() < 0.4:
        common += ["-I", str(pick(100, 350, 1000))]
    if rng.random() < 0.5:
        common += ["-N", str(pick(0, 2, 3))]
    runs = []
    st = list(common) + ["-w"]
    if rng.random() < 0.4:
        st += ["-c", pick("0.3", "0.5", "0.9", "1", "0.0001", "0")]
    if rng.random() < 0.3:
        st += ["-x"]
    if rng.random() < 0.4:
        st += ["-U", str(pick(0, 1, 2))]
    if rng.random() < 0.3:
        st += ["-B"]
    if rng.random() < 0.3:
        st += ["-V"]
    runs.append(("stat", st))
    fl = list(common)
    if rng.random() < 0.4:
        fl += ["-g", pick("0.3", "0.5", "0.9", "1")]
    used = np.bincount(t.rep_name, minlength=len(t.names))
    kind = pick("-n", "-c", "-f")
    if kind == "-n":
        fl += ["-n", t.names[int(np.argmax(used))] if rng.random() < 0.7 else t.names[int(rng.integers(0, len(t.names)))]]
    elif kind == "-c":
        fl += ["-c", t.clas[int(t.cla_of_row[int(rng.integers(0, len(t.start)))])]]
    else:
        fl += ["-f", t.fams[int(t.fam_of_row[int(rng.integers(0, len(t.start)))])]]
    if rng.random() < 0.5:
        fl += ["-t", str(pick(1, 2, 5))]
    if rng.random() < 0.5:
        fl += ["-r"]
    runs.append(("filter", fl))
    return runs


# ITX_FUZZ_EXTRA=<n>: n more seeds behind the committed 48 (a longer hunt on a GPU box)
@pytest.mark.parametrize("seed", list(range(7100, 7148 + int(os.environ.get("ITX_FUZZ_EXTRA", "0")))))
def test_random_case_matches_reference_binary(seed, exe, tmp_path):
    rng, chroms, t, r = _random_case(seed)
    inp = tmp_path / "in"
    inp.mkdir()
    synth.write_sizes(str(inp / "chrom.sizes"), chroms)
    synth.write_sizes(str(inp / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(inp / "rmsk.txt"), t)
    as_sam = bool(rng.random() < 0.3)
    aln = str(inp / ("reads.sam" if as_sam else "reads.bam"))
    if as_sam:
        synth.write_sam(aln, r, with_seq=True)
    else:
        synth.write_bam(aln, r, with_seq=bool(rng.random() < 0.7), block=int(rng.choice([0xff00, 3000])))
    for cmd, opts in _random_opts(rng, t):
        if as_sam:
            opts = opts + ["-S"]
        outs = {}
        for who, prog in (("ref", REF), ("new", exe)):
            work = tmp_path / f"{cmd}_{who}"
            work.mkdir()
            pr = subprocess.run([prog, cmd] + opts + ["-o", "out", str(inp / "chrom.sizes"), str(inp / "rep.sizes"), str(inp / "rmsk.txt"), aln],
                                cwd=work, capture_output=True, text=True, timeout=600)
            outs[who] = (pr.returncode, work, pr.stderr)
        (rc_r, w_r, err_r), (rc_n, w_n, err_n) = outs["ref"], outs["new"]
        tag = f"seed {seed}: {cmd} {' '.join(opts)}"
        assert rc_r in (0, 255) or rc_r > 0, f"{tag}: the reference itself died ({rc_r}): {err_r[-500:]}"
        assert rc_n == rc_r, f"{tag}: exit {rc_n} vs reference {rc_r}\n{err_n[-1500:]}"
        files_r, files_n = sorted(os.listdir(w_r)), sorted(os.listdir(w_n))
        assert files_n == files_r, tag
        for fn in files_r:
            a, b = (w_r / fn).read_bytes(), (w_n / fn).read_bytes()
            if fn.endswith(".bigWig"):
                assert refio.bigwig_digest(b) == refio.bigwig_digest(a), f"{tag}: {fn} decodes differently"
            else:
                assert a == b, f"{tag}: {fn} differs"


def test_file_list_matches_reference_binary(exe, tmp_path):
    """stat takes a comma-separated list of alignment files (generic.c:725): one engine, one set of counters, a fresh
    header (and tid map) per file — and a decoder whose windows must not leak from one file into the next."""
    chroms = [("chr1", 2_000_000), ("chr2", 700_000)]
    t = synth.make_table(9001, chroms, 3000, n_names=80, n_fams=12, n_clas=5)
    inp = tmp_path / "in"
    inp.mkdir()
    synth.write_sizes(str(inp / "chrom.sizes"), chroms)
    synth.write_sizes(str(inp / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(inp / "rmsk.txt"), t)
    paths = []
    for k, (hdr, n) in enumerate(((chroms, 20_000), (chroms[::-1] + [("chrUn", 5000)], 7_000), (chroms, 1))):
        r = synth.make_reads(9100 + k, hdr, n, read_len=(30, 120), paired_frac=0.2)
        p = str(inp / f"r{k}.bam")
        synth.write_bam(p, r, with_seq=True, block=0xff00 if k != 1 else 5000)
        paths.append(p)
    outs = {}
    for who, prog in (("ref", REF), ("new", exe)):
        work = tmp_path / who
        work.mkdir()
        pr = subprocess.run([prog, "stat", "-w", "-o", "out", str(inp / "chrom.sizes"), str(inp / "rep.sizes"), str(inp / "rmsk.txt"), ",".join(paths)],
                            cwd=work, capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-1500:]
        outs[who] = work
    for fn in sorted(os.listdir(outs["ref"])):
        a, b = (outs["ref"] / fn).read_bytes(), (outs["new"] / fn).read_bytes()
        if fn.endswith(".bigWig"):
            assert refio.bigwig_digest(b) == refio.bigwig_digest(a), fn
        else:
            assert a == b, fn


def test_pileup_matches_reference_binary(exe, tmp_path):
    """The rounding regime of the bigWig zoom summaries through the whole command: the pile-up input of tests/bwcases.py
    (400 000 reads on two consensus sequences: sum_squares passes 2^24 inside level-0 summaries, sum_data at the top),
    the bigWig blocks built on the device (the default) and by the host writer (ITX_BW_HOST=1), against the reference
    binary: text files byte for byte, bigWigs by decoded content."""
    import bwcases
    inp = tmp_path / "in"
    inp.mkdir()
    paths = bwcases.write_pileup_input(inp)
    outs = {}
    for who, prog, env in (("ref", REF, {}), ("dev", exe, {"ITX_TIMING": "1"}), ("host", exe, {"ITX_TIMING": "1", "ITX_BW_HOST": "1"})):
        work = tmp_path / who
        work.mkdir()
        pr = subprocess.run([prog, "stat"] + bwcases.PILEUP_OPTS + ["-o", "out"] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                            env=dict(os.environ, **env))
        assert pr.returncode == 0, (who, pr.stderr[-1500:])
        assert ("bigWig: device build" in pr.stderr) == (who == "dev"), (who, pr.stderr[-1500:])
        outs[who] = work
    files = sorted(os.listdir(outs["ref"]))
    for fn in ("out.iteres.wig", "out.iteres.unique.wig"):
        vals, order = refio.parse_wig(str(outs["ref"] / fn))
        dec = refio.bigwig_decode((outs["ref"] / fn.replace(".wig", ".bigWig")).read_bytes())
        n_sq, n_sd = bwcases.wig_depth(vals, [nm for nm, _, _ in dec["chroms"]], [z[0] for z in dec["zooms"]])
        assert n_sq >= 1 and n_sd >= 1, (fn, n_sq, n_sd)
    for who in ("dev", "host"):
        assert sorted(os.listdir(outs[who])) == files, who
        for fn in files:
            a, b = (outs["ref"] / fn).read_bytes(), (outs[who] / fn).read_bytes()
            if fn.endswith(".bigWig"):
                assert refio.bigwig_digest(b) == refio.bigwig_digest(a), f"{who}: {fn} decodes differently"
            else:
                assert a == b, f"{who}: {fn} differs"


def test_long_reads_match_reference_binary(exe, tmp_path):
    """Records of tens of kilobytes (long reads): they span BGZF blocks and the decoder's 16 KiB pieces; -E 0 so that the
    CIGAR end decides the interval on both strands."""
    chroms = [("chr1", 30_000_000)]
    t = synth.make_table(9201, chroms, 20_000, n_names=100, n_fams=12, n_clas=5)
    r = synth.make_reads(9202, chroms, 1500, read_len=(5_000, 40_000), odd_cigar_frac=0.4)
    inp = tmp_path / "in"
    inp.mkdir()
    synth.write_sizes(str(inp / "chrom.sizes"), chroms)
    synth.write_sizes(str(inp / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(inp / "rmsk.txt"), t)
    aln = str(inp / "long.bam")
    synth.write_bam(aln, r, with_seq=True)
    for cmd, opts in (("stat", ["-w", "-E", "0"]), ("stat", ["-w"]), ("filter", ["-c", t.clas[0], "-r"])):
        outs = {}
        for who, prog in (("ref", REF), ("new", exe)):
            work = tmp_path / f"{cmd}_{len(opts)}_{who}"
            work.mkdir()
            pr = subprocess.run([prog, cmd] + opts + ["-o", "out", str(inp / "chrom.sizes"), str(inp / "rep.sizes"), str(inp / "rmsk.txt"), aln], cwd=work,
                                capture_output=True, text=True, timeout=600)
            assert pr.returncode == 0, pr.stderr[-1500:]
            outs[who] = work
        for fn in sorted(os.listdir(outs["ref"])):
            a, b = (outs["ref"] / fn).read_bytes(), (outs["new"] / fn).read_bytes()
            if fn.endswith(".bigWig"):
                assert refio.bigwig_digest(b) == refio.bigwig_digest(a), fn
            else:
                assert a == b, (cmd, opts, fn)


@pytest.mark.parametrize("kind", ["header_only", "no_eof_marker", "cut_mid_block", "cut_on_block_boundary"])
def test_odd_files_match_reference_binary(kind, exe, tmp_path):
    """Files that end early or hold no record: the drop-in must stop where the reference stops and write the same files
    (a truncated last block is not inflated by either; the records before it count)."""
    chroms = [("chr1", 2_000_000)]
    t = synth.make_table(9301, chroms, 4000, n_names=60, n_fams=10, n_clas=4)
    r = synth.make_reads(9302, chroms, 0 if kind == "header_only" else 30_000, read_len=(30, 100))
    inp = tmp_path / "in"
    inp.mkdir()
    synth.write_sizes(str(inp / "chrom.sizes"), chroms)
    synth.write_sizes(str(inp / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(inp / "rmsk.txt"), t)
    aln = str(inp / "x.bam")
    synth.write_bam(aln, r, with_seq=True, eof=kind not in ("no_eof_marker",), block=20_000)
    if kind.startswith("cut"):
        data = open(aln, "rb").read()
        blocks = eng.index_bgzf(data)
        k = len(blocks) * 2 // 3
        cut = int(blocks["coff"][k]) + (int(blocks["csize"][k]) // 2 if kind == "cut_mid_block" else 0)
        open(aln, "wb").write(data[:cut])
    outs = {}
    for who, prog in (("ref", REF), ("new", exe)):
        work = tmp_path / who
        work.mkdir()
        pr = subprocess.run([prog, "stat", "-w", "-o", "out", str(inp / "chrom.sizes"), str(inp / "rep.sizes"), str(inp / "rmsk.txt"), aln], cwd=work,
                            capture_output=True, text=True, timeout=600)
        outs[who] = (pr.returncode, work, pr.stderr)
    (rc_r, w_r, err_r), (rc_n, w_n, err_n) = outs["ref"], outs["new"]
    assert rc_r >= 0, f"the reference itself crashed on {kind}: {err_r[-300:]}"
    assert rc_n == rc_r, (kind, rc_n, rc_r, err_n[-800:])
    for fn in sorted(os.listdir(w_r)):
        a, b = (w_r / fn).read_bytes(), (w_n / fn).read_bytes()
        if fn.endswith(".bigWig"):
            assert refio.bigwig_digest(b) == refio.bigwig_digest(a), (kind, fn)
        else:
            assert a == b, (kind, fn)
