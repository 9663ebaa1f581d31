"""GPU: the .loci file of `filter` / `cpgfilter` sorted and formatted on the device (include/iteres_amd.h itx_loci_*,
csrc/itx_loci.hip; the line rule csrc/itx_lociline.h has its own CPU test, tests/test_lociline.py).
1. the ABI, directly: tables of 0 .. 70 000 rows over 1, 3 and 300 chromosomes, many rows in one bin and rows on every bin level; the
   sorted order against (chromosome rank, bin, -row) sorted by Python with goldencase.bin_of and refio.kent_hash_order, the text
   against Python's own `%` line by line, for every threshold and read number, with the canary behind the text;
2. names of 200 - 255 bytes (a tile's text passes several 32 KiB windows); 3. lines the host has to look at; 4. the CpG kind;
5. argument checks; 6. the command: every filter / cpgfilter run of the goldens by both routes against the reference's files, and
   the timing line's route; 7. a BAM whose reads all lie below -Q, so that the read number is 0."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bedcase as bc
import goldencase as gc
import refio
from iteres_amd import build, engine as eng, synth
from test_lociline import CPG, FILTER, py_line

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
CANARY = 0xA5
COUNTS = [0, 1, 9, 10, 99_999, 2 ** 31 - 1]
READS = [1, 360_000_000, 2 ** 40]


def _table(names):
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    return np.frombuffer(b"".join(names) + b"\0", np.uint8).copy(), off


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Loci:
    def __init__(self, kind, t):
        self.t, self._h = t, C.c_void_p()
        self.keep = [_table(t[k]) for k in ("chroms", "reps", "clas", "fams")]
        (cb, co), (rb, ro), (kb, ko), (fb, fo) = self.keep
        eng._chk(eng.load().itx_loci_create(0, kind, _p(t["rows"]), _p(t["row_chrom"]), len(t["rows"]), _p(t["rank"]), len(t["chroms"]), _p(cb), _p(co), _p(rb), _p(ro),
                                            len(t["reps"]), _p(kb), _p(ko), len(t["clas"]), _p(fb), _p(fo), len(t["fams"]), C.byref(self._h)), "itx_loci_create")

    def order(self):
        out = np.zeros(max(len(self.t["rows"]), 1), np.uint32)
        ms = C.c_double(-1)
        eng._chk(eng.load().itx_loci_order(self._h, _p(out), C.byref(ms)), "itx_loci_order")
        assert ms.value >= 0
        return out[:len(self.t["rows"])].tolist()

    def _text(self, rc, res):
        eng._chk(rc, "itx_loci text")
        if res.hard:
            assert not res.text and res.bytes == 0
            return None, int(res.lines), int(res.hard)
        assert res.capacity >= res.bytes + 16 and res.text
        raw = C.string_at(res.text, res.capacity)
        assert raw[res.bytes:] == bytes([CANARY]) * (res.capacity - res.bytes), "the device wrote behind the text"
        return raw[:res.bytes], int(res.lines), 0

    def filter_text(self, cnt, threshold, reads_num):
        res = eng.LociText()
        cnt = np.ascontiguousarray(cnt, np.uint32)
        return self._text(eng.load().itx_loci_filter_text(self._h, _p(cnt), threshold, reads_num, C.byref(res)), res)

    def cpg_text(self, cnt, total, threshold):
        res = eng.LociText()
        cnt, total = np.ascontiguousarray(cnt, np.int32), np.ascontiguousarray(total, np.float64)
        return self._text(eng.load().itx_loci_cpg_text(self._h, _p(cnt), _p(total), threshold, C.byref(res)), res)

    def close(self):
        eng.load().itx_loci_destroy(self._h)
        self._h = None


def make_table(n, n_chrom, long_names=False, seed=0):
    """rows in 'file order' with the properties the order and the text depend on"""
    rng = np.random.default_rng(100 * n + n_chrom + seed)
    chroms = [b"chr%d" % (i + 1) for i in range(n_chrom)]
    if n_chrom >= 3:
        chroms[1], chroms[2] = b"chrX_KI270881v1_alt", b"M"
    reps = [b"Rep%d" % i for i in range(40)] + [b"(CATTC)n", b"L1PA2"]
    clas = [b"LINE", b"SINE", b"Simple_repeat", b"DNA?"]
    fams = [b"Fam%d" % i for i in range(9)] + [b"hAT-Charlie"]
    if long_names:
        reps = [b"r%03d" % i + b"n" * (196 + i % 56) for i in range(60)]
        clas += [b"c" * 255]
        fams += [b"f" * 255]
    rows = np.zeros(n, eng.ROW_DTYPE)
    start = np.zeros(n, np.int64)
    end = np.zeros(n, np.int64)
    for i in range(n):
        how = i % 8
        if how < 4:                                                       # many rows of one bin: the descending-row rule
            s = 1000 + int(rng.integers(0, 100_000))
            e = s + int(rng.integers(1, 500))
        elif how < 6:                                                     # anywhere, short
            s = int(rng.integers(0, 400_000_000))
            e = s + int(rng.integers(1, 3000))
        else:                                                             # lengths 1 .. 2^29: every bin level
            ln = 1 << int(rng.integers(0, 30))
            s = int(rng.integers(0, max(1, 2 ** 29 + 2 ** 20 - ln))) if ln >= 1 << 26 else int(rng.integers(0, 400_000_000))
            e = s + ln
        start[i], end[i] = s, e
    if n > 20:
        start[7], end[7] = 2 ** 29 - 5, 2 ** 29 + 5                       # across 512 M: bin 0
        start[9], end[9] = 12345, 12345 + 1                               # 1 to 10 digits
        start[11], end[11] = 1, 2 ** 31 - 1
    rows["start"], rows["end"] = start, end
    rows["chrom"] = -7                                                    # not read
    rows["rep"] = rng.integers(0, len(reps), n)
    rows["cla"] = rng.integers(0, len(clas), n)
    rows["fam"] = rng.integers(0, len(fams), n)
    row_chrom = rng.integers(0, n_chrom, n).astype(np.uint32)
    kent = refio.kent_hash_order([c.decode() for c in chroms])
    rank = np.array([kent.index(c.decode()) for c in chroms], np.uint32)
    if n_chrom == 300:
        assert rank.tolist() != list(range(300))
    return dict(rows=rows, row_chrom=row_chrom, rank=rank, chroms=chroms, reps=reps, clas=clas, fams=fams)


def want_order(t):
    r = t["rows"]
    bins = [gc.bin_of(int(s), int(e)) for s, e in zip(r["start"], r["end"])]
    assert all(0 <= b < 8192 for b in bins)
    rk = t["rank"][t["row_chrom"]].tolist()
    return sorted(range(len(r)), key=lambda k: (rk[k], bins[k], -k)), bins


def row_line(kind, t, k, count, reads_num, total=0.0):
    r = t["rows"][k]
    return py_line(kind, t["chroms"][t["row_chrom"][k]], t["reps"][r["rep"]], t["clas"][r["cla"]], t["fams"][r["fam"]], int(r["start"]), int(r["end"]), int(count),
                   reads_num, total)


def make_counts(n, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 40, n).astype(np.int64)
    pick = rng.integers(0, 2 * len(COUNTS), n)
    for i, c in enumerate(COUNTS):
        cnt[pick == i] = c
    return cnt.astype(np.uint32)


# ---- 1. order and text

SIZES = [0, 1, 255, 256, 257, 70_000]


@pytest.mark.parametrize("n_chrom", [1, 3, 300])
@pytest.mark.parametrize("n", SIZES)
def test_order_and_filter_text(n, n_chrom):
    t = make_table(n, n_chrom)
    order, bins = want_order(t)
    lo = Loci(FILTER, t)
    assert lo.order() == order
    if n >= 70_000:
        assert {sum(b >= o for o in (1, 9, 73, 585, 4681)) for b in bins} == {0, 1, 2, 3, 4, 5}
        assert max(np.bincount(np.array(bins) + 8192 * t["rank"][t["row_chrom"]].astype(np.int64))) > 50       # one bin, many rows
    cnt = make_counts(n, 5 + n)
    if n:
        cnt[0] = 2 ** 31 - 1
    above = int(cnt.max()) + 1 if n else 1
    assert above <= 2 ** 31
    for reads_num in READS:
        lines = [row_line(FILTER, t, k, cnt[k], reads_num) for k in order]
        cs = cnt[order].astype(np.int64)
        for thr in ([-1, 0, 1, 5, 2 ** 31 - 1] if reads_num == READS[1] else [1]):
            text, n_lines, hard = lo.filter_text(cnt, thr, reads_num)
            keep = np.flatnonzero(cs >= thr)
            assert hard == 0 and n_lines == len(keep), (thr, reads_num)
            assert text == b"".join(lines[j] for j in keep), (thr, reads_num)
    c2 = np.minimum(cnt, 2 ** 31 - 2)                                     # a threshold above every count: no text, no lines
    text, n_lines, hard = lo.filter_text(c2, 2 ** 31 - 1, 7)
    assert (text, n_lines, hard) == (b"", 0, 0)
    lo.close()


def test_counts_with_the_sign_bit():
    """(int)count: a count of 2^31 and above is negative to the threshold compare and prints with a sign (generic.c:1724-1728)"""
    t = make_table(300, 3)
    t["rows"]["start"][17], t["rows"]["end"][17] = 1000, 2000             # 2^64 / (0.36 * 1000): an RPKM below 2^63
    order, _ = want_order(t)
    cnt = make_counts(300, 1)
    cnt[5], cnt[17] = 2 ** 31, 2 ** 32 - 1
    lo = Loci(FILTER, t)
    text, n_lines, hard = lo.filter_text(cnt, -1, 360_000_000)
    keep = [k for k in order if int(cnt[k].astype(np.int32)) >= -1]
    assert 5 not in keep and 17 in keep
    assert hard == 0 and n_lines == len(keep) and text == b"".join(row_line(FILTER, t, k, cnt[k], 360_000_000) for k in keep)
    assert b"\t-1\t%.3f\t" % (float(2 ** 64) / (360_000_000 * 1e-9 * 1000.0)) in text
    lo.close()


# ---- 2. long names

def test_long_names_pass_several_windows():
    t = make_table(700, 3, long_names=True)
    order, _ = want_order(t)
    cnt = make_counts(700, 2)
    lo = Loci(FILTER, t)
    assert lo.order() == order
    lines = [row_line(FILTER, t, k, cnt[k], 360_000_000) for k in order]
    assert sum(len(x) for x in lines[:256]) > 2 * 32768 and max(len(x) for x in lines) > 700       # the first tile: three windows
    text, n_lines, hard = lo.filter_text(cnt, 0, 360_000_000)
    assert hard == 0 and n_lines == 700 and text == b"".join(lines)
    text, n_lines, hard = lo.filter_text(cnt, 10, 360_000_000)
    assert text == b"".join(x for x, k in zip(lines, order) if cnt[k] >= 10)
    lo.close()


# ---- 3. the host has to look

def test_hard_lines_hand_out_nothing():
    t = make_table(600, 3)
    t["rows"]["start"][300] = t["rows"]["end"][300] = 5000                # binKeeperAdd accepts start == end
    order, _ = want_order(t)
    cnt = np.full(600, 3, np.uint32)
    lo = Loci(FILTER, t)
    assert lo.order() == order
    text, n_lines, hard = lo.filter_text(cnt, 1, 0)                       # a read number of 0: every printed line is inf
    assert text is None and hard == 600
    text, n_lines, hard = lo.filter_text(np.zeros(600, np.uint32), 0, 0)  # 0 / 0
    assert text is None and hard == 600
    text, n_lines, hard = lo.filter_text(cnt, 1, 1000)                    # one printed row of length 0
    assert text is None and hard == 1
    cnt[300] = 0                                                          # the same row below the threshold is nobody's business
    text, n_lines, hard = lo.filter_text(cnt, 1, 1000)
    assert hard == 0 and n_lines == 599 and text == b"".join(row_line(FILTER, t, k, 3, 1000) for k in order if k != 300)
    lo.close()
    lc = Loci(CPG, t)
    tot = np.full(600, 1.5)
    tot[17] = np.inf
    assert lc.cpg_text(cnt.astype(np.int32), tot, 0.0)[::2] == (None, 1)
    tot[17] = 2.0 ** 63
    assert lc.cpg_text(cnt.astype(np.int32), tot, 0.0)[::2] == (None, 1)
    tot[17] = np.nan                                                      # nan > t is false: not printed, not hard
    text, n_lines, hard = lc.cpg_text(cnt.astype(np.int32), tot, 0.0)
    assert hard == 0 and n_lines == 599
    tot[17] = np.inf                                                      # inf below an infinite threshold: not printed either
    assert lc.cpg_text(cnt.astype(np.int32), tot, np.inf)[1:] == (0, 0)
    lc.close()


# ---- 4. the CpG kind

@pytest.mark.parametrize("n", [257, 70_000])
def test_cpg_text(n):
    t = make_table(n, 3, seed=3)
    order, _ = want_order(t)
    rng = np.random.default_rng(n)
    cnt = rng.integers(0, 2000, n).astype(np.int32)
    cnt[:3] = [0, 2 ** 31 - 1, -5]
    tot = np.round(rng.normal(0.5, 3.0, n), 2)
    ties = np.array([0.0625, 0.1875, -0.0625, -0.4375, 0.5, 0.0, -0.0, -0.0001, 1234567.0005, 2.0 ** 52 + 1, -(2.0 ** 63 - 1024), 4.9e-324])
    tot[:len(ties)] = ties
    tot[20:60] = rng.integers(-50, 50, 40) + rng.choice(ties[:4], 40)
    lc = Loci(CPG, t)
    assert lc.order() == order
    lines = [row_line(CPG, t, k, cnt[k], 0, float(tot[k])) for k in order]
    ts = tot[order]
    for thr in (0.0, 0.5, -1.0):
        text, n_lines, hard = lc.cpg_text(cnt, tot, thr)
        keep = np.flatnonzero(ts > thr)
        assert hard == 0 and n_lines == len(keep) and text == b"".join(lines[j] for j in keep), thr
    assert b"\t-0.000\n" in b"".join(lines) and b"\t0.062\n" in b"".join(lines) and b"\t-0.438\n" in b"".join(lines)
    lc.close()


# ---- 5. argument checks

def test_argument_checks():
    L = eng.load()
    t = make_table(10, 3)
    (cb, co), (rb, ro), (kb, ko), (fb, fo) = [_table(t[k]) for k in ("chroms", "reps", "clas", "fams")]
    h = C.c_void_p()

    def create(kind=FILTER, rows=t["rows"], rc_=t["row_chrom"], n=10, rank=t["rank"], nc=3, co_=co, ro_=ro, out=h):
        return L.itx_loci_create(0, kind, _p(rows), _p(rc_), n, _p(rank), nc, _p(cb), _p(co_), _p(rb), _p(ro_), len(t["reps"]), _p(kb), _p(ko), len(t["clas"]), _p(fb),
                                 _p(fo), len(t["fams"]), C.byref(out) if out is not None else None)
    assert create(out=None) == -1 and create(kind=2) == -1 and create(rows=None) == -1 and create(rc_=None) == -1 and create(rank=None) == -1
    assert create(co_=None) == -1 and create(ro_=None) == -1 and b"itx_loci_create" in L.itx_last_error()
    big_rank, big_off = np.zeros(1 << 19, np.uint32), np.zeros((1 << 19) + 1, np.uint64)
    assert create(rank=big_rank, nc=1 << 19, co_=big_off) == -2                                    # ITX_E_RANGE, before anything is allocated
    bad = t["rows"].copy()
    bad["rep"][4] = len(t["reps"])
    assert create(rows=bad) == -1
    far = t["rows"].copy()
    far["start"][2], far["end"][2] = 470_000_000, 470_000_100                                      # bin 4681 + 3585: not the key's
    assert create(rows=far) == -2 and b"bin" in L.itx_last_error()
    desc = co.copy()
    desc[1], desc[2] = desc[2], desc[1]
    assert create(co_=desc) == -1
    assert create(rank=np.array([0, 1, 3], np.uint32)) == -1
    assert h.value is None
    res = eng.LociText()
    cnt, tot = np.zeros(10, np.uint32), np.zeros(10)
    assert L.itx_loci_filter_text(None, _p(cnt), 1, 5, C.byref(res)) == -1 and L.itx_loci_cpg_text(None, _p(cnt), _p(tot), 0.0, C.byref(res)) == -1
    assert L.itx_loci_order(None, None, None) == -1
    lo, lc = Loci(FILTER, t), Loci(CPG, t)
    assert L.itx_loci_filter_text(lo._h, None, 1, 5, C.byref(res)) == -1 and L.itx_loci_filter_text(lo._h, _p(cnt), 1, 5, None) == -1
    assert L.itx_loci_cpg_text(lo._h, _p(cnt), _p(tot), 0.0, C.byref(res)) == -1 and b"filter" in L.itx_last_error()       # counts of the wrong kind
    assert L.itx_loci_filter_text(lc._h, _p(cnt), 1, 5, C.byref(res)) == -1 and b"cpgfilter" in L.itx_last_error()
    assert L.itx_loci_cpg_text(lc._h, _p(cnt), None, 0.0, C.byref(res)) == -1 and L.itx_loci_order(lo._h, None, None) == -1
    assert L.itx_loci_filter_text(lo._h, _p(cnt), 0, 5, C.byref(res)) == 0 and res.lines == 10                             # and the object is as good as before
    lo.close()
    lc.close()
    L.itx_loci_destroy(None)


# ---- 6. the command

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


DEVICE_LINE = re.compile(r"\[itx timing\] loci: (\d+) lines built on the device \((\d+) bytes, sort [0-9.]+ ms, text [0-9.]+ ms, host waited [0-9.]+ s\)")
HOST_LINE = re.compile(r"\[itx timing\] loci: (\d+) lines written by the host \((.+)\)")
RUNS = gc.list_runs("filter") + gc.list_runs("cpgfilter")


@pytest.mark.parametrize("case,run_name", RUNS, ids=[f"{c}-{r}" for c, r in RUNS])
def test_golden_runs_by_both_routes(case, run_name, exe, tmp_path):
    run = gc.manifest_run(case, run_name)
    src = os.path.join(gc.GOLDEN, case, "in")
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", run["aln"]]]
    for route in ("0", "1"):
        work = tmp_path / ("route" + route)
        work.mkdir()
        pr = subprocess.run([exe, run["cmd"]] + run["opts"] + ["-o", run["prefix"]] + paths, cwd=work, capture_output=True, text=True, timeout=600,
                            env=dict(os.environ, ITX_TIMING="1", ITX_HOST_LOCI=route))
        assert pr.returncode == run["rc"], pr.stderr[-2000:]
        for fn in run["files"]:
            assert (work / fn).read_bytes() == refio.read_bytes(os.path.join(gc.GOLDEN, case, run_name, fn)), (route, fn)
        for ln in run["stderr_tail"]:
            if ln.startswith("* Total"):
                assert ln in pr.stderr, (route, ln)
        dev, host = DEVICE_LINE.search(pr.stderr), HOST_LINE.search(pr.stderr)
        if route == "0" and "-r" not in run["opts"]:
            assert dev and not host, pr.stderr[-1500:]
            loci = [fn for fn in run["files"] if fn.endswith(".loci")][0]
            body = (work / loci).read_bytes().split(b"\n", 1)[1]
            assert int(dev.group(1)) == body.count(b"\n") and int(dev.group(2)) == len(body)
        else:
            assert host and not dev, pr.stderr[-1500:]
            assert ("-r" in host.group(2)) == ("-r" in run["opts"]) and ("ITX_HOST_LOCI=1" in host.group(2)) == ("-r" not in run["opts"])


def test_the_host_is_the_default_until_measured(exe, tmp_path):
    run = gc.manifest_run("mid", "filter_f")
    src = os.path.join(gc.GOLDEN, "mid", "in")
    paths = [refio.materialise(src, n, str(tmp_path)) for n in ["chrom.sizes", "rep.sizes", "rmsk.txt", run["aln"]]]
    env = {k: v for k, v in os.environ.items() if k != "ITX_HOST_LOCI"}
    pr = subprocess.run([exe, "filter"] + run["opts"] + ["-o", "out"] + paths, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(env, ITX_TIMING="1"))
    assert pr.returncode == 0 and "ITX_HOST_LOCI is not set" in HOST_LINE.search(pr.stderr).group(2)


# ---- 7. every read below -Q: the read number of -N 0 is 0

def test_reads_below_Q_leave_the_file_to_the_host(exe, tmp_path):
    chroms = [("chr1", 2_000_000), ("chr2", 500_000)]
    t = synth.make_table(5, chroms, 300, n_names=20, n_fams=5, n_clas=3)
    synth.write_sizes(str(tmp_path / "chrom.sizes"), chroms)
    synth.write_sizes(str(tmp_path / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(tmp_path / "rmsk.txt"), t)
    n_rows = len(t.chrom)
    recs = [bc.record(tid=int(t.chrom[i]), pos=int(t.start[i]), mapq=3, qname=b"q%d\0" % i, cigar=((0, 50),), l_qseq=0) for i in np.argsort(t.chrom, kind="stable")[:200]]
    (tmp_path / "reads.bam").write_bytes(bc.bam_bytes(chroms, recs))
    args = ["filter", "-Q", "10", "-N", "0", "-t", "0", "-o", "out", str(tmp_path / "chrom.sizes"), str(tmp_path / "rep.sizes"), str(tmp_path / "rmsk.txt"),
            str(tmp_path / "reads.bam")]
    outs = {}
    for route in ("0", "1"):
        work = tmp_path / ("route" + route)
        work.mkdir()
        pr = subprocess.run([exe] + args, cwd=work, capture_output=True, text=True, timeout=600, env=dict(os.environ, ITX_TIMING="1", ITX_HOST_LOCI=route))
        assert pr.returncode == 0, pr.stderr[-2000:]
        outs[route] = ((work / "out_ALL.iteres.loci").read_bytes(), (work / "out_ALL.iteres.reportloci").read_bytes())
        host = HOST_LINE.search(pr.stderr)
        assert host and not DEVICE_LINE.search(pr.stderr), pr.stderr[-1500:]
        if route == "0":
            assert "lines hold a number the device does not print" in host.group(2) and host.group(2).split()[0] == str(n_rows)
    assert outs["0"] == outs["1"] and outs["0"][0].count(b"\n") == n_rows + 1 and b"nan" in outs["0"][0]
    if os.path.exists(REF):
        work = tmp_path / "ref"
        work.mkdir()
        assert subprocess.run([REF] + args, cwd=work, capture_output=True, text=True, timeout=600).returncode == 0
        assert ((work / "out_ALL.iteres.loci").read_bytes(), (work / "out_ALL.iteres.reportloci").read_bytes()) == outs["0"]
