"""GPU: the repeat table built on the device (csrc/itx_table.hip, table_create_device) against the host build it replaces
(ITX_TABLE_HOST=1, the oracle): every array of the built table (itx_table_debug_copy) and every field of itx_table_get_info must be
equal, on small tables chosen for where the device build can go wrong — ties in both sort orders, all six bin levels, the sort's
chunk and workgroup boundaries, more than 256 chromosomes (some empty, some with one row), a chromosome boundary inside a block of the
running maximum, one early long row that dominates it over several blocks, the unit cases, both ends of the bin-width choice, bad
rows. Then the engine on a 50 k-row table against the oracle with each build, and the command with each build, file by file."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import enginecase as ec
import gcovcase as gv
from iteres_amd import build
from iteres_amd import engine as eng
from iteres_amd import synth

pytestmark = pytest.mark.gpu

SORT_CHUNK = 8192                      # csrc/itx_radixsort.h; also the rows of one workgroup of the running maximum (256 x 32)
IV = np.dtype([(k, "<i4") for k in ("s", "e", "pbelow")] + [(k, "<u4") for k in ("rank", "cs", "jcap", "covslot", "zslot")])
DTYPES = {"iv": IV, "orig": np.dtype("<i4"), "bl": np.dtype([("x", "<u4"), ("y", "<u4")]), "row_unit": np.dtype("<u4"), "part_unit": np.dtype("<u4"),
          "unit_slot": np.dtype("<u4"), "unit_ids": np.dtype([(k, "<u4") for k in "xyzw"]), "unit_covoff": np.dtype("<u8"), "chrom_off": np.dtype("<u4"),
          "bin_off": np.dtype("<u4")}
INFO = ("n_rows", "n_rep", "n_fam", "n_cla", "cov_len", "n_units", "n_slots", "table_bytes", "n_chrom", "bin_shift", "device")


def _build(monkeypatch, host, rows, cs, rl, nf, nc):
    if host:
        monkeypatch.setenv("ITX_TABLE_HOST", "1")
    else:
        monkeypatch.delenv("ITX_TABLE_HOST", raising=False)
    return eng.Table(rows, cs, rl, nf, nc)


def same_tables(monkeypatch, rows, cs, rl, nf, nc):
    """builds the table both ways and holds every array and every scalar equal; returns the device build's (info, arrays)"""
    out = []
    for host in (False, True):
        t = _build(monkeypatch, host, rows, cs, rl, nf, nc)
        out.append(({k: getattr(t.info, k) for k in INFO}, {k: v.view(DTYPES[k]) for k, v in t.snapshot().items()}))
        t.close()
    (di, da), (hi, ha) = out
    assert di == hi
    for k in eng.Table.SNAPSHOT:
        assert da[k].shape == ha[k].shape, k
        if not np.array_equal(da[k], ha[k]):
            at = int(np.flatnonzero(da[k] != ha[k])[0])
            raise AssertionError(f"{k}[{at}]: device {da[k][at]}, host {ha[k][at]} ({int((da[k] != ha[k]).sum())} of {len(da[k])} differ)")
    return di, da


def random_rows(seed, n, sizes, n_rep=37, max_len=3000, n_starts=None):
    """n valid rows over the chromosomes in random file order; n_starts: that few distinct starts per chromosome (ties)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    ok = np.flatnonzero(sizes > 1)
    chrom = ok[rng.integers(0, len(ok), n)]
    sz = sizes[chrom]
    start = (rng.random(n) * (sz - 1)).astype(np.int64)
    if n_starts:
        start = (start // np.maximum(sz // n_starts, 1)) * np.maximum(sz // n_starts, 1)
    end = np.minimum(start + 1 + rng.integers(0, max_len, n), sz)
    rep = rng.integers(0, n_rep, n)
    rows = eng.make_rows(chrom.astype(np.int32), start, end, rng.integers(0, 50, n), rng.integers(0, 400, n), rep, rep % 5, rep % 3)
    rl = rng.integers(1, 300, n_rep).astype(np.uint32)
    return rows, rl, 5, 3


def test_ties_in_both_orders(monkeypatch):
    """few distinct starts and few distinct (level, bin): file order decides in the order by start and in the ranks"""
    sizes = [3_000_000, 700_000]
    rows, rl, nf, nc = random_rows(1, 6000, sizes, n_starts=40, max_len=200_000)
    info, a = same_tables(monkeypatch, rows, sizes, rl, nf, nc)
    iv = a["iv"]
    assert (np.diff(iv["s"]) == 0).sum() > 4000                      # most neighbours start together ...
    same = np.flatnonzero((np.diff(iv["s"]) == 0) & (np.diff(a["orig"]) != 0))
    first = a["chrom_off"][1]
    same = same[(same + 1 != first)]
    assert (a["orig"][same] < a["orig"][same + 1]).all()           # ... and stand in file order


def test_all_six_levels_and_wide_bins(monkeypatch):
    """ends that cross the 128 kb, 1 Mb, 8 Mb, 64 Mb and 512 Mb boundaries; three chromosomes of 2^31 - 1 take the widest bins (shift 17)"""
    size = 0x7fffffff
    bounds = [1 << 17, 1 << 20, 1 << 23, 1 << 26, 1 << 29]
    s, e = [], []
    for k, b in enumerate(bounds):
        for m in (1, 3):
            if b * m < size:
                s += [b * m - 10, b * m - 1, b * m, b * m - 5000]
                e += [b * m + 10, b * m + 1, b * m + 7, b * m]
    s += [0, 5, size - 1, 0, 1 << 30]
    e += [1, 100, size, size, (1 << 30) + 50]
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(s))
    s, e = np.asarray(s, np.int64)[perm], np.asarray(e, np.int64)[perm]
    n = len(s)
    rep = rng.integers(0, 4, n)
    rows = eng.make_rows(rng.integers(0, 3, n).astype(np.int32), s, e, np.zeros(n), np.full(n, 100), rep, rep, rep)
    info, a = same_tables(monkeypatch, rows, [size] * 3, np.array([120, 0, 40, 7], np.uint32), 4, 4)
    assert info["bin_shift"] == 17
    levels = set()
    for x, y in zip(s, e):
        sb, eb, lv = int(x) >> 17, (int(y) - 1) >> 17, 0
        while sb != eb:
            sb, eb, lv = sb >> 3, eb >> 3, lv + 1
        levels.add(lv)
    assert levels == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("n", [SORT_CHUNK, SORT_CHUNK + 1, 3 * SORT_CHUNK + 1])
def test_sort_chunk_boundaries(monkeypatch, n):
    """rows that fill a sort chunk exactly, spill one into the next, and span four workgroups; three chromosomes, so that chromosome
    boundaries fall inside blocks of the running maximum"""
    sizes = [5_000_000, 1_200_000, 90_000]
    rows, rl, nf, nc = random_rows(10 + n, n, sizes)
    info, a = same_tables(monkeypatch, rows, sizes, rl, nf, nc)
    assert info["bin_shift"] == 7 and info["n_rows"] == n


def test_three_hundred_chromosomes(monkeypatch):
    """more than 256 chromosomes: two 8-bit passes over the chromosome; some have no rows, some one, one has size 0"""
    rng = np.random.default_rng(3)
    sizes = rng.integers(2_000, 60_000, 300)
    sizes[7] = 0
    rows, rl, nf, nc = random_rows(4, 9000, sizes)
    keep = np.ones(len(rows), bool)
    for c in (0, 11, 255, 256, 299):                                  # no rows at all
        keep &= rows["chrom"] != c
    for c in (1, 257, 298):                                           # exactly one
        idx = np.flatnonzero(rows["chrom"] == c)
        keep[idx[1:]] = False
    rows = rows[keep]
    info, a = same_tables(monkeypatch, rows, sizes, rl, nf, nc)
    per = np.diff(a["chrom_off"].astype(np.int64))
    assert info["n_chrom"] == 300 and (per[[0, 7, 11, 255, 256, 299]] == 0).all() and (per[[1, 257, 298]] == 1).all()


def test_chromosome_boundary_inside_a_scan_block_and_a_dominating_row(monkeypatch):
    """chromosome 0 ends 17 rows into the second block of the running maximum; chromosome 1 begins with a row that reaches its end, so
    its end is every later row's pbelow across the next three blocks, and must not leak back into chromosome 0 or on into 2"""
    n0, n1, n2 = SORT_CHUNK + 17, 3 * SORT_CHUNK, 100
    sizes = [4_000_000, 9_000_000, 50_000]
    rng = np.random.default_rng(5)
    chrom = np.concatenate([np.zeros(n0), np.ones(n1), np.full(n2, 2)]).astype(np.int32)
    sz = np.asarray(sizes)[chrom]
    start = (rng.random(len(chrom)) * (sz - 400)).astype(np.int64) + 200
    end = start + rng.integers(1, 150, len(chrom))
    start[n0], end[n0] = 0, sizes[1]                                  # the long row: first of chromosome 1 by start
    perm = rng.permutation(len(chrom))
    rep = rng.integers(0, 9, len(chrom))
    rows = eng.make_rows(chrom[perm], start[perm], end[perm], np.zeros(len(chrom)), np.full(len(chrom), 90), rep[perm], rep[perm] % 2, np.zeros(len(chrom)))
    info, a = same_tables(monkeypatch, rows, sizes, np.full(9, 77, np.uint32), 2, 1)
    iv, off = a["iv"], a["chrom_off"]
    assert off[1] == n0 and off[2] == n0 + n1
    assert iv["pbelow"][off[1]] == np.iinfo(np.int32).min and (iv["pbelow"][off[1] + 1:off[2]] == sizes[1]).all()
    assert iv["pbelow"][off[0]] == np.iinfo(np.int32).min and iv["pbelow"][off[2]] == np.iinfo(np.int32).min
    assert iv["pbelow"][:off[1]].max() < sizes[0] and iv["pbelow"][off[2]:].max() < sizes[2]


def test_units(monkeypatch):
    """a name with two (family, class) pairs — its rows' units are neighbours and not solo —, a name of length 0, a name no row uses"""
    #            name 0: (0, 0) and (1, 0), first seen as (1, 0); name 1: length 0; name 2: unused; name 3: one pair
    rep = [0, 3, 0, 1, 0, 3, 1, 0]
    fam = [1, 2, 0, 0, 1, 2, 0, 0]
    cla = [0, 1, 0, 1, 0, 1, 1, 0]
    n = len(rep)
    rows = eng.make_rows(np.zeros(n, np.int32), np.arange(n) * 100, np.arange(n) * 100 + 250, np.zeros(n), np.full(n, 60), rep, fam, cla)
    info, a = same_tables(monkeypatch, rows, [100_000], np.array([50, 0, 9, 20], np.uint32), 3, 2)
    assert info["n_units"] == 4
    assert [tuple(int(v) for v in u) for u in a["unit_ids"]] == [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 1, 1), (3, 2, 1, 1)]
    assert list(a["unit_slot"]) == [0, 51, 102, 103, 124] and info["n_slots"] == 124
    assert list(a["row_unit"][np.argsort(a["orig"])]) == [1, 3, 0, 2, 1, 3, 2, 0]


def test_no_rows(monkeypatch):
    info, a = same_tables(monkeypatch, np.zeros(0, eng.ROW_DTYPE), [1000, 70_000], np.array([5, 6], np.uint32), 1, 1)
    assert info["n_rows"] == 0 and info["n_units"] == 0 and len(a["iv"]) == 0 and (a["bl"]["x"] == 0).all() and (a["bl"]["y"] == 0).all()
    assert list(a["part_unit"]) == [0, 0]


def test_narrowest_bins_many_windows(monkeypatch):
    """shift 7 (a small genome) with a slot space of many windows of 2^13 slots: the windows' first units by bisection"""
    sizes = [2_000_000]
    rows, rl, nf, nc = random_rows(6, 3000, sizes, n_rep=600)
    rl = (rl.astype(np.int64) * 40).astype(np.uint32)
    info, a = same_tables(monkeypatch, rows, sizes, rl, nf, nc)
    assert info["bin_shift"] == 7 and len(a["part_unit"]) > 100 and len(set(a["part_unit"].tolist())) > 50


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_first_of_several_bad_rows(monkeypatch, host):
    """the first bad row is reported, whatever follows it: same code, same *bad_row, no table"""
    sizes = [500_000, 80_000]
    rows, rl, nf, nc = random_rows(7, 20_000, sizes)
    rows["end"][15_000] = sizes[rows["chrom"][15_000]] + 1            # past its chromosome
    rows["rep"][4_321] = 1000                                         # no such name: the FIRST bad row
    rows["chrom"][19_999] = 2                                         # no such chromosome
    rows["start"][4_322], rows["end"][4_322] = 0, 0                   # empty at 0: fits no bin
    if host:
        monkeypatch.setenv("ITX_TABLE_HOST", "1")
    else:
        monkeypatch.delenv("ITX_TABLE_HOST", raising=False)
    import ctypes as C
    L = eng.load()
    h, bad = C.c_void_p(), C.c_size_t(77)
    cs = np.asarray(sizes, np.int64)
    rc = L.itx_table_create(rows.ctypes.data_as(C.c_void_p), len(rows), cs.ctypes.data_as(C.c_void_p), 2, rl.ctypes.data_as(C.c_void_p), len(rl), nf, nc, 0,
                            C.byref(h), C.byref(bad))
    assert rc == -2 and bad.value == 4_321 and not h.value            # ITX_E_RANGE
    assert b"row 4321 " in L.itx_last_error()


# ---- the engine on a 50 k-row table, against the oracle, with each build

@pytest.fixture(scope="module")
def engine_case():
    chroms = [("c1", 30_000_000), ("c2", 9_000_000), ("c3", 300_000)]
    t = synth.make_table(31, chroms, 50_000, n_names=500, n_fams=40, n_clas=12, overlap_frac=0.05, shuffle_frac=0.03, inconsistent_frac=0.01)
    rl = np.array([t.rep_len.get(n, 0) for n in t.names], np.uint32)
    rows = eng.make_rows(t.chrom, t.start, t.end, t.cons_start, t.cons_end, t.rep_name, t.fam_of_row, t.cla_of_row)
    r = synth.make_reads(32, list(chroms) + [("chrNotInSizes", 5000)], 60_000, read_len=(30, 150), paired_frac=0.3, odd_cigar_frac=0.1)
    rd = {"tid": r.tid, "pos": r.pos, "tmpend": r.tmpend(), "mapq": r.mapq, "flag": r.flag, "mpos": r.mpos, "isize": r.isize}
    cs = np.array([s for _, s in chroms], np.int64)
    t2c = np.array([0, 1, 2, -1], np.int32)
    want = {}
    ot = ec.oracle_table(rows, cs, rl, len(t.fams), len(t.clas))
    for mode in ("stat", "filter"):
        want[mode] = ot.run(dict(filter_mode=mode == "filter"), t2c, rd["tid"], rd["pos"], rd["tmpend"], rd["mapq"], rd["flag"], rd["mpos"], rd["isize"])
    ot.close()
    return rows, cs, rl, len(t.fams), len(t.clas), t2c, rd, want


@pytest.mark.parametrize("mode", ["stat", "filter"])
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_engine_against_the_oracle(monkeypatch, engine_case, host, mode):
    rows, cs, rl, nf, nc, t2c, rd, want = engine_case
    t = _build(monkeypatch, host, rows, cs, rl, nf, nc)
    e = eng.Engine(t, dict(filter_mode=mode == "filter"), batch_capacity=25_000)
    e.set_tidmap(t2c)
    hits = e.submit_host(rd["tid"], rd["pos"], rd["tmpend"], rd["mapq"], eng.flag5(rd["flag"]), rd["mpos"], rd["isize"], want_hits=True)
    got = e.finish()
    e.close()
    t.close()
    ec.assert_same(got, want[mode], hits, mode == "filter", len(rows))
    assert int(want[mode]["cnt"][9]) > 5_000


# ---- the command with each build

@pytest.mark.parametrize("cmd,opts", [("stat", ("-w",)), ("filter", ("-G",))])
def test_command_with_each_build(tmp_path, cmd, opts):
    """every output file of a run is the same with the table built on the device and by the host"""
    lib, exe = build.build_all()
    d = str(tmp_path / "in")
    gv.make_inputs(d)
    files = [os.path.join(d, f) for f in ("chrom.sizes", "rep.sizes", "rmsk.txt", "reads.bam")]
    outs = {}
    for name, env in (("device", {}), ("host", {"ITX_TABLE_HOST": "1"})):
        out = str(tmp_path / name)
        os.makedirs(out)
        base = {k: v for k, v in os.environ.items() if k != "ITX_TABLE_HOST"}
        pr = subprocess.run([exe, cmd] + list(opts) + ["-o", "out"] + files, cwd=out, capture_output=True, text=True, timeout=600,
                            env=dict(base, ITX_TIMING="1", ITX_TIMING_TABLE="1", **env))
        assert pr.returncode == 0, pr.stderr[-2000:]
        assert ("table: device" in pr.stderr) == (name == "device"), pr.stderr[-2000:]
        outs[name] = out
    names = sorted(os.listdir(outs["device"]))
    assert names == sorted(os.listdir(outs["host"])) and len(names) >= 3
    for fn in names:
        assert filecmp.cmp(os.path.join(outs["device"], fn), os.path.join(outs["host"], fn), shallow=False), fn
