"""GPU: `filter -b -a`, every emitted record tagged with the row it was counted for (include/iteres_amd.h
itx_bamout_annotate_enable, csrc/itx_bamout.hip k_bo_measure<true> / k_bo_gather<uint32_t, true>, the rule: csrc/itx_reptag.h).
1. the ABI on built records: the expected stream is the Python restatement (tests/reptagcase.py) applied to the counted records;
   the emitted members inflate to it (refio.bgzf_decompress) and are the host build of the member rule over it. Tiles, rows, cuts
   by a payload boundary at every kind of place in a record, the LDS window, host appends, the sort, the index, the levels;
2. without annotate_enable nothing changes; state and argument checks;
3. the command: the file with the tags taken off is the file of the run without -a, every record's tags are those of the row the
   CPU oracle chooses, the records group to the .loci file's counts, and the other outputs do not move."""
import collections
import ctypes as C
import filecmp
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import baicase as bai
import bgzfmemberhost as bm
import goldencase as gc
import refbam
import refio
import reptagcase as rt
from iteres_amd import engine as eng
from oracle import binding as orc
from test_gpu_bamout import REF, exe, mixed_records, pile, raw_records, rec_of_len, routes, rule, run_filter, tensors   # noqa: F401  (fixtures too)
from test_gpu_bamsort import key_of, split_records, srec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = bai.PAYLOAD                               # 8192: bytes of the stream per member
LDS = 32768                                   # bytes k_bo_gather stages at a time (csrc/itx_bamout.hip BO_LDS)
TILE = 256


# ---- the table of the ABI tests

def table(n_rows, seed=3, name_len=None):
    """rows (engine.ROW_DTYPE) over 5 / 3 / 4 names; name_len: the length of every name (default: 3 .. 12 bytes)"""
    rng = np.random.default_rng(seed)

    def names(n, first):
        return [bytes([first + k]) * (name_len if name_len is not None else 3 + (k * 5) % 10) for k in range(n)]
    reps, clas, fams = names(5, 65), names(3, 97), names(4, 75)
    rows = np.zeros(n_rows, eng.ROW_DTYPE)
    rows["start"] = rng.integers(0, 2**32, n_rows, dtype=np.uint64).astype(np.uint32)
    rows["end"] = rng.integers(0, 2**32, n_rows, dtype=np.uint64).astype(np.uint32)
    rows["rep"], rows["cla"], rows["fam"] = np.arange(n_rows) % 5, np.arange(n_rows) % 3, np.arange(n_rows) % 4
    return rows, reps, clas, fams


def tag_len(tab, row):
    rows, reps, clas, fams = tab
    w = rows[row]
    return 26 + len(reps[w["rep"]]) + len(clas[w["cla"]]) + len(fams[w["fam"]])


def expected(tab, recs, hit):
    return b"".join(rt.annotate_rows(recs, hit, *tab))


def check_stream(rule, got, want):
    """got: every member handed out; want: the annotated records, one behind the other"""
    assert refio.bgzf_decompress(got) == want
    ms = bm.split_members(got)
    assert ms == rule.members(want)
    return ms


def run_annotated(rule, tab, recs, hit, cap=None, level=None):
    import torch
    bo = eng.Bamout(batch_capacity=cap or max(len(recs), 1))
    try:
        if level is not None:
            bo.set_level(level)
        bo.annotate_enable(*tab)
        raw, off = tensors(recs)
        bo.run(raw, off, torch.from_numpy(np.asarray(hit, np.int32)).cuda())
        bo.wait_kernels()
        got = bo.finish()
        st, tb = bo.stats(), bo.tag_bytes()
    finally:
        bo.close()
    want = expected(tab, recs, hit)
    if level is None:
        check_stream(rule, got, want)
    else:
        assert refio.bgzf_decompress(got) == want
    n_hit = int((np.asarray(hit) >= 0).sum())
    assert st["records"] == n_hit and st["payload_bytes"] == len(want)
    assert tb == len(want) - sum(len(r) for r, h in zip(recs, hit) if h >= 0)
    return got, want


TAB7 = table(7)


def pattern(kind, n, n_rows=7):
    i = np.arange(n)
    return {"all": i % n_rows, "none": np.full(n, -1), "alternating": np.where(i % 2 == 0, i % n_rows, -1), "first": np.where(i == 0, 2, -1),
            "last": np.where(i == n - 1, n_rows - 1, -1)}[kind].astype(np.int32)


@pytest.mark.parametrize("kind", ["all", "none", "alternating", "first", "last"])
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tiles(rule, n, kind):
    run_annotated(rule, TAB7, mixed_records(n, n), pattern(kind, n))


@pytest.mark.parametrize("n_rows", [1, 2, 70_001])
@pytest.mark.parametrize("name_len", [1, 254])
def test_first_and_last_row_of_a_table(rule, n_rows, name_len):
    tab = table(n_rows, seed=n_rows, name_len=name_len)
    recs = mixed_records(5, 40)
    hit = np.where(np.arange(40) % 3 == 0, 0, np.where(np.arange(40) % 3 == 1, n_rows - 1, -1)).astype(np.int32)
    got, want = run_annotated(rule, tab, recs, hit)
    first = rt.strip(split_records(want)[1])[1]                             # (record 1: the last row)
    assert first[3:] == (int(tab[0][-1]["start"]), int(tab[0][-1]["end"])) and len(first[0]) == name_len


def test_a_row_with_three_empty_names(rule):
    rows, reps, clas, fams = table(4)
    reps, clas, fams = reps + [b""], clas + [b""], fams + [b""]
    rows[2]["rep"], rows[2]["cla"], rows[2]["fam"] = 5, 3, 4
    recs = mixed_records(6, 30)
    hit = (np.arange(30) % 4).astype(np.int32)
    got, want = run_annotated(rule, (rows, reps, clas, fams), recs, hit)
    r2 = split_records(want)[2]
    assert r2.endswith(b"ZNZ\0ZCZ\0ZFZ\0ZSI" + struct.pack("<I", rows[2]["start"]) + b"ZEI" + struct.pack("<I", rows[2]["end"])) and len(r2) == len(recs[2]) + 26


# ---- a payload boundary at every kind of place inside an annotated record

EDGE_L = 300                                  # the cut record's own bytes
EDGE_ROW = 4                                  # TAB7's row 4: repName 4, repClass 1, repFamily 0


def edge_places():
    rows, reps, clas, fams = TAB7
    nl, cl, fl = (len(t[rows[EDGE_ROW][k]]) for t, k in ((reps, "rep"), (clas, "cla"), (fams, "fam")))
    zs = EDGE_L + 12 + nl + cl + fl                                         # where the ZS key starts
    out = {"in_block_size_%d" % k: k for k in (1, 2, 3)}
    out.update(last_original_byte=EDGE_L - 1, behind_the_original=EDGE_L, in_ZN_key_1=EDGE_L + 1, in_ZN_key_2=EDGE_L + 2, name_starts=EDGE_L + 3, in_name=EDGE_L + 5,
               on_NUL=EDGE_L + 3 + nl, behind_NUL=EDGE_L + 4 + nl)
    out.update({"ZS_integer_byte_%d" % k: zs + 3 + k for k in range(5)})
    out.update(in_ZE_key=zs + 8, last_byte=zs + 13)
    return out


@pytest.mark.parametrize("place", list(edge_places()))
def test_a_payload_boundary_inside_the_record(rule, place):
    """the record before it is sized so that byte `k` of the annotated record is the first byte of the second payload"""
    k = edge_places()[place]
    filler = P - k - tag_len(TAB7, 0)
    recs = [rec_of_len(filler, 1), rec_of_len(EDGE_L, 2), rec_of_len(90, 3)]
    hit = np.array([0, EDGE_ROW, 1], np.int32)
    got, want = run_annotated(rule, TAB7, recs, hit)
    assert len(rt.annotate_rows(recs[:1], hit[:1], *TAB7)[0]) == P - k and len(bm.split_members(got)) == 2
    assert refio.bgzf_decompress(bm.split_members(got)[1]) == want[P:]      # the second member starts with byte k of the cut record


def test_a_record_of_three_payloads_and_17_bytes_has_its_tags_in_the_fourth(rule):
    recs = [rec_of_len(3 * P + 17, 1)] + mixed_records(10, 20)
    hit = pattern("all", len(recs))
    got, want = run_annotated(rule, TAB7, recs, hit)
    ms = bm.split_members(got)
    assert len(ms) >= 4 and refio.bgzf_decompress(ms[3])[17:20] == b"ZNZ"


# ---- the LDS window of 32 KiB

@pytest.mark.parametrize("over", [1, 17])
def test_a_tile_whose_tags_take_it_past_the_lds_window(rule, over):
    """one tile: with its tags the tile's bytes pass 32 768 by `over`, without them they stay below"""
    n = 200
    hit = np.zeros(n, np.int32)
    tags = n * tag_len(TAB7, 0)
    own = LDS + over - tags
    lens = [own // n] * n
    lens[-1] += own - sum(lens)
    recs = [rec_of_len(L, i) for i, L in enumerate(lens)]
    assert sum(lens) < LDS < sum(lens) + tags == LDS + over and n < TILE
    run_annotated(rule, TAB7, recs, hit)


def test_a_record_of_40000_bytes_among_short_ones(rule):
    recs = mixed_records(11, 100) + [rec_of_len(40_000, 5)] + mixed_records(12, 100)
    run_annotated(rule, TAB7, recs, pattern("all", len(recs)))
    run_annotated(rule, TAB7, recs, np.where(np.arange(len(recs)) == 100, 6, -1).astype(np.int32))


# ---- several calls, the host's records annotated by the host build of the same header

@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("reptag_gpu") / "libreptag_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "reptag_host.cpp")])
    L = C.CDLL(so)
    L.itxr_len.argtypes = [C.c_uint32] * 3
    L.itxr_len.restype = C.c_uint32
    L.itxr_piece.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                             C.c_void_p]
    L.itxr_piece.restype = None

    def annotate(tab, recs, hit):
        rows, reps, clas, fams = tab
        out = []
        for r, h in zip(recs, hit):
            w = rows[h]
            a, b, c = reps[w["rep"]], clas[w["cla"]], fams[w["fam"]]
            n = len(r) + L.itxr_len(len(a), len(b), len(c))
            buf = C.create_string_buffer(n)
            L.itxr_piece(r, len(r), a, len(a), b, len(b), c, len(c), int(w["start"]), int(w["end"]), 0, n, buf)
            out.append(buf.raw)
        return out
    return annotate


def test_three_calls_with_host_appends_between(rule, host_rule):
    import torch
    bo = eng.Bamout(batch_capacity=600)
    bo.annotate_enable(*TAB7)
    want = []
    for c in range(3):
        recs = mixed_records(40 + c, 513 - c)
        hit = pattern("alternating" if c == 1 else "all", len(recs))
        raw, off = tensors(recs)
        bo.run(raw, off, torch.from_numpy(hit).cuda())
        bo.wait_kernels()
        want += rt.annotate_rows(recs, hit, *TAB7)
        if c < 2:
            hrecs = mixed_records(50 + c, 37)
            hhit = pattern("all", 37)
            mine = host_rule(TAB7, hrecs, hhit)
            assert mine == rt.annotate_rows(hrecs, hhit, *TAB7)             # the C build of the rule, as host/out_bam.c uses it
            bo.append_host(b"".join(mine))
            want += mine
    got = bo.finish()
    st = bo.stats()
    bo.close()
    check_stream(rule, got, b"".join(want))
    assert st["batches"] == 3 and st["host_batches"] == 2 and st["records"] == len(want)


# ---- the sort, the index, the levels

def sorted_case(n=700):
    rng = np.random.default_rng(8)
    recs = [srec(int(rng.integers(0, 3)), int(rng.integers(0, 90_000)), flag=16 * int(rng.integers(0, 2)), name=b"s%d" % i, L=80 + i % 90) for i in range(n)]
    return recs, pattern("all", n)


def test_sort_replays_the_annotated_records_in_two_rounds(rule):
    import torch
    recs, hit = sorted_case()
    l_ref = [100_000] * 3
    bo = eng.Bamout(batch_capacity=400)                                     # 700 records: two runs, then two rounds of the replay
    bo.sort_enable()
    bo.index_enable(l_ref)
    bo.annotate_enable(*TAB7)
    for a, b in ((0, 400), (400, 700)):
        raw, off = tensors(recs[a:b])
        bo.run(raw, off, torch.from_numpy(hit[a:b]).cuda())
        bo.wait_kernels()
        assert bo.out == b""
    got = bo.sort_all()
    status, idx, info = bo.index_finish(0)
    ss, st = bo.sort_stats(), bo.stats()
    bo.close()
    want = sorted(rt.annotate_rows(recs, hit, *TAB7), key=key_of)          # stable: equal keys in stream order
    ms = check_stream(rule, got, b"".join(want))
    assert ss["rounds"] == 2 and ss["records"] == 700 and st["payload_bytes"] == sum(len(w) for w in want)
    assert (status, idx) == bai.expected(l_ref, b"".join(want), [len(m) for m in ms], 0) and status == bai.OK


def test_index_of_the_annotated_stream(rule):
    import torch
    recs, hit = sorted_case(600)
    order = sorted(range(600), key=lambda i: key_of(recs[i]))
    recs, hit = [recs[i] for i in order], hit[order]
    hit[::5] = -1
    l_ref = [100_000] * 3
    bo = eng.Bamout(batch_capacity=600)
    bo.index_enable(l_ref)
    bo.annotate_enable(*TAB7)
    raw, off = tensors(recs)
    bo.run(raw, off, torch.from_numpy(hit).cuda())
    bo.wait_kernels()
    got = bo.finish()
    status, idx, info = bo.index_finish(777)
    bo.close()
    want = expected(TAB7, recs, hit)
    ms = check_stream(rule, got, want)
    assert (status, idx) == bai.expected(l_ref, want, [len(m) for m in ms], 777) and status == bai.OK and info["entries"] == int((hit >= 0).sum())


def test_levels_inflate_to_the_same_stream(rule):
    recs = mixed_records(13, 400) + [rec_of_len(2 * P + 5, 2)]
    hit = pattern("alternating", len(recs))
    hit[-1] = 3
    outs = [run_annotated(rule, TAB7, recs, hit, level=lv) for lv in (0, 1, 6)]
    assert outs[0][1] == outs[1][1] == outs[2][1] and len({len(o[0]) for o in outs}) == 3
    assert bm.split_members(outs[2][0]) == rule.members(outs[2][1])        # level 6 set by hand is the default's members


# ---- 2. without the call nothing changes; state and argument checks

def test_without_annotate_enable_the_stream_is_the_plain_one(rule):
    import torch
    recs = mixed_records(14, 2 * TILE + 1) + [rec_of_len(3 * P + 17, 1)]
    hit = pattern("alternating", len(recs))
    hit[-1] = 0
    bo = eng.Bamout(batch_capacity=len(recs))
    raw, off = tensors(recs)
    bo.run(raw, off, torch.from_numpy(hit).cuda())
    bo.wait_kernels()
    got = bo.finish()
    tb = bo.tag_bytes()
    bo.close()
    plain = b"".join(r for r, h in zip(recs, hit) if h >= 0)
    check_stream(rule, got, plain)
    assert tb == 0 and plain != expected(TAB7, recs, hit)


def enable(L, bo, rows, tabs):
    """itx_bamout_annotate_enable over explicit (pool bytes, offsets) per table"""
    args = []
    keep = []
    for pool, off in tabs:
        o = np.asarray(off, np.uint64)
        keep.append(o)
        args += [pool, o.ctypes.data, len(off) - 1]
    return L.itx_bamout_annotate_enable(bo._h, rows.ctypes.data if rows is not None else None, 0 if rows is None else len(rows), *args)


def test_state_and_argument_checks(rule):
    import torch
    L = eng.load()
    rows = np.zeros(3, eng.ROW_DTYPE)
    rows["rep"], rows["cla"], rows["fam"] = [0, 1, 0], [0, 0, 0], [1, 0, 1]
    good = [(b"abcd", [0, 2, 4]), (b"xy", [0, 2]), (b"pqr", [0, 1, 3])]
    bo = eng.Bamout(batch_capacity=64)
    # bad arguments: nothing is taken, the object stays un-annotated
    assert L.itx_bamout_annotate_enable(bo._h, rows.ctypes.data, 3, None, None, 0, None, None, 0, None, None, 0) == -1
    assert enable(L, bo, rows, [(b"abcd", [0, 3, 2]), good[1], good[2]]) == -1 and b"ascend" in L.itx_last_error()
    for k in ("rep", "cla", "fam"):
        bad = rows.copy()
        bad[2][k] = 2 if k != "cla" else 1
        assert enable(L, bo, bad, good) == -1 and b"row 2" in L.itx_last_error(), k
    big = b"x" * 65536
    assert enable(L, bo, rows, [(big + b"ab", [0, 65536, 65538]), good[1], good[2]]) == -6      # ITX_E_LIMIT: a name of 2^16 bytes
    assert enable(L, bo, rows, [(big, [0, 65535, 65536]), good[1], good[2]]) == 0               # 65 535 bytes: taken
    assert enable(L, bo, rows, good) == -5 and b"twice" in L.itx_last_error()
    # a chosen row equal to n_rows: refused, nothing appended, the next good batch works
    recs = mixed_records(15, 10)
    raw, off = tensors(recs)
    hits = torch.from_numpy(np.array([0, 1, 2, 3, -1, 0, 0, 0, 0, 0], np.int32)).cuda()
    assert L.itx_bamout_run(bo._h, C.c_void_p(raw.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(hits.data_ptr()), 10, None) == -1
    assert b"outside" in L.itx_last_error() and bo.stats()["records"] == 0 and bo.stats()["carry"] == 0
    hit = np.array([1, -1, 2, 1, -1, 2, 2, 1, 1, 2], np.int32)
    bo.run(raw, off, torch.from_numpy(hit).cuda())
    bo.wait_kernels()
    got = bo.finish()
    bo.close()
    tab = (rows, [big[:65535], b"x"], [b"xy"], [b"p", b"qr"])
    check_stream(rule, got, expected(tab, recs, hit))
    # after the first batch
    bo = eng.Bamout(batch_capacity=64)
    bo.append_host(recs[0])
    assert enable(L, bo, rows, good) == -5 and b"begun" in L.itx_last_error()
    bo.finish()
    bo.close()


# ---- 3. the command

BAM = "out_%s.iteres.bam"


def oracle_rows(root, case, aln, opts):
    """the row the CPU oracle chooses per record of <root>/<case>/in/<aln> (-1: none), and the table model the rows index"""
    saved = gc.GOLDEN
    gc.GOLDEN = str(root)
    try:
        p = gc.parse_opts("filter", list(opts))
        tm = gc.build_table_model(case, p["filter_field"], p["filter_name"])
        header, rd = gc.load_reads(case, aln)
    finally:
        gc.GOLDEN = saved
    ot = orc.OracleTable(tm.chrom_size, tm.rep_len, len(tm.fams), len(tm.clas))
    st = ot.add_rows(tm.chrom, [r["start"] for r in tm.rows], [r["end"] for r in tm.rows], [r["cons_start"] for r in tm.rows], [r["cons_end"] for r in tm.rows],
                     tm.rep, tm.fam, tm.cla)
    assert (st == np.arange(len(tm.rows))).all()

    def run_oracle(skip):
        return ot.run(p, gc.tid_map(header, tm, p["add_chr"]), rd["tid"], rd["pos"], rd["tmpend"], rd["mapq"], rd["flag"], rd["mpos"], rd["isize"], skip=skip)
    dup, veto = gc.side_masks(p, tm, header, rd, ot, run_oracle)
    return run_oracle(dup)["hit_row"], tm, header


def tag_line(err):
    m = re.search(r"batches by the host route, (\d+) tag bytes appended", err)
    assert m, err[-1500:]
    return int(m.group(1))


def check_command(exe, root, case, d, aln, tmp_path, sel, extra, env=None):
    """`sel` (one of -n / -c / -f and its name, or -C ...) with `extra` options: -b -a against the same command without -a"""
    env = dict({"ITX_HOST_NAMES": "0"}, **(env or {}))
    sub = sel[sel.index(next(o for o in sel if o in ("-n", "-c", "-f"))) + 1]
    opts = tuple(sel) + tuple(extra)
    with_a = run_filter(exe, d, str(tmp_path / "a"), ("-b", "-a") + opts, aln, env)
    plain = run_filter(exe, d, str(tmp_path / "b"), ("-b",) + opts, aln, env)
    bam = BAM % sub
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    for fn in os.listdir(tmp_path / "b"):                                  # .loci, .reportloci (and the read lists) do not move
        if not fn.startswith(bam):
            assert filecmp.cmp(tmp_path / "a" / fn, tmp_path / "b" / fn, shallow=False), fn
    head_a, recs_a = raw_records(tmp_path / "a" / bam)
    head_b, recs_b = raw_records(tmp_path / "b" / bam)
    assert head_a == head_b and len(recs_a) == len(recs_b) > 5
    stripped = [rt.strip(r) for r in recs_a]
    assert [s[0] for s in stripped] == recs_b                               # 1. the tags off: the file without -a (sorted under -s)
    # 2. the tags are those of the row the oracle chooses for that read
    hit_row, tm, header = oracle_rows(root, case, os.path.basename(str(aln)), [o for o in opts if o not in ("-s", "-i", "-l", "0", "1")])
    _, in_recs = raw_records(aln)
    assert len(in_recs) == len(hit_row)

    def values(h):
        w = tm.rows[int(h)]
        return w["name"].encode(), w["cname"].encode(), w["fname"].encode(), int(w["start"]), int(w["end"])
    want = [(r, values(h)) for r, h in zip(in_recs, hit_row) if h >= 0]
    assert len(want) == len(recs_a)
    if "-s" not in opts:                                                    # in file order: record by record
        assert stripped == want
    else:                                                                   # sorted: the same (record, tags) pairs
        assert collections.Counter(stripped) == collections.Counter(want)
    # 3. grouped by (reference, ZS, ZE, ZN) the records give the readsCount column of the command's own .loci file, line for line
    if "-t" not in opts:
        add_chr = "-C" in opts
        groups = collections.Counter()
        for rec, (zn, zc, zf, zs, ze) in stripped:
            tid, = struct.unpack_from("<i", rec, 4)
            groups[(gc.rename_chr(header[tid][0], add_chr), zs, ze, zn.decode())] += 1
        _, lrows = refio.parse_loci(tmp_path / "a" / (bam[:-4] + ".loci"))
        loci = {(r[0], int(r[1]), int(r[2]), r[4]): int(r[7]) for r in lrows}
        assert len(loci) == len(lrows) and dict(groups) == loci
    # 4. the timing line counts the tag bytes; the plain run's line is the one it was
    assert tag_line(with_a.stderr) == sum(len(a) - len(b) for a, b in zip(recs_a, recs_b)) and "tag bytes" not in plain.stderr
    assert routes(with_a.stderr)["records"] == len(recs_a) and routes(with_a.stderr)["payload"] == sum(len(r) for r in recs_a)
    data = open(tmp_path / "a" / bam, "rb").read()
    assert data.endswith(bm.EOF_MARKER)
    if "-i" in opts:                                                        # 5. the index is that of the annotated file
        status, idx = bai.expected_for_file(data)
        mine = open(tmp_path / "a" / (bam + ".bai"), "rb").read()
        assert status == bai.OK and mine == idx
        if refbam.present:
            refbam.check_index(tmp_path / "a" / bam, mine)
            assert refbam.check_fetch(tmp_path / "a" / bam, mine, refbam.edge_regions(tmp_path / "a" / bam)) > 5
    if refbam.present:                                                      # 6. the reference's BAM library reads what was appended
        lines_a, lines_b = refbam.view(tmp_path / "a" / bam)[1], refbam.view(tmp_path / "b" / bam)[1]
        assert len(lines_a) == len(lines_b) == len(stripped)
        for la, lb, (_, (zn, zc, zf, zs, ze)) in zip(lines_a, lines_b, stripped):
            assert la == lb + b"\tZN:Z:%s\tZC:Z:%s\tZF:Z:%s\tZS:i:%d\tZE:i:%d" % (zn, zc, zf, zs, ze)
    if os.path.exists(REF) and "-s" not in opts:                            # 7. the reference counts over it what it counts over the input
        ref_opts = [o for o in opts if o not in ("-i", "-l", "0", "1", "-t", "3")]
        run_filter(exe, d, str(tmp_path / "ref_in"), ref_opts, aln, binary=REF)
        run_filter(exe, d, str(tmp_path / "ref_out"), ref_opts, tmp_path / "a" / bam, binary=REF)
        name = bam[:-4] + ".loci"
        assert [r[:8] for r in refio.parse_loci(tmp_path / "ref_in" / name)[1]] == [r[:8] for r in refio.parse_loci(tmp_path / "ref_out" / name)[1]]
    return with_a


PILE_RUNS = {"paired_c": ("paired.bam", "-c", ()), "paired_c_si": ("paired.bam", "-c", ("-s", "-i")), "single_n_l0": ("single.bam", "-n", ("-l", "0")),
             "single_n_l1_i": ("single.bam", "-n", ("-l", "1", "-i")), "paired_c_r": ("paired.bam", "-c", ("-r",)), "paired_c_R": ("paired.bam", "-c", ("-R",)),
             "paired_c_T": ("paired.bam", "-c", ("-T",))}


@pytest.mark.parametrize("which", list(PILE_RUNS))
def test_command(which, pile, exe, tmp_path):
    root, d, big, name = pile
    aln, flt, extra = PILE_RUNS[which]
    check_command(exe, root, "bamout", d, d / aln, tmp_path, (flt, big if flt == "-c" else name), extra)


@pytest.mark.parametrize("extra", [(), ("-s", "-i")], ids=["plain", "sorted_indexed"])
def test_command_both_routes_in_one_file(extra, pile, exe, tmp_path):
    """mixed.bam: the windows with chrU records take the host route, whose records the host annotates (host/out_bam.c)"""
    root, d, big, name = pile
    with_a = check_command(exe, root, "bamout", d, d / "mixed.bam", tmp_path, ("-c", big), extra)
    r = routes(with_a.stderr)
    assert r["dev"] >= 2 and r["host"] >= 1, r


GOLDEN_RUNS = {"sidechan": (("-c", None), ("-R",)), "mid": (("-n", "Rep1"), ("-s", "-i")), "quirks": (("-f", "L1"), ("-l", "1")), "addchr": (("-C", "-c", None), ("-i",))}


@pytest.mark.parametrize("case", list(GOLDEN_RUNS))
def test_command_on_the_golden_inputs(case, exe, tmp_path):
    sel, extra = GOLDEN_RUNS[case]
    src = os.path.join(gc.GOLDEN, case, "in")
    aln = refio.materialise(src, "reads.bam", str(tmp_path))

    class D:                                                               # run_filter joins the three table files onto d
        def __truediv__(self, name):
            return refio.materialise(src, name, str(tmp_path))
    if None in sel:                                                         # the class with the most rows
        tm = gc.build_table_model(case)
        sel = tuple(tm.clas[int(np.bincount(tm.cla).argmax())] if o is None else o for o in sel)
    check_command(exe, gc.GOLDEN, case, D(), aln, tmp_path, sel, extra)
