"""GPU: the levels of the BAM's members (`filter -b -l`; include/iteres_amd.h itx_bamout_set_level, csrc/itx_bamout_members.hip
k_bo_member_stored / k_bo_member_fast over csrc/itx_bgzflevels.h).
1. through engine.Bamout, for levels 0 and 1: the device's member sequence equals the host build of the same headers
   (tests/bgzflevels_host.cpp) over payload-sized slices of the expected stream, in the shapes test_gpu_bamout.py uses for the
   default level; level 6 by set_level is the object that never called it; state and argument checks;
2. with the index and with the sort: the records, the index's restatement (tests/baicase.py) and the members at both levels;
3. the command: -l 0 and -l 1 decode to the records of -b, -l 6 is -b's file, the other outputs do not change, -b -s -i -l 1 on
   shuffled input through the index, the host route in the middle, and ITX_TIMING's line."""
import filecmp
import os
import re
import struct

import numpy as np
import pytest

import baicase as bai
import bgzflevelshost as bl
import bgzfmemberhost as bm
from iteres_amd import engine as eng
from test_gpu_bamidx import regions
from test_gpu_bamout import (TILE, exe, gather, hit_pattern, mixed_records, pile, raw_records, rec_of_len, routes, run_filter,   # noqa: F401  (fixtures too)
                             tensors)
from test_gpu_bamsort import key_of, shuffled_bam, split_records, srec
from test_gpu_bed import HEADER, window

pytestmark = pytest.mark.gpu

P = bai.PAYLOAD
LEVELS = (0, 1)


@pytest.fixture(scope="module")
def lv(tmp_path_factory):
    return bl.LevelRule(tmp_path_factory.mktemp("bamout_levels_rule"))


@pytest.fixture(scope="module")
def inf():
    h = eng.Inflater()
    yield h
    h.close()


def check_stream(lv, got, want, level):
    """got: every member the object handed out; want: the gathered records. The members' bytes are the host build's."""
    ms = bm.split_members(got)
    assert ms == lv.members(want, level)
    assert b"".join(bm.check_member(m) for m in ms) == want
    assert all(len(m) <= P + 31 for m in ms)
    if level == 0:
        assert len(got) == len(want) + 31 * len(ms)
    return ms


def run_once(lv, level, recs, rows, cap=None):
    import torch
    bo = eng.Bamout(batch_capacity=cap or max(len(recs), 1))
    try:
        bo.set_level(level)
        assert bo.level() == level
        if recs:
            raw, off = tensors(recs)
            bo.run(raw, off, torch.from_numpy(np.asarray(rows, np.int32)).cuda())
            bo.wait_kernels()
        got = bo.finish()
        st = bo.stats()
    finally:
        bo.close()
    ms = check_stream(lv, got, gather(recs, rows), level)
    assert st["members"] == len(ms) and st["out_bytes"] == len(got)
    return got, st


# ---- 1. the member sequence

@pytest.mark.parametrize("level", LEVELS)
def test_no_records_and_one_record(lv, level):
    got, st = run_once(lv, level, [], [])
    assert got == b"" and st["members"] == 0
    got, st = run_once(lv, level, [rec_of_len(77)], [3])
    assert st["records"] == 1 and st["members"] == 1 and (len(got) == 77 + 31 if level == 0 else len(got) <= 77 + 31)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_tile_boundaries(lv, n, level):
    recs = mixed_records(n, n)
    for kind in ("all", "third"):
        rows = hit_pattern(kind, n)
        got, st = run_once(lv, level, recs, rows)
        assert st["records"] == int((rows >= 0).sum()) and st["member_ms"] > 0


@pytest.mark.parametrize("level", LEVELS)
def test_a_record_longer_than_three_payloads(lv, level):
    recs = mixed_records(9, 40) + [rec_of_len(3 * P + 17, 1)] + mixed_records(10, 300)
    rows = np.where(np.arange(len(recs)) % 2 == 0, 1, -1).astype(np.int32)
    got, st = run_once(lv, level, recs, rows)
    assert st["members"] >= 4


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_totals_around_whole_payloads(lv, delta, level):
    for k in (1, 3):
        total = k * P + delta
        recs, left, i = [], total, 0
        while left:
            L = 200 + i % 57 if left >= 200 + i % 57 + 48 else left
            recs.append(rec_of_len(L, i))
            left -= L
            i += 1
        got, st = run_once(lv, level, recs, [7] * len(recs))
        ms = bm.split_members(got)
        assert st["payload_bytes"] == total and len(ms) == k + (delta > 0)
        assert struct.unpack_from("<I", ms[-1], len(ms[-1]) - 4)[0] == (total - 1) % P + 1


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("tail", [0, 1])
def test_finish_tail(lv, tail, level):
    import torch
    recs = [rec_of_len(P // 4, i) for i in range(8)] + ([rec_of_len(48, 9)] if tail else [])
    bo = eng.Bamout(batch_capacity=64)
    bo.set_level(level)
    raw, off = tensors(recs)
    bo.run(raw, off, torch.zeros(len(recs), dtype=torch.int32, device="cuda:0"))
    assert len(bm.split_members(bytes(bo.out))) == 2 and bo.stats()["carry"] == (48 if tail else 0)
    if tail:
        bo.append_host(rec_of_len(P - 47, 3))
        assert bo.stats()["carry"] == 1
    got = bo.finish()
    bo.close()
    ms = check_stream(lv, got, b"".join(recs) + (rec_of_len(P - 47, 3) if tail else b""), level)
    assert len(ms) == (4 if tail else 2)


@pytest.mark.parametrize("level", LEVELS)
def test_three_window_calls_with_host_appends_between(lv, inf, level):
    """70 001 records of one parsed window in three calls; whole records from the host before, between and after them"""
    import torch
    n = 70_001
    recs = [rec_of_len(48 + (i * 7) % 90, i) for i in range(n)]
    rows = hit_pattern("third", n)
    rows[-1] = 2
    assert window(inf, bc_bam(recs)) == n
    hits = torch.from_numpy(rows).cuda()
    h0, h1, h2 = mixed_records(21, 3), mixed_records(22, 400), [rec_of_len(5000, 4)]
    bo = eng.Bamout(batch_capacity=32768)
    bo.set_level(level)
    bo.append_host(b"".join(h0))
    cuts = [0, 32768, 32768 + 32767, n]
    want = [b"".join(h0)]
    for c in range(3):
        a, b = cuts[c], cuts[c + 1]
        bo.append_window(inf, a, b - a, hits[a:b])
        want.append(gather(recs[a:b], rows[a:b]))
        if c == 0:
            bo.append_host(b"".join(h1))
            want.append(b"".join(h1))
        assert (sum(len(w) for w in want)) % P == bo.stats()["carry"]
    bo.wait_kernels()
    bo.append_host(b"".join(h2))
    want.append(b"".join(h2))
    got = bo.finish()
    st = bo.stats()
    bo.close()
    check_stream(lv, got, b"".join(want), level)
    assert st["batches"] == 3 and st["host_batches"] == 3 and st["carry"] == 0


def bc_bam(recs):
    import bedcase as bc
    return bc.bam_bytes(HEADER, recs)


def test_set_level_6_is_the_object_that_never_called_it():
    import torch
    recs = mixed_records(5, 700)
    raw, off = tensors(recs)
    rows = torch.from_numpy(hit_pattern("third", 700)).cuda()
    out = []
    for call in (False, True):
        bo = eng.Bamout(batch_capacity=1024)
        assert bo.level() == 6
        if call:
            bo.set_level(6)
        bo.run(raw, off, rows)
        out.append(bo.finish())
        assert bo.level() == 6
        bo.close()
    assert out[0] == out[1] and len(bm.split_members(out[0])) >= 3


def test_argument_and_state_checks(lv):
    import torch
    L = eng.load()
    assert L.itx_bamout_set_level(None, 1) == -1 and L.itx_bamout_get_level(None) == -1
    recs = mixed_records(6, 300)
    raw, off = tensors(recs)
    rows = torch.zeros(300, dtype=torch.int32, device="cuda:0")
    bo = eng.Bamout(batch_capacity=512)
    for bad in (2, -1, 5, 7, 9):
        assert L.itx_bamout_set_level(bo._h, bad) == -1 and b"level" in L.itx_last_error()       # ITX_E_ARG, nothing changes
    assert bo.level() == 6
    assert L.itx_bamout_set_level(bo._h, 1) == 0 and bo.level() == 1
    assert L.itx_bamout_set_level(bo._h, 0) == -5 and b"twice" in L.itx_last_error() and bo.level() == 1
    assert L.itx_bamout_set_level(bo._h, 2) == -1 and bo.level() == 1                              # the argument is checked first
    bo.run(raw, off, rows)                                                                          # a later run is unaffected
    check_stream(lv, bo.finish(), b"".join(recs), 1)
    bo.close()
    late = eng.Bamout(batch_capacity=512)
    late.run(raw, off, rows)
    assert L.itx_bamout_set_level(late._h, 1) == -5 and b"begun" in L.itx_last_error() and late.level() == 6
    got = late.finish()
    assert L.itx_bamout_set_level(late._h, 0) == -5
    late.close()
    assert bm.split_members(got) == bm.MemberRule(lv_dir(lv)).members(b"".join(recs))              # the default level's members
    host_first = eng.Bamout(batch_capacity=16)
    host_first.append_host(recs[0])
    assert L.itx_bamout_set_level(host_first._h, 0) == -5
    host_first.finish()
    host_first.close()


def lv_dir(lv):
    return os.path.dirname(lv.L._name)


# ---- 2. with the index and with the sort

def drive(level, l_ref, steps, first, cap, sort):
    """steps: ("run", records, rows) or ("host", records) -> (members, counted records in input order, status, index bytes)"""
    import torch
    bo = eng.Bamout(batch_capacity=cap)
    try:
        bo.set_level(level)
        if sort:
            bo.sort_enable()
        bo.index_enable(l_ref)
        counted = []
        for s in steps:
            if s[0] == "run":
                raw, off = tensors(s[1])
                bo.run(raw, off, torch.from_numpy(np.asarray(s[2], np.int32)).cuda())
                bo.wait_kernels()
                counted += [r for r, h in zip(s[1], s[2]) if h >= 0]
            else:
                bo.append_host(b"".join(s[1]))
                counted += s[1]
        got = bo.sort_all() if sort else bo.finish()
        status, idx, info = bo.index_finish(first)
        return got, counted, status, idx
    finally:
        bo.close()


def test_index_at_both_levels(lv):
    """the index's bytes are the restatement's over the members of each level: their sizes differ, so every virtual offset does"""
    l_ref = [5_000_000, 1000, 3_000_000]
    recs = [srec(0 if i < 500 else 2, 100 + 37 * i, name=b"n%d" % i, L=60 + (i * 7) % 90) for i in range(900)]
    rows = [1 if i % 3 else -1 for i in range(600)]
    steps = [("run", recs[:600], rows), ("host", recs[600:])]
    seen = {}
    for level in LEVELS:
        got, counted, status, idx = drive(level, l_ref, steps, 333, 600, False)
        stream = b"".join(counted)
        ms = check_stream(lv, got, stream, level)
        assert len(ms) >= 4 and status == bai.OK
        assert (status, idx) == bai.expected(l_ref, stream, [len(m) for m in ms], 333)
        seen[level] = ([len(m) for m in ms], idx)
    assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", ["descending257", "boundary", "tail"])
def test_sort_at_both_levels(lv, level, case):
    if case == "descending257":
        recs = [srec(1 - i // 200, 90_000 - 13 * i, 16 * (i % 2), b"d%d" % i, L=60 + i % 70) for i in range(257)]
        l_ref = [100_000, 100_000]
    else:
        recs = ([srec(1, 9, L=50)] if case == "tail" else []) + [srec(1, 5, L=P), srec(0, 20, L=P // 2), srec(0, 10, L=P // 2)]
        l_ref = [1000, 1000]
    steps = [("host", recs[:1]), ("run", recs[1:], [0] * (len(recs) - 1))]
    got, counted, status, idx = drive(level, l_ref, steps, 28, max(len(recs), 1), True)
    want = sorted(counted, key=key_of)
    assert want != counted
    stream = b"".join(want)
    ms = check_stream(lv, got, stream, level)
    assert split_records(b"".join(bm.check_member(m) for m in ms)) == want
    assert status == bai.OK and (status, idx) == bai.expected(l_ref, stream, [len(m) for m in ms], 28)
    if case != "descending257":
        assert len(ms) == 2 + (case == "tail") and struct.unpack_from("<I", ms[-1], len(ms[-1]) - 4)[0] == (50 if case == "tail" else P)


# ---- 3. the command

BAM = "out_ALL.iteres.bam"


def level_line(err):
    """ITX_TIMING's `bam out:` line, whole"""
    lines = [ln for ln in err.splitlines() if ln.startswith("[itx timing] bam out:")]
    assert len(lines) == 1, err[-1500:]
    return lines[0]


PARENT_LINE = (r"\[itx timing\] bam out: \d+ records, \d+ payload bytes, \d+ members \(\d+ bytes\), [0-9.]+ ms in the gather kernels, [0-9.]+ ms in the member "
               r"kernels, host waited [0-9.]+ s, \d+ batches gathered on the device, \d+ batches by the host route")


def test_command_levels(pile, exe, tmp_path):
    root, d, big, name = pile
    env = {"ITX_HOST_NAMES": "0"}
    runs = {k: run_filter(exe, d, str(tmp_path / k), opts, d / "paired.bam", env)
            for k, opts in (("b", ("-b", "-r")), ("l0", ("-b", "-r", "-l", "0")), ("l1", ("-b", "-l", "1", "-r")), ("l6", ("-b", "-r", "-l", "6")))}
    names = sorted(os.listdir(tmp_path / "b"))
    assert BAM in names and any(n.endswith(".loci") for n in names) and any(n.endswith(".reportloci") for n in names)
    head, recs = raw_records(tmp_path / "b" / BAM)
    assert len(recs) > 200
    for k in ("l0", "l1", "l6"):
        assert sorted(os.listdir(tmp_path / k)) == names
        for fn in names:                                                    # .loci, .reportloci and the read lists: byte-identical
            if fn != BAM:
                assert filecmp.cmp(tmp_path / k / fn, tmp_path / "b" / fn, shallow=False), (k, fn)
        assert raw_records(tmp_path / k / BAM) == (head, recs)
        data = open(tmp_path / k / BAM, "rb").read()
        assert data.endswith(bm.EOF_MARKER)
        for m in bm.split_members(data):
            bm.check_member(m)
    assert filecmp.cmp(tmp_path / "l6" / BAM, tmp_path / "b" / BAM, shallow=False)          # -l 6 writes the file -b writes
    size = {k: os.path.getsize(tmp_path / k / BAM) for k in runs}
    assert size["l0"] > size["l1"] > size["b"]                             # stored; cut matches of at most 32 bytes; the default
    # the timing line: `, level <n>` ends it when -l was given, and only then
    for k, n in (("l0", 0), ("l1", 1), ("l6", 6)):
        assert re.fullmatch(PARENT_LINE + ", level %d" % n, level_line(runs[k].stderr)), level_line(runs[k].stderr)
    assert re.fullmatch(PARENT_LINE, level_line(runs["b"].stderr)), level_line(runs["b"].stderr)
    assert routes(runs["l1"].stderr)["records"] == len(recs) and routes(runs["l1"].stderr)["out_bytes"] < routes(runs["l0"].stderr)["out_bytes"]


@pytest.mark.parametrize("opts", [("-R",), ("-T",), ("-D",), ("-C",), ("-c", "CLASS")], ids=["R", "T", "D", "C", "c"])
def test_command_level_1_with_other_options(opts, pile, exe, tmp_path):
    root, d, big, name = pile
    opts = tuple(big if o == "CLASS" else o for o in opts)
    sub = big if "-c" in opts else "ALL"
    run_filter(exe, d, str(tmp_path / "b"), ("-b",) + opts, d / "paired.bam")
    run_filter(exe, d, str(tmp_path / "l1"), ("-b", "-l", "1") + opts, d / "paired.bam")
    bam = f"out_{sub}.iteres.bam"
    assert sorted(os.listdir(tmp_path / "b")) == sorted(os.listdir(tmp_path / "l1"))
    for fn in os.listdir(tmp_path / "b"):
        if fn != bam:
            assert filecmp.cmp(tmp_path / "l1" / fn, tmp_path / "b" / fn, shallow=False), fn
    assert raw_records(tmp_path / "l1" / bam) == raw_records(tmp_path / "b" / bam)


def fetch_equivalence(path, n_regions=150):
    """the emitted file and its .bai: the index is the restatement's, and what it fetches is what a walk over every record finds"""
    data = open(path, "rb").read()
    l_ref, stream, sizes, first, raw, ustart = bai.split_bam(data)
    status, want = bai.expected(l_ref, stream, sizes, first)
    idx = open(str(path) + ".bai", "rb").read()
    assert status == bai.OK and idx == want
    parsed = bai.parse_bai(idx)
    at = len(raw) - len(stream)
    recs = bai.records_of(stream)
    hits = 0
    for tid, beg, end in regions(l_ref, recs, n=n_regions):
        found = bai.fetch(parsed, raw, ustart, tid, beg, end)
        assert found == bai.linear_scan(raw, at, tid, beg, end), (tid, beg, end)
        hits += bool(found)
    assert hits >= n_regions // 4, hits
    return len(recs)


def test_command_sorted_and_indexed_at_level_1_with_the_host_route_in_the_middle(pile, exe, tmp_path):
    """mixed.bam shuffled, its chrU records (whose windows take the host route) one run in the middle: -b -s -i -l 1"""
    root, d, big, name = pile
    head, recs = raw_records(d / "mixed.bam")
    shuffled_bam(tmp_path / "shuffled.bam", head, recs, 5, keep_together=lambda r: key_of(r)[0] == 1)
    srt = run_filter(exe, d, str(tmp_path / "l1"), ("-b", "-s", "-i", "-l", "1"), tmp_path / "shuffled.bam", {"ITX_HOST_NAMES": "0"})
    run_filter(exe, d, str(tmp_path / "b"), ("-b",), tmp_path / "shuffled.bam", {"ITX_HOST_NAMES": "0"})
    rt = routes(srt.stderr)
    assert rt["dev"] >= 2 and rt["host"] >= 1, rt
    _, recs_b = raw_records(tmp_path / "b" / BAM)
    _, recs_s = raw_records(tmp_path / "l1" / BAM)
    assert recs_s == sorted(recs_b, key=key_of) != recs_b and len(recs_s) == rt["records"] > 200
    assert fetch_equivalence(tmp_path / "l1" / BAM) == len(recs_s)
    assert level_line(srt.stderr).endswith("final kernels, level 1")
    for fn in os.listdir(tmp_path / "b"):
        if fn != BAM:
            assert filecmp.cmp(tmp_path / "l1" / fn, tmp_path / "b" / fn, shallow=False), fn


def test_command_host_route_in_the_middle_at_level_1(pile, exe, tmp_path):
    """the windows of mixed.bam's chrU records take the host route between device windows: one ordered stream at level 1, indexed"""
    root, d, big, name = pile
    with_l = run_filter(exe, d, str(tmp_path / "l1"), ("-b", "-i", "-l", "1"), d / "mixed.bam")
    run_filter(exe, d, str(tmp_path / "b"), ("-b",), d / "mixed.bam")
    rt = routes(with_l.stderr)
    assert rt["dev"] >= 2 and rt["host"] >= 1, rt
    assert raw_records(tmp_path / "l1" / BAM) == raw_records(tmp_path / "b" / BAM)
    fetch_equivalence(tmp_path / "l1" / BAM)
