"""GPU: the .bai index of `filter -b -i` built on the device beside the BAM (include/iteres_amd.h itx_bamout_index_*,
csrc/itx_bamidx.hip). Every case compares the index's bytes with the Python restatement of the rule (tests/baicase.py) applied to
the stream and to the members the object handed out:
1. the ABI: shapes around the record tile (255 / 256 / 257), around payload boundaries, chunks that merge and chunks that do not, a
   spliced record over 3000 windows, references without records, 70 001 records over three `run` calls with host appends between
   them and a pool that grows, finish with and without a tail;
2. when no index can be made: the status, no bytes, and the members unchanged;
3. argument and state checks;
4. fetch equivalence: the records fetched through OUR index by the restatement's independent reader equal a linear scan's;
5. the command: the .bai beside the .bam equals the restatement's for the emitted file, every other output equals a run without -i."""
import ctypes as C
import filecmp
import os
import re

import numpy as np
import pytest

import baicase as bai
import baishapes as shapes
import goldencase as gc
import refio
from iteres_amd import engine as eng, synth

pytestmark = pytest.mark.gpu

from baishapes import M, P, all_hit, big_case, rec       # the case inputs: shared with tests/test_gpu_bam_vs_reference.py


def tensors(recs):
    import torch
    off = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint32)
    raw = torch.from_numpy(np.frombuffer(b"".join(recs) + bytes(64), np.uint8).copy()).cuda()
    return raw, torch.from_numpy(off.view(np.int32).copy()).cuda()


def drive(l_ref, steps, first=0, cap=None, index=True):
    """steps: ("run", records, rows) or ("host", records). -> (members, the counted stream, status, index bytes, counters)"""
    import torch
    bo = eng.Bamout(batch_capacity=cap or max([len(s[1]) for s in steps if s[0] == "run"] + [1]))
    try:
        if index:
            bo.index_enable(l_ref)
        stream = []
        for s in steps:
            if s[0] == "run":
                raw, off = tensors(s[1])
                bo.run(raw, off, torch.from_numpy(np.asarray(s[2], np.int32)).cuda())
                bo.wait_kernels()
                stream += [r for r, h in zip(s[1], s[2]) if h >= 0]
            else:
                bo.append_host(b"".join(s[1]))
                stream += s[1]
        got = bo.finish()
        status, idx, info = bo.index_finish(first) if index else (None, None, None)
        return got, b"".join(stream), status, idx, info
    finally:
        bo.close()


def check(l_ref, steps, first=0, cap=None, plain=False):
    got, stream, status, idx, info = drive(l_ref, steps, first, cap)
    sizes = [size for off, size, isize in bai.member_walk(got)]
    want_status, want = bai.expected(l_ref, stream, sizes, first)
    assert status == want_status
    assert idx == want
    assert info["entries"] == len(bai.records_of(stream))
    if plain:                                                              # the members are the same with and without an index
        assert drive(l_ref, steps, first, cap, index=False)[0] == got
    return got, stream, idx, info


# ---- 1. shapes

def test_no_records_three_references():
    got, stream, idx, info = check([1000, 0, 5_000_000], [], first=77)
    assert got == b"" and idx == b"BAI\1" + (3).to_bytes(4, "little") + bytes(3 * 8) + bytes(8) and info["chunks"] == 0


def test_one_record():
    got, stream, idx, info = check([100_000], [("run", [rec(0, 20_000)], [4])], first=1234, plain=True)
    r, = bai.parse_bai(idx)
    assert r["bins"] == {4682: [(1234 << 16, 1234 << 16 | len(stream))]} and r["lin"] == [0, 1234 << 16] and info["chunks"] == 1


def test_records_that_are_not_counted_leave_no_trace():
    recs = [rec(0, 100 + i) for i in range(40)]
    rows = [-1] * 40
    got, stream, idx, info = check([100_000], [("run", recs, rows)], first=9)
    assert got == b"" and info["entries"] == 0 and bai.parse_bai(idx)[0] == {"bins": {}, "meta": None, "lin": []}


@pytest.mark.parametrize("hit", ["all", "third"])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_tile_boundaries(n, hit):
    """records on both sides of a 16 KiB window and of a 128 KiB bin boundary, so that chunks start inside a tile and at its edge"""
    check(*shapes.tile_boundaries(n, hit), first=4096, plain=True)


def test_a_record_starts_on_the_last_byte_of_a_payload():
    got, stream, idx, info = check(*shapes.last_byte_of_a_payload(), first=500)
    chunks = bai.parse_bai(idx)[0]["bins"][4681]
    assert chunks[0][0] == 500 << 16 and len(bai.member_walk(got)) == 3


@pytest.mark.parametrize("tail", [0, 1])
def test_a_record_ends_exactly_on_a_payload_boundary(tail):
    """without a tail the last chunk ends where whatever follows the members begins; finish with and without a tail member"""
    got, stream, idx, info = check(*shapes.ends_on_a_payload_boundary(tail), first=28, plain=True)
    mem = bai.member_walk(got)
    assert len(mem) == 2 + tail
    r = bai.parse_bai(idx)
    assert r[0]["meta"][:3] == (28 << 16, (28 + mem[0][1]) << 16, 2)
    end = (28 + len(got)) << 16 if not tail else (28 + mem[2][0]) << 16 | 50
    assert r[1]["meta"][:3] == ((28 + mem[0][1]) << 16, end, 1 + tail)


def test_a_record_of_three_payloads_and_17_bytes():
    got, stream, idx, info = check(*shapes.three_payloads_and_17_bytes(), first=3)
    assert len(bai.member_walk(got)) == 4


def test_one_batch_of_more_than_1024_members():
    """more members than the one-workgroup scan of ALL member sizes has threads (k_size_scan, csrc/itx_textpack.h, 1024), so a thread
    sums several sizes: every chunk's virtual offset rests on those sums. 24 000 counted records in one batch, one reference"""
    recs = [rec(0, 1000 + 40 * i, L=300 + i % 101) for i in range(24_000)]
    got, stream, idx, info = check([2_000_000], [("run", recs, all_hit(recs))], first=200, plain=True)
    assert len(bai.member_walk(got)) > 1024


def test_references_without_records_between_references_with_records():
    got, stream, idx, info = check(*shapes.references_without_records(), first=100)
    r = bai.parse_bai(idx)
    assert [x["meta"] is not None for x in r] == [False, True, True, False, True, False, True]
    assert len(r[2]["lin"]) == 1 << 15 and r[2]["lin"][-2] == 0 and len(r[6]["lin"]) == 1 and len(r[4]["lin"]) == 2


@pytest.mark.parametrize("L", [80, P + 900], ids=["one_member", "across_members"])
def test_bin_parent_bin_again(L):
    """bin X, its parent, bin X again: inside one member the two runs of X merge into one chunk; when every record fills more
    than a member, the second run begins in a later member than the first ended in, and they stay two chunks"""
    got, stream, idx, info = check(*shapes.bin_parent_bin_again(L), first=64)
    bins = bai.parse_bai(idx)[0]["bins"]
    assert sorted(bins) == [585, 4681] and len(bins[585]) == 1
    assert len(bins[4681]) == (1 if L < P else 2) and info["chunks"] == (2 if L < P else 3)


def test_a_spliced_record_over_3000_windows():
    got, stream, idx, info = check(*shapes.spliced_over_3000_windows(), first=11)
    lin = bai.parse_bai(idx)[0]["lin"]
    assert len(lin) == (50_001_064 >> 14) + 1 > 3000 and len(set(lin[1:30_000_000 >> 14])) == 1


def regions(l_ref, counted, seed=20, n=300):
    """n regions (tid, beg, end): around counted records, around 16 KiB window boundaries, around bin boundaries of the upper levels"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 3 == 0:
            tid, pos, end = counted[int(rng.integers(len(counted)))][:3]
            beg = max(pos - int(rng.integers(0, 300)), 0)
            fin = beg + int(rng.integers(1, 3000))
        else:
            tid = (0, 2, 3, 1)[int(rng.integers(4))]
            shift = 14 if k % 3 == 1 else (17, 20, 23)[int(rng.integers(3))]
            edge = int(rng.integers(1, max(l_ref[tid] >> shift, 1) + 1)) << shift
            beg = max(edge - int(rng.integers(0, 2000)), 0)
            fin = edge + int(rng.integers(1, 2000))
        fin = min(fin, l_ref[tid])
        if beg >= fin:
            beg = fin - 1
        out.append((tid, beg, fin))
    return out


@pytest.fixture(scope="module")
def big():
    l_ref, steps = big_case()
    first = 3000
    got, stream, idx, info = check(l_ref, steps, first=first, cap=32768, plain=True)
    return l_ref, steps, first, got, stream, idx, info


def test_three_runs_with_host_appends_between_and_a_pool_that_grows(big):
    l_ref, steps, first, got, stream, idx, info = big
    counted = 404 + sum(h >= 0 for s in steps if s[0] == "run" for h in s[2])
    assert 23_000 < counted < 24_000
    assert info["grows"] >= 1 and info["entries"] == counted and info["batch_ms"] > 0 and info["finish_ms"] > 0
    r = bai.parse_bai(idx)
    assert r[1] == {"bins": {}, "meta": None, "lin": []} and sum(x["meta"][2] for x in r if x["meta"]) == info["entries"]
    levels = {sum(b >= f for f in (1, 9, 73, 585, 4681)) for x in r for b in x["bins"]}
    assert levels >= {2, 3, 4, 5}, levels


def test_lifecycle_and_host_record_buffers_that_regrow():
    """an index enabled and destroyed with no call between; then, twice in one process: a host append of one record, whose offsets
    leave room for 1 + 0 + 1024 records, then one of 1500, so that the five buffers of the host route are taken anew under one object;
    the index is the restatement's"""
    bo = eng.Bamout(batch_capacity=16)
    bo.index_enable([100_000])
    bo.close()
    steps = [("host", [rec(0, 100)]), ("host", [rec(0, 200 + 40 * i, L=60 + i % 90) for i in range(1500)])]
    for _ in range(2):
        got, stream, idx, info = check([100_000], steps, first=7)
        assert info["entries"] == 1501 and refio.bgzf_decompress(got) == stream


def test_fetch_equivalence(big):
    l_ref, steps, first, got, stream, idx, info = big
    sizes = [size for off, size, isize in bai.member_walk(got)]
    coff = np.cumsum([0] + sizes)
    ustart = {first + int(coff[k]): min(k * P, len(stream)) for k in range(len(sizes) + 1)}
    parsed = bai.parse_bai(idx)
    hits = 0
    recs = bai.records_of(stream)
    r_tid, r_pos, r_end, r_at, _ = np.array(recs, np.int64).T              # the linear scan: every record against the region
    for tid, beg, end in regions(l_ref, recs):
        found = bai.fetch(parsed, stream, ustart, tid, beg, end)
        assert found == set(r_at[(r_tid == tid) & (r_pos < end) & (r_end > beg)].tolist()), (tid, beg, end)
        hits += bool(found)
    assert hits >= 150, hits


# ---- 2. no index can be made

@pytest.mark.parametrize("kind,status", [("unsorted_pos", bai.UNSORTED), ("unsorted_tid", bai.UNSORTED), ("unsorted_across_batches", bai.UNSORTED),
                                         ("beyond_max", bai.BEYOND_MAX), ("at_max", bai.OK), ("beyond_l_ref", bai.BEYOND_REF), ("no_such_reference", bai.BEYOND_REF)])
def test_no_index(kind, status):
    l_ref = [1 << 30, 100_000]
    a = [rec(0, 100 + i) for i in range(300)]
    b = [rec(1, 100 + i) for i in range(300)]
    steps = {"unsorted_pos": [("run", a[:200] + [rec(0, 50)] + a[200:], [0] * 301)],
             "unsorted_tid": [("run", b + a, [0] * 600)],
             "unsorted_across_batches": [("run", a, [0] * 300), ("host", [rec(0, 398)]), ("run", b, [0] * 300)],
             "beyond_max": [("run", a + [rec(0, (1 << 29) - 10, ((M, 11),))] + b, [0] * 601)],
             "at_max": [("run", a + [rec(0, (1 << 29) - 10, ((M, 10),))] + b, [0] * 601)],
             "beyond_l_ref": [("run", a, [0] * 300), ("host", b + [rec(1, 99_990, ((M, 11),))])],
             "no_such_reference": [("host", a + b + [rec(2, 5)])]}[kind]
    got, stream, st, idx, info = drive(l_ref, steps, first=5)
    sizes = [size for off, size, isize in bai.member_walk(got)]
    assert (st, idx) == bai.expected(l_ref, stream, sizes, 5) and st == status and (idx is None) == (status != bai.OK)
    assert got == drive(l_ref, steps, first=5, index=False)[0] and refio.bgzf_decompress(got) == stream


def test_not_counted_records_do_not_spoil_the_order():
    recs = [rec(0, 500), rec(0, 100), rec(0, 600), rec(3, 1 << 29), rec(0, 700)]
    check([1000], [("run", recs, [0, -1, 0, -1, 0])])


# ---- 3. arguments and states

def test_argument_and_state_checks():
    import torch
    L = eng.load()
    res = eng.BamoutIndexResult()
    lr = (C.c_int32 * 2)(1000, 1000)
    assert L.itx_bamout_index_enable(None, 2, lr) == -1 and L.itx_bamout_index_finish(None, 0, C.byref(res)) == -1
    bo = eng.Bamout(batch_capacity=16)
    assert L.itx_bamout_index_enable(bo._h, -1, lr) == -1 and L.itx_bamout_index_enable(bo._h, 2, None) == -1
    assert L.itx_bamout_index_finish(bo._h, 0, C.byref(res)) == -5 and b"index_enable" in L.itx_last_error()
    assert L.itx_bamout_index_enable(bo._h, 2, lr) == 0
    assert L.itx_bamout_index_enable(bo._h, 2, lr) == -5 and b"twice" in L.itx_last_error()
    assert L.itx_bamout_index_finish(bo._h, 0, C.byref(res)) == -5 and b"not finished" in L.itx_last_error()
    assert L.itx_bamout_index_finish(bo._h, 0, None) == -1
    bo.append_host(rec(0, 5))
    bo.finish()
    assert L.itx_bamout_index_finish(bo._h, 1 << 47, C.byref(res)) == -6
    st, idx, info = bo.index_finish(0)
    assert st == 0 and idx[:4] == b"BAI\1"
    assert L.itx_bamout_index_finish(bo._h, 0, C.byref(res)) == -5 and b"twice" in L.itx_last_error()
    bo.close()
    late = eng.Bamout(batch_capacity=16)                                   # after the first batch
    late.append_host(rec(0, 5))
    assert L.itx_bamout_index_enable(late._h, 2, lr) == -5 and b"begun" in L.itx_last_error()
    late.finish()
    late.close()
    many = eng.Bamout(batch_capacity=16)                                   # 2^16 references: accepted, and no index at the end
    many.index_enable([100] * 65536)
    many.append_host(rec(0, 5))
    many.finish()
    st, idx, info = many.index_finish(0)
    assert (st, idx) == (bai.TOO_MANY_REFS, None) == bai.expected([100] * 65536, b"", [], 0)
    many.close()
    most = eng.Bamout(batch_capacity=16)                                   # 2^16 - 1 references, a record on the last
    raw, off = tensors([rec(65534, 5)])
    most.index_enable([100] * 65535)
    most.run(raw, off, torch.zeros(1, dtype=torch.int32, device="cuda:0"))
    got = most.finish()
    st, idx, info = most.index_finish(0)
    assert (st, idx) == bai.expected([100] * 65535, rec(65534, 5), [len(got)], 0) and st == 0
    most.close()


# ---- 5. the command

from test_gpu_bamout import CHROMS, exe, pile, routes, run_filter          # noqa: E402,F401  (fixtures and the synthetic inputs)


def index_line(err):
    m = re.search(r"; index: (\d+) entries, (\d+) chunks, (\d+) bytes, [0-9.]+ ms in the entry kernels, [0-9.]+ ms in the final kernels", err)
    assert m, err[-1500:]
    return tuple(map(int, m.groups()))


def check_command(exe, d, tmp_path, opts, aln, sub="ALL", env=None):
    """-b -i against -b alone and against the restatement; returns the -b -i run"""
    env = dict({"ITX_HOST_NAMES": "0"}, **(env or {}))
    with_i = run_filter(exe, d, str(tmp_path / "bi"), ("-b", "-i") + tuple(opts), aln, env)
    run_filter(exe, d, str(tmp_path / "b"), ("-b",) + tuple(opts), aln, env)
    bam = f"out_{sub}.iteres.bam"
    assert sorted(os.listdir(tmp_path / "bi")) == sorted(os.listdir(tmp_path / "b") + [bam + ".bai"])
    for fn in os.listdir(tmp_path / "b"):
        assert filecmp.cmp(tmp_path / "bi" / fn, tmp_path / "b" / fn, shallow=False), fn
    data = open(tmp_path / "bi" / bam, "rb").read()
    status, want = bai.expected_for_file(data)
    assert status == bai.OK and open(tmp_path / "bi" / (bam + ".bai"), "rb").read() == want
    entries, chunks, size = index_line(with_i.stderr)
    assert entries == routes(with_i.stderr)["records"] > 20 and size == len(want)
    return with_i


@pytest.mark.parametrize("which", ["single_ALL", "paired_R", "paired_T", "paired_r", "paired_c"])
def test_command(which, pile, exe, tmp_path):
    root, d, big_cla, name = pile
    aln, opts = {"single_ALL": ("single.bam", ()), "paired_R": ("paired.bam", ("-R",)), "paired_T": ("paired.bam", ("-T",)), "paired_r": ("paired.bam", ("-r",)),
                 "paired_c": ("paired.bam", ("-c", big_cla))}[which]
    check_command(exe, d, tmp_path, opts, d / aln, sub=big_cla if "-c" in opts else "ALL")


def test_command_host_route_in_the_middle(pile, exe, tmp_path):
    root, d, big_cla, name = pile
    with_i = check_command(exe, d, tmp_path, (), d / "mixed.bam")
    rt = routes(with_i.stderr)
    assert rt["dev"] >= 2 and rt["host"] >= 1, rt


def test_command_on_a_golden_input(exe, tmp_path):
    src = os.path.join(gc.GOLDEN, "mid", "in")                             # the input of the filter_* runs of that case
    aln = refio.materialise(src, "reads.bam", str(tmp_path))

    class D:                                                               # run_filter joins the three table files onto d
        def __truediv__(self, name):
            return refio.materialise(src, name, str(tmp_path))
    check_command(exe, D(), tmp_path, (), aln)


def test_command_unsorted_input(pile, exe, tmp_path):
    root, d, big_cla, name = pile
    r = synth.make_reads(33, CHROMS, 3000, sorted_=False)
    synth.write_bam(str(tmp_path / "unsorted.bam"), r, block=6000)
    pr = run_filter(exe, d, str(tmp_path / "bi"), ("-b", "-i"), tmp_path / "unsorted.bam")
    run_filter(exe, d, str(tmp_path / "b"), ("-b",), tmp_path / "unsorted.bam")
    assert sorted(os.listdir(tmp_path / "bi")) == sorted(os.listdir(tmp_path / "b")) and "out_ALL.iteres.bam" in os.listdir(tmp_path / "bi")
    for fn in os.listdir(tmp_path / "b"):
        assert filecmp.cmp(tmp_path / "bi" / fn, tmp_path / "b" / fn, shallow=False), fn
    assert "no index is written for out_ALL.iteres.bam: the counted records are not in coordinate order" in pr.stderr
    assert bai.expected_for_file(open(tmp_path / "bi" / "out_ALL.iteres.bam", "rb").read()) == (bai.UNSORTED, None)
