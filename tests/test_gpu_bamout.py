"""GPU: the BAM of `filter -b` built on the device (include/iteres_amd.h itx_bamout_*, csrc/itx_bamout.hip).
1. the ABI, directly: raw BAM records in device tensors (itx_bamout_run) and in a parsed window (itx_bamwin_bamout) with the chosen
   rows given as an array. The expectation is a numpy gather of the hit records; every member is well formed, the members inflate
   to the expectation, and the member sequence equals the host build of the member rule (tests/bgzfmember_host.cpp) on successive
   payload-sized slices of it: the bytes are a pure function of the stream, whatever the batches were;
2. host appends between device batches, the leftover carried across calls, finish with and without a tail;
3. argument and state checks;
4. the command: the emitted file against the records the CPU oracle chooses, the other outputs against a run without -b, both
   routes in one file, and the reference binary reading the emitted file where it is built."""
import ctypes as C
import filecmp
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bedcase as bc
import bgzfmemberhost as bm
import goldencase as gc
import refio
from iteres_amd import build, engine as eng, synth
from oracle import binding as orc
from test_gpu_bed import HEADER, window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "iteres")
TILE = 256                                    # records per workgroup of k_bo_measure / k_bo_gather (csrc/itx_bamout.hip BO_TILE)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return bm.MemberRule(tmp_path_factory.mktemp("bamout_rule"))


@pytest.fixture(scope="module")
def inf():
    h = eng.Inflater()
    yield h
    h.close()


def rec_of_len(L, i=0):
    """a well-formed record of exactly L bytes (block_size field included), L >= 48: the length is made up by a Z tag"""
    base = bc.record(tid=i % 4, pos=100 + i, qname=b"q%02d\0" % (i % 100), cigar=((0, 20),))
    pad = L - len(base) - 4
    assert pad >= 0, L
    r = bc.record(tid=i % 4, pos=100 + i, qname=b"q%02d\0" % (i % 100), cigar=((0, 20),), aux=bc.tag("ZZ", "Z", bytes([65 + i % 23]) * pad + b"\0"))
    assert len(r) == L
    return r


def mixed_records(seed, n):
    """records of 48 .. 400 bytes at every alignment, contents that compress and contents that do not"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(48, 400))
        if i % 7 == 3:
            base = bc.record(tid=i % 4, pos=i, qname=b"r%d\0" % i, cigar=((0, 30),))
            noise = bytes(rng.integers(1, 255, max(L - len(base) - 4, 0), dtype=np.uint8))
            out.append(bc.record(tid=i % 4, pos=i, qname=b"r%d\0" % i, cigar=((0, 30),), aux=bc.tag("ZZ", "Z", noise + b"\0")))
        else:
            out.append(rec_of_len(L, i))
    return out


def tensors(recs):
    import torch
    dev = torch.device("cuda:0")
    off = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint32) if recs else np.zeros(0, np.uint32)
    raw = torch.from_numpy(np.frombuffer(b"".join(recs) + bytes(64), np.uint8).copy()).to(dev)
    return raw, torch.from_numpy(off.view(np.int32).copy()).to(dev)


def gather(recs, rows):
    return b"".join(r for r, h in zip(recs, rows) if h >= 0)


def check_stream(rule, got, want):
    """got: every member the object handed out, finish included; want: the gathered records"""
    ms = bm.split_members(got)
    assert b"".join(bm.check_member(m) for m in ms) == want
    assert ms == rule.members(want)
    assert all(struct.unpack_from("<I", m, len(m) - 4)[0] == rule.payload for m in ms[:len(want) // rule.payload])


def run_once(rule, recs, rows, cap=None):
    import torch
    bo = eng.Bamout(batch_capacity=cap or max(len(recs), 1))
    if recs:
        raw, off = tensors(recs)
        bo.run(raw, off, torch.from_numpy(np.asarray(rows, np.int32)).cuda())
        bo.wait_kernels()
    got = bo.finish()
    st = bo.stats()
    bo.close()
    check_stream(rule, got, gather(recs, rows))
    return got, st


# ---- 1. one batch

def hit_pattern(kind, n):
    i = np.arange(n)
    return {"all": np.full(n, 5), "none": np.full(n, -1), "third": np.where(i % 3 == 0, i % 50, -1)}[kind].astype(np.int32)


def test_no_records(rule):
    got, st = run_once(rule, [], [])
    assert got == b"" and st["members"] == 0 and st["records"] == 0


@pytest.mark.parametrize("hit", [True, False])
def test_one_record(rule, hit):
    got, st = run_once(rule, [rec_of_len(77)], [3 if hit else -1])
    assert st["records"] == int(hit) and st["payload_bytes"] == (77 if hit else 0) and st["members"] == int(hit)
    assert (len(bm.split_members(got)) == 1) == hit


@pytest.mark.parametrize("kind", ["all", "none", "third"])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_tile_boundaries(rule, n, kind):
    recs = mixed_records(n, n)
    rows = hit_pattern(kind, n)
    got, st = run_once(rule, recs, rows)
    assert st["records"] == int((rows >= 0).sum()) and st["batches"] == 1 and st["host_batches"] == 0
    assert st["payload_bytes"] == len(gather(recs, rows)) and st["out_bytes"] == len(got)
    if kind != "none":
        assert st["gather_ms"] > 0 and st["member_ms"] > 0


def test_a_record_longer_than_three_payloads(rule):
    P = rule.payload
    recs = mixed_records(9, 40) + [rec_of_len(3 * P + 17, 1)] + mixed_records(10, 300)
    rows = np.where(np.arange(len(recs)) % 2 == 0, 1, -1).astype(np.int32)
    assert rows[40] >= 0
    got, st = run_once(rule, recs, rows)
    assert st["members"] >= 4


def test_one_batch_of_1026_members(rule):
    """more members in one batch than the one-workgroup scan of their sizes has threads (k_size_scan, csrc/itx_textpack.h, 1024): a
    thread sums two sizes and the threads behind the ragged end none. 23 995 records, 1025 whole payloads and a tail"""
    P = rule.payload
    recs, total = [], 0
    while total <= 1025 * P + 100:
        recs.append(rec_of_len(300 + len(recs) % 101, len(recs)))
        total += len(recs[-1])
    assert 1025 * P < total < 1026 * P
    got, st = run_once(rule, recs, np.full(len(recs), 5, np.int32))
    assert st["members"] == 1026 and st["batches"] == 1


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("k", [1, 3])
def test_totals_around_whole_payloads(rule, k, delta):
    """exactly k payloads: no tail member; one byte more: a tail of one byte; one byte less: a tail one byte short of a payload"""
    total = k * rule.payload + delta
    recs, left, i = [], total, 0
    while left:
        L = 200 + i % 57 if left >= 200 + i % 57 + 48 else left
        recs.append(rec_of_len(L, i))
        left -= L
        i += 1
    others = mixed_records(3, len(recs))                                  # interleaved, not hit
    both = [x for pair in zip(recs, others) for x in pair]
    rows = np.tile(np.array([7, -1], np.int32), len(recs))
    got, st = run_once(rule, both, rows)
    ms = bm.split_members(got)
    assert st["payload_bytes"] == total and len(ms) == -(-total // rule.payload) == k + (delta > 0)
    assert struct.unpack_from("<I", ms[-1], len(ms[-1]) - 4)[0] == (total - 1) % rule.payload + 1


# ---- 2. several calls: the leftover carries, host appends keep their place, finish

def test_three_window_calls_with_host_appends_between(rule, inf):
    """70 001 records of one parsed window in three calls; whole records from the host before, between and after them"""
    import torch
    n = 70_001
    recs = [rec_of_len(48 + (i * 7) % 90, i) for i in range(n)]
    rows = hit_pattern("third", n)
    rows[-1] = 2
    assert window(inf, bc.bam_bytes(HEADER, recs)) == n
    hits = torch.from_numpy(rows).cuda()
    h0, h1, h2 = mixed_records(21, 3), mixed_records(22, 400), [rec_of_len(5000, 4)]
    bo = eng.Bamout(batch_capacity=32768)
    bo.append_host(b"".join(h0))
    cuts = [0, 32768, 32768 + 32767, n]                                    # a full batch, one record less, the rest from an odd index
    want = [b"".join(h0)]
    for c in range(3):
        a, b = cuts[c], cuts[c + 1]
        bo.append_window(inf, a, b - a, hits[a:b])
        carry = bo.stats()["carry"]
        assert 0 <= carry < rule.payload
        want.append(gather(recs[a:b], rows[a:b]))
        if c == 0:
            bo.append_host(b"".join(h1))
            bo.append_host(b"")
            want.append(b"".join(h1))
        assert (sum(len(w) for w in want)) % rule.payload == bo.stats()["carry"]
    bo.wait_kernels()
    bo.append_host(b"".join(h2))
    want.append(b"".join(h2))
    got = bo.finish()
    st = bo.stats()
    bo.close()
    want = b"".join(want)
    check_stream(rule, got, want)
    assert st["batches"] == 3 and st["host_batches"] == 3 and st["carry"] == 0
    assert st["records"] == int((rows >= 0).sum()) + 3 + 400 + 1 and st["payload_bytes"] == len(want)


@pytest.mark.parametrize("tail", [0, 1])
def test_finish_tail(rule, tail):
    P = rule.payload
    recs = [rec_of_len(P // 4, i) for i in range(8)] + ([rec_of_len(48, 9)] if tail else [])
    bo = eng.Bamout(batch_capacity=64)
    import torch
    raw, off = tensors(recs)
    rows = torch.zeros(len(recs), dtype=torch.int32, device="cuda:0")
    bo.run(raw, off, rows)
    before = bytes(bo.out)
    assert len(bm.split_members(before)) == 2 and bo.stats()["carry"] == (48 if tail else 0)
    if tail:                                                              # 48 + (P - 47) bytes: one more payload and a tail of one byte
        bo.append_host(rec_of_len(P - 47, 3))
        assert bo.stats()["carry"] == 1
    got = bo.finish()
    ms = bm.split_members(got)
    assert len(ms) == (4 if tail else 2)
    if tail:
        assert struct.unpack_from("<I", ms[-1], len(ms[-1]) - 4)[0] == 1
    check_stream(rule, got, b"".join(recs) + (rec_of_len(P - 47, 3) if tail else b""))
    bo.close()


def test_bytes_behind_the_reported_length_are_untouched(rule):
    """the two page-locked buffers are filled by the test between batches: a batch's copy writes its `len` bytes and nothing behind"""
    import torch
    big, small = mixed_records(31, 900), mixed_records(32, 300)
    bo = eng.Bamout(batch_capacity=1024)
    seen = {}
    for recs in (big, big, small, small):
        raw, off = tensors(recs)
        bo.run(raw, off, torch.ones(len(recs), dtype=torch.int32, device="cuda:0"), collect=False)
        got = bo.collect()
        addr, ln, room = bo.last
        assert ln == len(got) > 0 and ln <= room
        if addr in seen:
            assert room == seen[addr], "the buffer was replaced: the case does not test what it says"
            behind = C.string_at(addr + ln, room - ln)
            assert behind == b"\xa5" * (room - ln)
            assert C.string_at(addr, ln) == got
        C.memset(addr, 0xA5, room)
        seen[addr] = room
    assert len(seen) == 2
    bo.finish()
    bo.close()


# ---- 3. argument and state checks

def test_argument_checks(rule, inf):
    import torch
    L = eng.load()
    h = C.c_void_p()
    m = eng.BamoutMembers()
    assert L.itx_bamout_create(0, 0, 0, C.byref(h)) == -1 and L.itx_bamout_create(0, 16, 0, None) == -1
    assert L.itx_bamout_finish(None) == -1 and L.itx_bamout_get_stats(None, None) == -1 and L.itx_bamout_wait_kernels(None) == -1
    assert L.itx_bamout_append_host(None, None, 0) == -1 and L.itx_bamout_collect(None, C.byref(m)) == -1
    assert L.itx_bamout_run(None, None, None, None, 0, None) == -1 and L.itx_bamout_pending(None) == 0
    bo = eng.Bamout(batch_capacity=16)
    z = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p = C.c_void_p(z.data_ptr())
    assert L.itx_bamout_collect(bo._h, None) == -1
    assert L.itx_bamwin_bamout(None, bo._h, 0, 0, p, None) == -1 and L.itx_bamwin_bamout(inf._h, None, 0, 0, p, None) == -1
    assert L.itx_bamwin_bamout(inf._h, bo._h, 0, 1 << 40, p, None) == -1                   # beyond the parsed window
    assert L.itx_bamout_run(bo._h, p, p, p, 17, None) == -1                                 # above the capacity
    assert L.itx_bamout_run(bo._h, None, None, None, 5, None) == -1                         # records without arrays
    assert L.itx_bamout_append_host(bo._h, None, 3) == -1
    ragged = rec_of_len(60) + rec_of_len(70)[:-1]
    assert L.itx_bamout_append_host(bo._h, ragged, len(ragged)) == -1 and b"whole records" in L.itx_last_error()
    assert L.itx_bamout_append_host(bo._h, b"\x01\x00", 2) == -1
    assert bo.stats()["records"] == 0 and bo.stats()["carry"] == 0                          # nothing of the refused calls was appended
    # a record that claims a gibibyte: ITX_E_LIMIT, nothing appended
    liar = bytearray(rec_of_len(64))
    liar[0:4] = struct.pack("<I", 0x40000000)
    raw, off = tensors([bytes(liar)])
    assert L.itx_bamout_run(bo._h, C.c_void_p(raw.data_ptr()), C.c_void_p(off.data_ptr()), p, 1, None) == -6
    assert bo.stats()["records"] == 0 and bo.stats()["carry"] == 0
    # two batches wait: a third that completes a payload is refused and leaves the stream as it was
    one = rec_of_len(rule.payload)
    bo.append_host(one, collect=False)
    bo.append_host(one, collect=False)
    assert L.itx_bamout_pending(bo._h) == 2
    assert L.itx_bamout_append_host(bo._h, one, len(one)) == -5 and b"collect" in L.itx_last_error()
    assert bo.stats()["records"] == 2
    bo.append_host(rec_of_len(100), collect=False)                                          # completes none: taken
    got = bo.finish()
    check_stream(rule, got, one + one + rec_of_len(100))
    assert L.itx_bamout_finish(bo._h) == -5                                                 # ITX_E_STATE: called twice
    assert L.itx_bamout_append_host(bo._h, one, len(one)) == -5
    assert L.itx_bamout_run(bo._h, p, p, p, 1, None) == -5
    bo.close()


# ---- 4. the command

@pytest.fixture(scope="module")
def exe():
    lib, exe = build.build_all()
    return exe


CHROMS = [("chr1", 3_000_000), ("chr2", 1_500_000), ("chrM", 16_571)]
BAM_HEADER = [("chr1", 3_000_000), ("chrU", 150_000), ("chr2", 1_500_000), ("chrM", 16_571)]     # chrU: not in the size file


@pytest.fixture(scope="module")
def pile(tmp_path_factory):
    """inputs laid out as a golden case (tests/goldencase.py reads <case>/in), so that the table model and the side masks of the
    oracle tests serve here too"""
    root = tmp_path_factory.mktemp("bamout_cases")
    d = root / "bamout" / "in"
    d.mkdir(parents=True)
    t = synth.make_table(91, CHROMS, 6000, n_names=80, n_fams=12, n_clas=5, overlap_frac=0.05)
    synth.write_sizes(str(d / "chrom.sizes"), CHROMS)
    synth.write_sizes(str(d / "rep.sizes"), t.rep_len.items())
    synth.write_rmsk(str(d / "rmsk.txt"), t)
    for name, header, tids, pf in (("single.bam", CHROMS, None, 0.0), ("paired.bam", CHROMS, None, 0.6), ("mixed.bam", BAM_HEADER, None, 0.2)):
        r = synth.make_reads(17 + len(name), header, 5000, paired_frac=pf, tids=tids)
        r.mapq[:64] = 37                                                   # (-R: the reference's key buffer is set by the first MAPQ >= Q record)
        synth.write_bam(str(d / name), r, block=6000)
    big = t.clas[int(np.bincount(np.asarray(t.cla_of_row)).argmax())]
    name = t.names[int(np.bincount(np.asarray(t.rep_name)).argmax())]
    return root, d, big, name


def raw_records(path):
    """(the header's bytes, the records' bytes one by one) of a BAM file"""
    raw = refio.bgzf_decompress(open(path, "rb").read())
    l_text, = struct.unpack_from("<i", raw, 4)
    off = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, off)
    off += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, off)
        off += 8 + l_name
    head, recs = raw[:off], []
    while off < len(raw):
        bs, = struct.unpack_from("<i", raw, off)
        recs.append(raw[off:off + 4 + bs])
        off += 4 + bs
    assert off == len(raw)
    return head, recs


def oracle_rows(root, aln, opts):
    """the row the CPU oracle chooses per record of <case>/in/<aln> for these options (-1: none), and the per-locus counts"""
    saved = gc.GOLDEN
    gc.GOLDEN = str(root)
    try:
        p = gc.parse_opts("filter", [o for o in opts if o != "-b"])
        tm = gc.build_table_model("bamout", p["filter_field"], p["filter_name"])
        header, rd = gc.load_reads("bamout", aln)
    finally:
        gc.GOLDEN = saved
    ot = orc.OracleTable(tm.chrom_size, tm.rep_len, len(tm.fams), len(tm.clas))
    st = ot.add_rows(tm.chrom, [r["start"] for r in tm.rows], [r["end"] for r in tm.rows], [r["cons_start"] for r in tm.rows], [r["cons_end"] for r in tm.rows],
                     tm.rep, tm.fam, tm.cla)
    assert (st == np.arange(len(tm.rows))).all()

    def run_oracle(skip):
        return ot.run(p, gc.tid_map(header, tm, p["add_chr"]), rd["tid"], rd["pos"], rd["tmpend"], rd["mapq"], rd["flag"], rd["mpos"], rd["isize"], skip=skip)
    dup, veto = gc.side_masks(p, tm, header, rd, ot, run_oracle)
    assert not veto.any()
    res = run_oracle(dup)
    return res["hit_row"], res["locus_cnt"]


def run_filter(exe, d, out, opts, aln, env=None, binary=None):
    os.makedirs(out, exist_ok=True)
    pr = subprocess.run([binary or exe, "filter"] + list(opts) + ["-o", "out", str(d / "chrom.sizes"), str(d / "rep.sizes"), str(d / "rmsk.txt"), str(aln)],
                        cwd=out, capture_output=True, text=True, timeout=600, env=dict(os.environ, ITX_TIMING="1", ITX_BGZF_CHUNK="40000", **(env or {})))
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr


def routes(err):
    m = re.search(r"\[itx timing\] bam out: (\d+) records, (\d+) payload bytes, (\d+) members \((\d+) bytes\), [0-9.]+ ms in the gather kernels, [0-9.]+ ms in the member "
                  r"kernels, host waited [0-9.]+ s, (\d+) batches gathered on the device, (\d+) batches by the host route", err)
    assert m, err[-1500:]
    return dict(zip(("records", "payload", "members", "out_bytes", "dev", "host"), map(int, m.groups())))


def check_emitted(path, aln, hit_row):
    """the emitted file against the input and the chosen rows; returns the number of records"""
    data = open(path, "rb").read()
    assert data.endswith(bm.EOF_MARKER)
    for m in bm.split_members(data):
        bm.check_member(m)
    head, recs = raw_records(aln)
    got_head, got = raw_records(path)
    assert got_head == head
    want = [r for r, h in zip(recs, hit_row) if h >= 0]
    assert len(got) == len(want) and got == want
    header, rd = refio.read_bam(path)                                       # an independent parse of the records
    assert len(rd["tid"]) == len(want) and header == refio.read_bam(aln)[0]
    return len(want)


def loci_total(path):
    _, rows = refio.parse_loci(path)
    return sum(int(r[7]) for r in rows), [r[:8] for r in rows]


OPTSETS = {"single_ALL": ("single.bam", ()), "paired_ALL": ("paired.bam", ()), "single_n": ("single.bam", ("-n", "NAME")), "paired_c": ("paired.bam", ("-c", "CLASS")),
           "paired_R": ("paired.bam", ("-R",)), "paired_T": ("paired.bam", ("-T",)), "single_R_t3": ("single.bam", ("-R", "-t", "3")),
           "paired_r": ("paired.bam", ("-r",))}


@pytest.mark.parametrize("which", list(OPTSETS))
def test_command(which, pile, exe, tmp_path):
    root, d, big, name = pile
    aln, opts = OPTSETS[which]
    opts = tuple({"NAME": name, "CLASS": big}.get(o, o) for o in opts)
    sub = name if "-n" in opts else big if "-c" in opts else "ALL"
    env = {"ITX_HOST_NAMES": "0"}                                           # -b -r: one classification for both gatherers
    with_b = run_filter(exe, d, str(tmp_path / "b"), ("-b",) + opts, d / aln, env)
    run_filter(exe, d, str(tmp_path / "plain"), opts, d / aln, env)
    names = sorted(os.listdir(tmp_path / "b"))
    assert names == sorted(os.listdir(tmp_path / "plain") + [f"out_{sub}.iteres.bam"])
    for fn in os.listdir(tmp_path / "plain"):
        assert filecmp.cmp(tmp_path / "b" / fn, tmp_path / "plain" / fn, shallow=False), fn
    hit_row, locus_cnt = oracle_rows(root, aln, opts)
    n = check_emitted(tmp_path / "b" / f"out_{sub}.iteres.bam", d / aln, hit_row)
    assert n == int(locus_cnt.sum()) and n > (200 if sub == "ALL" else 20)
    if "-t" not in opts:
        assert loci_total(tmp_path / "b" / f"out_{sub}.iteres.loci")[0] == n
    else:                                                                   # every counted record goes in, whatever -t says
        run_filter(exe, d, str(tmp_path / "t1"), [o for o in opts if o not in ("-t", "3")], d / aln, env)
        assert loci_total(tmp_path / "t1" / f"out_{sub}.iteres.loci")[0] == n > loci_total(tmp_path / "b" / f"out_{sub}.iteres.loci")[0]
    rt = routes(with_b.stderr)
    assert rt["records"] == n and rt["dev"] >= 3 and rt["host"] == 0 and rt["members"] >= (2 if sub == "ALL" else 1), rt
    if os.path.exists(REF):
        # an independent reader accepts the file: the reference counts the same reads per locus over it as over the input
        ref_opts = [o for o in opts if o not in ("-t", "3")]
        run_filter(exe, d, str(tmp_path / "ref_in"), ref_opts, d / aln, binary=REF)
        run_filter(exe, d, str(tmp_path / "ref_out"), ref_opts, tmp_path / "b" / f"out_{sub}.iteres.bam", binary=REF)
        assert loci_total(tmp_path / "ref_in" / f"out_{sub}.iteres.loci")[1] == loci_total(tmp_path / "ref_out" / f"out_{sub}.iteres.loci")[1]


@pytest.mark.parametrize("opts", [(), ("-R",), ("-r",)], ids=["ALL", "R", "r"])
def test_command_both_routes_in_one_file(opts, pile, exe, tmp_path):
    """mapped records on chrU, which the size file lacks, lie in the middle of the sorted file: their windows take the host route
    (the warning is per record), the windows before and after stay on the device, and the file is one ordered stream"""
    root, d, big, name = pile
    with_b = run_filter(exe, d, str(tmp_path / "b"), ("-b",) + opts, d / "mixed.bam", {"ITX_HOST_NAMES": "0"})
    run_filter(exe, d, str(tmp_path / "plain"), opts, d / "mixed.bam", {"ITX_HOST_NAMES": "0"})
    for fn in os.listdir(tmp_path / "plain"):
        assert filecmp.cmp(tmp_path / "b" / fn, tmp_path / "plain" / fn, shallow=False), fn
    hit_row, locus_cnt = oracle_rows(root, "mixed.bam", opts)
    n = check_emitted(tmp_path / "b" / "out_ALL.iteres.bam", d / "mixed.bam", hit_row)
    rt = routes(with_b.stderr)
    assert rt["records"] == n == int(locus_cnt.sum()) and rt["dev"] >= 2 and rt["host"] >= 1, rt
    assert with_b.stderr.count("read ends mapped to chromosome chrU will be discarded") == 1
    # the host route's windows lie between device windows: hits before and after the chrU records
    _, rd = refio.read_bam(d / "mixed.bam")
    u = np.flatnonzero(rd["tid"] == 1)
    assert (hit_row[:u[0]] >= 0).sum() > 100 and (hit_row[u[-1] + 1:] >= 0).sum() > 100
