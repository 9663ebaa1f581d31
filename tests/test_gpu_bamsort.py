"""GPU: `filter -b -s`, the counted records held on the device, sorted by coordinate and replayed through the member path
(include/iteres_amd.h itx_bamout_sort_*, csrc/itx_bamout_sort.hip; the order is csrc/itx_bamsortrule.h).
The oracle is Python and shares no code with the product: sorted(records, key=(tid, pos, reverse)) over the records of the stream as
-b alone would write it (Python's sort is stable). Every ABI case compares three things with it: the collected members' bytes (the
host build of the member rule, tests/bgzfmemberhost.py, over payload-sized slices of the sorted stream), the decoded record sequence,
and the index's bytes (tests/baicase.py's restatement over the sorted stream and the emitted members) with status OK.
1. the ABI through engine.Bamout: shapes around the record tile, equal keys, strands, references without records, long records,
   payload boundaries, no / two / three passes over tid, 70 001 records replayed in 18 rounds from a held stream and a pool that
   grow, state and argument checks, fetch equivalence through the index;
2. the command: -b -i -s against -b of the same input.
A held stream beyond 2^32 bytes is not among the cases: DESIGN.md ("Coordinate sort on the device") says why."""
import ctypes as C
import filecmp
import os
import re
import struct

import numpy as np
import pytest

import baicase as bai
import bedcase as bc
import bgzfmemberhost as bm
import goldencase as gc
import refio
from iteres_amd import engine as eng, synth
from test_bamsort_rule import py_header
from test_gpu_bamidx import regions, tensors
from test_gpu_bamout import BAM_HEADER, CHROMS, exe, pile, raw_records, routes, rule, run_filter   # noqa: F401  (fixtures and the synthetic inputs)

pytestmark = pytest.mark.gpu

P = bai.PAYLOAD
M, N = 0, 3
_BASE = len(bc.record(qname=b"q\0", cigar=((M, 50),), aux=bc.tag("ZZ", "Z", b"\0")))


def srec(tid, pos, flag=0, name=b"q", cigar=((M, 50),), L=None):
    """a record at (tid, pos) on the strand flag & 16 says; L: its exact length in bytes (block_size field included), made up by a Z tag"""
    qn = name + b"\0"
    if L is None:
        return bc.record(tid=tid, pos=pos, flag=flag, qname=qn, cigar=cigar)
    pad = L - _BASE - (len(qn) - 2) - 4 * (len(cigar) - 1)
    assert pad >= 0, L
    r = bc.record(tid=tid, pos=pos, flag=flag, qname=qn, cigar=cigar, aux=bc.tag("ZZ", "Z", bytes([65 + pos % 23]) * pad + b"\0"))
    assert len(r) == L
    return r


def key_of(r):
    """(tid, pos, reverse) of a record's bytes: the oracle's sort key"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    flag, = struct.unpack_from("<H", r, 18)
    return tid, pos, (flag >> 4) & 1


def split_records(stream):
    out, at = [], 0
    while at < len(stream):
        bs, = struct.unpack_from("<I", stream, at)
        out.append(stream[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(stream)
    return out


def drive(l_ref, steps, first=0, cap=None, index=True, sort=True, stream_bytes=0):
    """steps: ("run", records, rows) or ("host", records). -> (members, the counted records in input order, status, index bytes,
    the index's counters, stats, the sort's counters)"""
    import torch
    bo = eng.Bamout(batch_capacity=cap or max([len(s[1]) for s in steps if s[0] == "run"] + [1]), stream_bytes=stream_bytes)
    try:
        if sort:
            bo.sort_enable()
        if index:
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
            if sort:
                assert bo.out == b"" and bo.stats()["members"] == 0        # nothing leaves during the pass
        got = bo.sort_all() if sort else bo.finish()
        status, idx, info = bo.index_finish(first) if index else (None, None, None)
        return got, counted, status, idx, info, bo.stats(), bo.sort_stats()
    finally:
        bo.close()


def check(rule, l_ref, steps, first=0, cap=None, index=True, stream_bytes=0):
    got, counted, status, idx, info, st, ss = drive(l_ref, steps, first, cap, index, True, stream_bytes)
    want = sorted(counted, key=key_of)
    stream = b"".join(want)
    ms = bm.split_members(got)
    assert ms == rule.members(stream)                                      # 1. the members' bytes
    assert split_records(b"".join(bm.check_member(m) for m in ms)) == want   # 2. the decoded record sequence
    if index:                                                              # 3. the index's bytes
        assert status == bai.OK
        assert (status, idx) == bai.expected(l_ref, stream, [len(m) for m in ms], first)
        assert info["entries"] == len(want)
    cap = cap or max([len(s[1]) for s in steps if s[0] == "run"] + [1])
    assert ss["records"] == st["records"] == len(want) and ss["rounds"] == -(-len(want) // cap) and st["carry"] == 0
    assert st["members"] == len(ms) == -(-len(stream) // P) and st["payload_bytes"] == len(stream)
    return got, want, idx, st, ss


def all_hit(recs):
    return [0] * len(recs)


# ---- 1. the ABI

def test_no_records_three_references(rule):
    got, want, idx, st, ss = check(rule, [1000, 0, 5_000_000], [], first=77)
    assert got == b"" and idx == b"BAI\1" + (3).to_bytes(4, "little") + bytes(3 * 8) + bytes(8) and ss["rounds"] == 0


def test_one_record(rule):
    got, want, idx, st, ss = check(rule, [100_000], [("run", [srec(0, 20_000, 16)], [4])], first=1234)
    assert len(bm.split_members(got)) == 1 and ss["rounds"] == 1


@pytest.mark.parametrize("route", ["run", "host"])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_descending_records_around_the_tile(rule, n, route):
    recs = [srec(2 - i * 3 // n, 70_000 - 64 * i, 16 * (i % 2), b"d%d" % i, L=60 + i % 90) for i in range(n)]
    step = ("run", recs, all_hit(recs)) if route == "run" else ("host", recs)
    got, want, idx, st, ss = check(rule, [1 << 20] * 3, [step], first=4096, cap=n)
    assert want == recs[::-1]


def test_equal_keys_keep_their_input_order(rule):
    """1 000 records with one key and distinct names, half from a device batch and half from the host route"""
    recs = [srec(1, 5000, 16, b"name%04d" % ((i * 37) % 1000)) for i in range(1000)]
    got, want, idx, st, ss = check(rule, [9000, 9000], [("run", recs[:500], all_hit(recs[:500])), ("host", recs[500:])], cap=512)
    assert want == recs and len({r for r in recs}) == 1000 and ss["rounds"] == 2


def test_equal_positions_with_alternating_strands(rule):
    """forward before reverse at one position, each strand's records in input order"""
    recs = [srec(0, 300 + (i // 20), 16 * ((i + 1) % 2), b"s%d" % i) for i in range(400)]
    got, want, idx, st, ss = check(rule, [9000], [("run", recs, all_hit(recs))])
    assert [key_of(r)[2] for r in want[:20]] == [0] * 10 + [1] * 10 and want[:10] == recs[1:20:2]


def test_references_without_records_between_those_that_arrive_out_of_order(rule):
    l_ref = [50_000, 70_000, 90_000, 0, 60_000, 20_000]
    recs = [srec(4, 100 + i, name=b"a%d" % i) for i in range(30)] + [srec(0, 40_000 - i, name=b"b%d" % i) for i in range(30)] + \
           [srec(2, 500 + (i * 7) % 30, 16 * (i % 2), name=b"c%d" % i) for i in range(30)]
    got, want, idx, st, ss = check(rule, l_ref, [("run", recs[:45], all_hit(recs[:45])), ("host", recs[45:])], first=100)
    assert [x["meta"] is not None for x in bai.parse_bai(idx)] == [True, False, True, False, True, False]


def test_a_record_of_three_payloads_and_17_bytes_moves_from_last_to_first(rule):
    recs = [srec(0, 1000 + 10 * i, L=300) for i in range(40)] + [srec(0, 5, L=3 * P + 17)]
    got, want, idx, st, ss = check(rule, [100_000], [("run", recs, all_hit(recs))], first=3)
    assert want[0] == recs[-1] and len(bm.split_members(got)) == 5


def test_a_record_whose_sorted_place_starts_on_the_last_byte_of_a_payload(rule):
    recs = [srec(0, 40_000, L=77), srec(0, 30, L=P - 100), srec(0, 20, L=100), srec(0, 10, L=P - 1)]
    got, want, idx, st, ss = check(rule, [100_000], [("run", recs, all_hit(recs))], first=500)
    assert want == recs[::-1] and len(bm.split_members(got)) == 3
    assert bai.parse_bai(idx)[0]["bins"][4681][0][0] == 500 << 16


@pytest.mark.parametrize("tail", [0, 1])
def test_the_sorted_stream_ends_on_a_payload_boundary_or_with_a_tail(rule, tail):
    recs = ([srec(1, 9, L=50)] if tail else []) + [srec(1, 5, L=P), srec(0, 20, L=P // 2), srec(0, 10, L=P // 2)]
    got, want, idx, st, ss = check(rule, [1000, 1000], [("host", recs[:1]), ("run", recs[1:], all_hit(recs[1:]))], first=28)
    ms = bm.split_members(got)
    assert len(ms) == 2 + tail and struct.unpack_from("<I", ms[-1], len(ms[-1]) - 4)[0] == (50 if tail else P)


@pytest.mark.parametrize("n_ref", [1, 257, 65_537])
def test_passes_over_tid(rule, n_ref):
    """ceil(bits(n_ref - 1) / 8) passes over tid: none, two and three. 65 537 references run without an index (which refuses that
    many), so the count comes from the highest tid seen"""
    top = n_ref - 1
    tids = sorted({0, top, top // 2, min(255, top), min(256, top), min(65_535, top), top & 0xff00, top & 0xff})
    recs = [srec(t, 900 - 7 * k - i, 16 * (i % 2), b"t%d_%d" % (t, i)) for i in range(6) for k, t in enumerate(reversed(tids))]
    index = n_ref < 65_536
    got, want, idx, st, ss = check(rule, [1000] * n_ref if index else [], [("run", recs[:20], all_hit(recs[:20])), ("host", recs[20:])], index=index)
    assert [key_of(r)[0] for r in want] == sorted(key_of(r)[0] for r in recs) and key_of(want[-1])[0] == top


def test_records_that_are_not_counted_leave_no_trace(rule):
    recs = [srec(0, 900 - i, name=b"n%d" % i) for i in range(300)] + [srec(-1, -1, name=b"unmapped")]
    rows = [3 if i % 3 == 1 else -1 for i in range(300)] + [-1]
    got, want, idx, st, ss = check(rule, [1000], [("run", recs, rows)])
    assert len(want) == 100 and ss["records"] == 100
    none = check(rule, [1000], [("run", recs, [-1] * 301)])
    assert none[0] == b"" and none[4]["rounds"] == 0


def test_input_in_order_gives_the_members_of_a_run_without_the_sort(rule):
    recs = sorted([srec(i % 3, (i * 7919) % 50_000, 16 * (i % 2), b"o%d" % i, L=60 + i % 200) for i in range(3000)], key=key_of)
    steps = [("run", recs[:1000], all_hit(recs[:1000])), ("host", recs[1000:1500]), ("run", recs[1500:], all_hit(recs[1500:]))]
    got, want, idx, st, ss = check(rule, [50_100] * 3, steps, first=9, cap=1500)
    plain = drive([50_100] * 3, steps, first=9, cap=1500, sort=False)
    assert want == recs and got == plain[0] and idx == plain[3]


def big_case():
    """70 001 counted records: three `run` calls (4 096, 4 095 and 4 000 records, a third, all and half of them counted) with host
    appends before, between and after them; positions repeat, so that equal keys meet across the calls; now and then a spliced
    record, so that every bin level has chunks. References 0, 2 and 3 have records."""
    l_ref = [4_000_000, 1000, 3_700_000, 5_000_000]
    rng = np.random.default_rng(13)
    n = 12_191 + 62_540

    def one(k):
        tid = (0, 2, 3)[int(rng.integers(3))]
        pos = int(rng.integers(0, 30_000)) * 100
        cig = ((M, 30), (N, 20_000 << (k % 6)), (M, 20)) if k % 101 == 0 else ((M, 20 + k % 80),)
        return srec(tid, pos, 16 * int(rng.integers(2)), b"r%d" % k, cig)
    recs = [one(k) for k in range(n)]
    cuts = [0, 20_000, 24_096, 44_096, 48_191, 68_191, 72_191, n]
    kinds = ["host", "run", "host", "run", "host", "run", "host"]
    every = {1: 3, 3: 1, 5: 2}
    steps = []
    for c, kind in enumerate(kinds):
        part = recs[cuts[c]:cuts[c + 1]]
        steps.append(("host", part) if kind == "host" else ("run", part, [2 if i % every[c] == 0 else -1 for i in range(len(part))]))
    counted = sum(len(s[1]) for s in steps if s[0] == "host") + sum(h >= 0 for s in steps if s[0] == "run" for h in s[2])
    assert counted == 70_001, counted
    return l_ref, steps


@pytest.fixture(scope="module")
def big(rule):
    l_ref, steps = big_case()
    first = 3000
    got, want, idx, st, ss = check(rule, l_ref, steps, first=first, cap=4096, stream_bytes=1)
    return l_ref, first, got, want, idx, st, ss


def test_three_runs_and_host_appends_replayed_in_18_rounds(big):
    l_ref, first, got, want, idx, st, ss = big
    assert len(want) == 70_001 and ss["rounds"] == 18 and st["batches"] == 3 and st["host_batches"] == 4
    assert st["grows"] >= 3 and ss["pool_grows"] >= 1, (st, ss)            # the held stream from its minimum; the pool
    assert ss["sort_ms"] > 0 and ss["replay_ms"] > 0
    inside = sum((len(b"".join(want[:k])) % P) != 0 for k in range(4096, 70_001, 4096))
    assert inside >= 16                                                    # round boundaries fall inside payloads
    keys = [key_of(r) for r in want]
    assert sum(a == b for a, b in zip(keys, keys[1:])) > 5000               # equal keys, kept in input order by the oracle


def test_fetch_equivalence(big):
    """300 seeded regions through OUR index by the restatement's independent reader against a linear scan; seed 20 gives 215
    regions that fetch a record (counted on the CPU from the case alone)"""
    l_ref, first, got, want, idx, st, ss = big
    stream = b"".join(want)
    sizes = [size for off, size, isize in bai.member_walk(got)]
    coff = np.cumsum([0] + sizes)
    ustart = {first + int(coff[k]): min(k * P, len(stream)) for k in range(len(sizes) + 1)}
    parsed = bai.parse_bai(idx)
    recs = bai.records_of(stream)
    r_tid, r_pos, r_end, r_at, _ = np.array(recs, np.int64).T
    hits = 0
    for tid, beg, end in regions(l_ref, recs, seed=20):
        found = bai.fetch(parsed, stream, ustart, tid, beg, end)
        assert found == set(r_at[(r_tid == tid) & (r_pos < end) & (r_end > beg)].tolist()), (tid, beg, end)
        hits += bool(found)
    assert hits == FETCH_HITS >= 150, hits


FETCH_HITS = 215


def test_argument_and_state_checks(rule):
    import torch
    L = eng.load()
    more = C.c_int(7)
    ss = eng.BamoutSortStats()
    assert L.itx_bamout_sort_enable(None) == -1 and L.itx_bamout_sort_next(None, C.byref(more)) == -1 and L.itx_bamout_sort_get_stats(None, C.byref(ss)) == -1
    bo = eng.Bamout(batch_capacity=16)
    assert L.itx_bamout_sort_next(bo._h, None) == -1 and L.itx_bamout_sort_get_stats(bo._h, None) == -1
    assert L.itx_bamout_sort_next(bo._h, C.byref(more)) == -5 and b"sort_enable" in L.itx_last_error() and more.value == 0
    assert L.itx_bamout_sort_enable(bo._h) == 0
    assert L.itx_bamout_sort_enable(bo._h) == -5 and b"twice" in L.itx_last_error()
    assert L.itx_bamout_finish(bo._h) == -5 and b"sort_next" in L.itx_last_error()      # finish in sort mode
    one = srec(0, 5, L=P)
    for k in range(4):                                                     # no two-batch limit during the pass: nothing is pending
        bo.append_host(one, collect=False)
    assert L.itx_bamout_pending(bo._h) == 0 and bo.stats()["carry"] == 4 * P
    assert bo.sort_next() is False
    z = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p = C.c_void_p(z.data_ptr())
    assert L.itx_bamout_run(bo._h, p, p, p, 1, None) == -5 and L.itx_bamout_append_host(bo._h, one, len(one)) == -5      # after the replay
    assert L.itx_bamout_sort_next(bo._h, C.byref(more)) == -5 and b"finished" in L.itx_last_error()
    assert bm.split_members(bytes(bo.out)) == rule.members(one * 4)
    bo.close()
    late = eng.Bamout(batch_capacity=16)                                   # after the first batch
    late.append_host(srec(0, 5))
    assert L.itx_bamout_sort_enable(late._h) == -5 and b"begun" in L.itx_last_error()
    late.finish()
    late.close()
    mid = eng.Bamout(batch_capacity=2)                                     # run after the first sort_next, while rounds remain
    mid.sort_enable()
    mid.append_host(b"".join(srec(0, 50 - i) for i in range(5)))
    assert mid.sort_next() is True
    assert L.itx_bamout_run(mid._h, p, p, p, 1, None) == -5 and b"replayed" in L.itx_last_error()
    assert L.itx_bamout_append_host(mid._h, one, len(one)) == -5
    assert mid.sort_next() is True and mid.sort_next() is False and mid.sort_stats()["rounds"] == 3
    assert split_records(refio.bgzf_decompress(bytes(mid.out))) == [srec(0, 50 - i) for i in range(5)][::-1]
    mid.close()
    for route in ("run", "host"):                                          # a counted record that names no reference: ITX_E_LIMIT, no member
        bad = eng.Bamout(batch_capacity=16)
        bad.sort_enable()
        recs = [srec(0, 9), srec(-1, -1), srec(0, 3)]
        if route == "run":
            raw, off = tensors(recs)
            bad.run(raw, off, torch.zeros(3, dtype=torch.int32, device="cuda:0"))
        else:
            bad.append_host(b"".join(recs))
        assert L.itx_bamout_sort_next(bad._h, C.byref(more)) == -6 and b"tid or pos below 0" in L.itx_last_error() and more.value == 0
        assert L.itx_bamout_pending(bad._h) == 0 and bad.stats()["members"] == 0
        bad.close()
    neg = eng.Bamout(batch_capacity=16)                                    # pos = -1 alone does the same
    neg.sort_enable()
    neg.append_host(srec(2, -1))
    assert L.itx_bamout_sort_next(neg._h, C.byref(more)) == -6
    neg.close()


# ---- 2. the command

def sort_line(err):
    m = re.search(r"; sort: (\d+) records sorted, (\d+) rounds, [0-9.]+ ms in the sort kernels, [0-9.]+ ms in the replay gathers", err)
    assert m, err[-1500:]
    return tuple(map(int, m.groups()))


def header_parts(head):
    """(the text, what follows it) of a BAM header's bytes"""
    l_text, = struct.unpack_from("<i", head, 4)
    assert head[:4] == b"BAM\1"
    return head[8:8 + l_text], head[8 + l_text:]


def check_command(exe, d, tmp_path, opts, aln, sub="ALL", env=None):
    """-b -i -s against -b alone of the same input, the oracle and the index's restatement; returns the -b -i -s run"""
    env = dict({"ITX_HOST_NAMES": "0"}, **(env or {}))
    srt = run_filter(exe, d, str(tmp_path / "bsi"), ("-b", "-s", "-i") + tuple(opts), aln, env)
    run_filter(exe, d, str(tmp_path / "b"), ("-b",) + tuple(opts), aln, env)
    bam = f"out_{sub}.iteres.bam"
    assert sorted(os.listdir(tmp_path / "bsi")) == sorted(os.listdir(tmp_path / "b") + [bam + ".bai"])
    for fn in os.listdir(tmp_path / "b"):                                  # .loci, .reportloci, the read lists
        if fn != bam:
            assert filecmp.cmp(tmp_path / "bsi" / fn, tmp_path / "b" / fn, shallow=False), fn
    head_b, recs_b = raw_records(tmp_path / "b" / bam)
    head_s, recs_s = raw_records(tmp_path / "bsi" / bam)
    assert recs_s == sorted(recs_b, key=key_of) and len(recs_s) > 20
    (text_b, refs_b), (text_s, refs_s) = header_parts(head_b), header_parts(head_s)
    assert text_s == py_header(text_b) and refs_s == refs_b and b"SO:coordinate" in text_s.split(b"\n")[0]
    data = open(tmp_path / "bsi" / bam, "rb").read()
    assert data.endswith(bm.EOF_MARKER)
    status, want = bai.expected_for_file(data)
    assert status == bai.OK and open(tmp_path / "bsi" / (bam + ".bai"), "rb").read() == want
    n, rounds = sort_line(srt.stderr)
    assert n == len(recs_s) == routes(srt.stderr)["records"] and rounds == 1
    assert "no index is written" not in srt.stderr
    return srt, recs_b


def test_command_unsorted_input(pile, exe, tmp_path):
    root, d, big_cla, name = pile
    r = synth.make_reads(33, CHROMS, 3000, sorted_=False)
    synth.write_bam(str(tmp_path / "unsorted.bam"), r, block=6000)
    srt, recs_b = check_command(exe, d, tmp_path, (), tmp_path / "unsorted.bam")
    assert recs_b != sorted(recs_b, key=key_of)


def shuffled_bam(path, head, recs, seed, keep_together=None):
    """the records in a seeded random order behind the same header; keep_together(record): those records stay one run in the middle"""
    rng = np.random.default_rng(seed)
    mid = [r for r in recs if keep_together and keep_together(r)]
    rest = [r for r in recs if not (keep_together and keep_together(r))]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    mid = [mid[i] for i in rng.permutation(len(mid))]
    order = rest[:len(rest) // 2] + mid + rest[len(rest) // 2:]
    buf = head + b"".join(order)
    with open(path, "wb") as f:
        f.write(b"".join(synth.bgzf_block(buf[i:i + 6000]) for i in range(0, len(buf), 6000)) + synth.BGZF_EOF)
    return order


def test_command_host_route_in_the_middle(pile, exe, tmp_path):
    """mixed.bam shuffled, its chrU records (which send their windows through the host route) kept as one run in the middle"""
    root, d, big_cla, name = pile
    head, recs = raw_records(d / "mixed.bam")
    shuffled_bam(tmp_path / "shuffled.bam", head, recs, 5, keep_together=lambda r: key_of(r)[0] == 1)
    srt, recs_b = check_command(exe, d, tmp_path, (), tmp_path / "shuffled.bam")
    rt = routes(srt.stderr)
    assert rt["dev"] >= 2 and rt["host"] >= 1, rt


def test_command_on_a_shuffled_golden_input(exe, tmp_path):
    src = os.path.join(gc.GOLDEN, "mid", "in")
    head, recs = raw_records(refio.materialise(src, "reads.bam", str(tmp_path)))
    shuffled_bam(tmp_path / "shuffled.bam", head, recs, 6)

    class D:                                                               # run_filter joins the three table files onto d
        def __truediv__(self, name):
            return refio.materialise(src, name, str(tmp_path))
    check_command(exe, D(), tmp_path, (), tmp_path / "shuffled.bam")


@pytest.mark.parametrize("which", ["r", "R", "T", "c"])
def test_command_options(which, pile, exe, tmp_path):
    root, d, big_cla, name = pile
    r = synth.make_reads(34, CHROMS, 3000, paired_frac=0.6, sorted_=False)
    r.mapq[:64] = 37
    synth.write_bam(str(tmp_path / "unsorted.bam"), r, block=6000)
    opts = {"r": ("-r",), "R": ("-R",), "T": ("-T",), "c": ("-c", big_cla)}[which]
    check_command(exe, d, tmp_path, opts, tmp_path / "unsorted.bam", sub=big_cla if which == "c" else "ALL")


def test_command_already_sorted_input(pile, exe, tmp_path):
    """on input stably sorted by (tid, pos, reverse), -b -i -s differs from -b -i in the header's members only, and the .bai by the
    offset that shift makes"""
    root, d, big_cla, name = pile
    head, recs = raw_records(d / "single.bam")
    with open(tmp_path / "sorted.bam", "wb") as f:                         # (bam_bytes: an @HD line without SO, so the header's members differ)
        f.write(bc.bam_bytes(CHROMS, sorted(recs, key=key_of), block=6000))
    run_filter(exe, d, str(tmp_path / "bsi"), ("-b", "-s", "-i"), tmp_path / "sorted.bam")
    run_filter(exe, d, str(tmp_path / "bi"), ("-b", "-i"), tmp_path / "sorted.bam")
    bam = "out_ALL.iteres.bam"
    assert sorted(os.listdir(tmp_path / "bsi")) == sorted(os.listdir(tmp_path / "bi"))
    a, b = open(tmp_path / "bsi" / bam, "rb").read(), open(tmp_path / "bi" / bam, "rb").read()
    sa, sb = bai.split_bam(a), bai.split_bam(b)
    first_a, first_b = sa[3], sb[3]
    assert a[first_a:] == b[first_b:] and sa[1] == sb[1] and len(sa[2]) > 2     # the record members, byte for byte
    text_a, text_b = header_parts(sa[4])[0], header_parts(sb[4])[0]
    assert text_a == py_header(text_b) != text_b
    ia, ib = bai.parse_bai(open(tmp_path / "bsi" / (bam + ".bai"), "rb").read()), bai.parse_bai(open(tmp_path / "bi" / (bam + ".bai"), "rb").read())
    shift = (first_a - first_b) << 16

    def moved(ref):
        return {"bins": {bn: [(x + shift, y + shift) for x, y in ch] for bn, ch in ref["bins"].items()},
                "meta": ref["meta"] and (ref["meta"][0] + shift, ref["meta"][1] + shift) + ref["meta"][2:],
                "lin": [v + shift if v else 0 for v in ref["lin"]]}
    assert ia == [moved(r) for r in ib]
    assert open(tmp_path / "bsi" / (bam + ".bai"), "rb").read() == bai.expected_for_file(a)[1]
