"""GPU: `filter -b -s -m`, the mates of the counted pairs joined to the sorted BAM on the device (include/iteres_amd.h
itx_bamout_mates_*, csrc/itx_bamout_mates.hip; the rule is csrc/itx_materule.h).
The oracle is Python and shares no code with the product (tests/matecase.py): wanted / candidate / match applied to struct-parsed
records, the chosen mates appended to the counted records in input order, and a stable sort by (tid, pos, reverse). Every case compares
the collected members' bytes (the host build of the member rule over payload-sized slices of the expected stream), the decoded record
sequence and, where an index is enabled, the index's bytes (tests/baicase.py) with it, and the wanted / found counters.
A step is ("run", records, rows): a device batch; ("host", records, counted rows or None): a host-route window, whose counted records go
to append_host and all of whose records go to mates_append_host, as host/out_bam.c does it.
A candidate stream beyond 2^32 bytes is not among the cases: DESIGN.md ("Mates of the counted pairs") says why."""
import ctypes as C

import numpy as np
import pytest

import baicase as bai
import bedcase as bc
import bgzfmemberhost as bm
import matecase as mc
from iteres_amd import engine as eng
from test_gpu_bamidx import regions, tensors
from test_gpu_bamout import rule   # noqa: F401  (fixture)
from test_gpu_bamout_annotate import table
from test_gpu_bamsort import split_records

pytestmark = pytest.mark.gpu

P = bai.PAYLOAD
M = 0
R1, R2, REV, MREV = 0x41, 0x81, 0x10, 0x20
L_REF = [1 << 20] * 4
_BASE = len(bc.record(qname=b"q\0", cigar=((M, 50),), aux=bc.tag("ZZ", "Z", b"\0")))
TAB7 = table(7)


def prec(tid, pos, flag, name, mtid=-1, mpos=-1, L=None):
    """a record at (tid, pos) whose mate is said to lie at (mtid, mpos); L: its exact length in bytes, made up by a Z tag"""
    qn = name + b"\0"
    if L is None:
        return bc.record(tid=tid, pos=pos, flag=flag, qname=qn, cigar=((M, 50),), mtid=mtid, mpos=mpos)
    pad = L - _BASE - (len(qn) - 2)
    assert pad >= 0, L
    r = bc.record(tid=tid, pos=pos, flag=flag, qname=qn, cigar=((M, 50),), mtid=mtid, mpos=mpos, aux=bc.tag("ZZ", "Z", bytes([65 + pos % 23]) * pad + b"\0"))
    assert len(r) == L
    return r


def pair(name, tid, p1, p2, mtid=None, L2=None):
    """(READ1, READ2) of a proper pair: READ1 forward at p1, READ2 reverse at p2 on mtid (default: the same reference)"""
    mtid = tid if mtid is None else mtid
    return prec(tid, p1, R1 | MREV, name, mtid, p2), prec(mtid, p2, R2 | REV, name, tid, p1, L=L2)


def drive(steps, l_ref=L_REF, first=0, cap=None, index=True, mates=True, tab=None, stream_bytes=0, level=None):
    """-> (members, counted records, their rows, every record seen, status, index bytes, stats, sort stats, mates stats)"""
    import torch
    bo = eng.Bamout(batch_capacity=cap or max([len(s[1]) for s in steps if s[0] == "run"] + [1]), stream_bytes=stream_bytes)
    try:
        if level is not None:
            bo.set_level(level)
        bo.sort_enable()
        if mates:
            bo.mates_enable()
        if tab is not None:
            bo.annotate_enable(*tab)
        if index:
            bo.index_enable(l_ref)
        counted, rows, seen = [], [], []
        for s in steps:
            if s[0] == "run":
                raw, off = tensors(s[1])
                bo.run(raw, off, torch.from_numpy(np.asarray(s[2], np.int32)).cuda())
                bo.wait_kernels()
                counted += [r for r, h in zip(s[1], s[2]) if h >= 0]
                rows += [h for h in s[2] if h >= 0]
            else:
                hit = s[2] if s[2] is not None else [0] * len(s[1])
                mine = [r for r, h in zip(s[1], hit) if h >= 0]
                mrows = [h for h in hit if h >= 0]
                if tab is not None:
                    if mates:
                        bo.mates_host_rows(mrows)
                    mine_bytes = b"".join(mc.rt.annotate_rows(mine, mrows, *tab))     # (the host route annotates what it counted itself)
                else:
                    mine_bytes = b"".join(mine)
                bo.append_host(mine_bytes)
                if mates:
                    bo.mates_append_host(b"".join(s[1]))
                counted += mine
                rows += mrows
            seen += s[1]
            assert bo.out == b"" and bo.stats()["members"] == 0            # nothing leaves during the pass
        got = bo.sort_all()
        status, idx, info = bo.index_finish(first) if index else (None, None, None)
        return got, counted, rows, seen, status, idx, bo.stats(), bo.sort_stats(), bo.mates_stats()
    finally:
        bo.close()


def check(rule, steps, l_ref=L_REF, first=0, cap=None, index=True, tab=None, stream_bytes=0):
    got, counted, rows, seen, status, idx, st, ss, ms_ = drive(steps, l_ref, first, cap, index, True, tab, stream_bytes)
    want, n_wanted, n_found = mc.expected(counted, seen, rows if tab is not None else None, tab)
    stream = b"".join(want)
    ms = bm.split_members(got)
    assert ms == rule.members(stream)                                      # 1. the members' bytes
    assert split_records(b"".join(bm.check_member(m) for m in ms)) == want   # 2. the decoded record sequence
    if index:                                                              # 3. the index's bytes
        assert status == bai.OK
        assert (status, idx) == bai.expected(l_ref, stream, [len(m) for m in ms], first)
    assert (ms_["wanted"], ms_["found"]) == (n_wanted, n_found)
    assert ms_["candidates"] == sum(mc.candidate(r) for r in seen) and ms_["candidate_bytes"] == sum(len(r) for r in seen if mc.candidate(r))
    assert ss["records"] == len(want) and st["records"] == len(counted) and st["carry"] == 0
    return got, want, counted, ms_


def hits(recs, row=0):
    """the rows of a device batch: READ1s and unpaired reads are counted, the others not"""
    return [row if (mc.fields(r)["flag"] & 0x41) != 0x1 and not mc.fields(r)["flag"] & 0x80 else -1 for r in recs]


# ---- shapes

def test_no_paired_record_gives_the_members_of_the_sort_alone(rule):
    recs = [prec(i % 3, 5000 - 7 * i, REV * (i % 2), b"u%d" % i) for i in range(300)]
    steps = [("run", recs[:200], [0] * 200), ("host", recs[200:], None)]
    got, want, counted, ms_ = check(rule, steps)
    assert ms_["candidates"] == ms_["wanted"] == 0
    assert got == drive(steps, mates=False)[0]


@pytest.mark.parametrize("order", ["behind", "in_front"])
def test_one_pair(rule, order):
    r1, r2 = pair(b"p", 1, 3000, 3200)
    recs = [r1, r2] if order == "behind" else [r2, r1]
    got, want, counted, ms_ = check(rule, [("run", recs, hits(recs))])
    assert want == [r1, r2] and ms_["found"] == 1


def test_the_mate_in_another_run_call(rule):
    r1, r2 = pair(b"p", 1, 3000, 2000)
    other = [prec(0, 10 * i, 0, b"s%d" % i) for i in range(5)]
    for a, b in ((r1, r2), (r2, r1)):
        got, want, counted, ms_ = check(rule, [("run", [a] + other, hits([a] + other)), ("run", other[:2] + [b], hits(other[:2] + [b]))], cap=8)
        assert r2 in want and want.index(r2) < want.index(r1) and ms_["found"] == 1


def test_the_mate_through_the_host_route_with_read1_by_the_device(rule):
    r1, r2 = pair(b"p", 2, 100, 400)
    got, want, counted, ms_ = check(rule, [("run", [r1], [3]), ("host", [prec(0, 1, 0, b"x"), r2], [0, -1])])
    assert want[-2:] == [r1, r2] and ms_["found"] == 1


def test_read1_through_the_host_route_with_the_mate_by_the_device(rule):
    r1, r2 = pair(b"p", 2, 100, 400)
    got, want, counted, ms_ = check(rule, [("run", [r2, prec(0, 9, 0, b"x")], [-1, 0]), ("host", [r1], [0])])
    assert want[-2:] == [r1, r2] and ms_["found"] == 1


@pytest.mark.parametrize("n", [255, 256, 257])
def test_pairs_around_the_tile(rule, n):
    prs = [pair(b"t%d" % i, i % 3, 90_000 - 50 * i, 90_000 - 50 * i + 30 + i % 17, L2=60 + i % 90) for i in range(n)]
    recs = [r for p in prs for r in p]
    got, want, counted, ms_ = check(rule, [("run", recs[:n], hits(recs[:n])), ("run", recs[n:], hits(recs[n:]))], cap=n)
    assert ms_["found"] == n and len(want) == 2 * n


@pytest.fixture(scope="module")
def collision():
    return mc.collide(b"c")


def test_equal_hash_at_one_place_is_not_a_match(rule, collision):
    a, b = collision
    r1, _ = pair(a, 1, 100, 400)
    _, wrong = pair(b, 1, 100, 400)
    assert mc.key_wanted(r1) == mc.key_candidate(wrong) and not mc.match(r1, wrong)
    got, want, counted, ms_ = check(rule, [("run", [r1, wrong], [0, -1])])
    assert want == [r1] and (ms_["wanted"], ms_["found"], ms_["candidates"]) == (1, 0, 1)
    _, right = pair(a, 1, 100, 400)
    got, want, counted, ms_ = check(rule, [("run", [wrong, r1, wrong, right], [-1, 0, -1, -1])])     # the walk passes the colliding ones
    assert want == [r1, right] and ms_["found"] == 1


def test_same_name_elsewhere_is_not_a_match(rule):
    r1, r2 = pair(b"p", 1, 100, 400)
    other_pos = prec(1, 401, R2 | REV, b"p", 1, 100)
    other_tid = prec(2, 400, R2 | REV, b"p", 1, 100)
    got, want, counted, ms_ = check(rule, [("run", [other_pos, r1, other_tid], [-1, 0, -1])])
    assert want == [r1] and (ms_["wanted"], ms_["found"], ms_["candidates"]) == (1, 0, 2)


def test_the_mate_on_another_reference(rule):
    r1, r2 = pair(b"p", 3, 100, 77, mtid=0)
    decoy = prec(3, 77, R2 | REV, b"p", 3, 100)                             # the same place on READ1's own reference
    got, want, counted, ms_ = check(rule, [("run", [decoy, r1, r2], [-1, 0, -1])])
    assert want == [r2, r1] and ms_["found"] == 1


def test_of_two_matching_candidates_the_first_is_emitted(rule):
    r1, r2 = pair(b"p", 1, 100, 400)
    second = prec(1, 400, R2, b"p", 1, 100, L=99)                           # matches as well; it differs in strand and length
    got, want, counted, ms_ = check(rule, [("run", [r2, r1], [-1, 0]), ("run", [second], [-1])], cap=2)
    assert want == [r1, r2] and ms_["candidates"] == 2
    got, want, counted, ms_ = check(rule, [("run", [second, r1], [-1, 0]), ("host", [r2], [-1])], cap=2)
    assert want == [r1, second]


@pytest.mark.parametrize("annotate", [False, True])
def test_two_read1s_that_want_one_candidate(rule, annotate):
    r1, r2 = pair(b"p", 1, 100, 400)
    again = prec(1, 90, R1 | MREV, b"p", 1, 400)                           # a second READ1 of that name that points at the same mate
    steps = [("run", [again, r2, r1], [5, -1, 2])]
    got, want, counted, ms_ = check(rule, steps, tab=TAB7 if annotate else None)
    assert len(want) == 3 and (ms_["wanted"], ms_["found"]) == (2, 2)
    if annotate:
        mate = [w for w in want if mc.fields(w)["flag"] & 0x80][0]
        assert mc.rt.strip(mate) == (r2, mc.rt.strip(want[0])[1]) and mc.rt.strip(want[0])[0] == again      # the tags of `again`'s row, 5
        assert mc.rt.strip(mate)[1] != mc.rt.strip(want[1])[1]


def test_annotated_mates_from_both_routes(rule):
    prs = [pair(b"a%d" % i, i % 2, 1000 + 10 * i, 5000 - 10 * i, L2=70 + i) for i in range(40)]
    dev = [r for p in prs[:20] for r in p]
    host = [r for p in prs[20:] for r in p][::-1]
    steps = [("run", dev, [i % 7 if i % 2 == 0 else -1 for i in range(40)]), ("host", host, [-1 if mc.fields(r)["flag"] & 0x80 else 1 + k % 6 for k, r in enumerate(host)])]
    got, want, counted, ms_ = check(rule, steps, tab=TAB7)
    assert ms_["found"] == 40 and len(want) == 80


def test_a_counted_read1_without_a_mate_is_still_written(rule):
    r1, r2 = pair(b"p", 1, 100, 400)
    got, want, counted, ms_ = check(rule, [("run", [r1, prec(1, 50, 0, b"s")], [0, 0])])
    assert len(want) == 2 and (ms_["wanted"], ms_["found"], ms_["candidates"]) == (1, 0, 0)


@pytest.mark.parametrize("what", ["0x100", "0x800", "0x4", "0x8", "read1", "unpaired"])
def test_a_record_each_clause_of_candidate_excludes(rule, what):
    r1, r2 = pair(b"p", 1, 100, 400)
    flag = {"0x100": R2 | REV | 0x100, "0x800": R2 | REV | 0x800, "0x4": R2 | REV | 0x4, "0x8": R2 | REV | 0x8, "read1": R1 | 0x80 | REV, "unpaired": REV | 0x80}[what]
    no = prec(1, 400, flag, b"p", 1, 100)
    assert not mc.candidate(no) and mc.fields(no)["pos"] == mc.fields(r1)["mpos"]
    got, want, counted, ms_ = check(rule, [("run", [no, r1], [-1, 0])])
    assert want == [r1] and (ms_["wanted"], ms_["found"], ms_["candidates"]) == (1, 0, 0)


def test_a_counted_single_end_with_an_unmapped_mate_wants_nothing(rule):
    single = prec(1, 100, R1 | 0x8, b"p", 1, 100)
    mate = prec(1, 100, R2 | 0x4, b"p", 1, 100)
    looks_right = prec(1, 100, R2 | REV, b"p", 1, 100)
    got, want, counted, ms_ = check(rule, [("run", [single, mate, looks_right], [0, -1, -1])])
    assert want == [single] and (ms_["wanted"], ms_["candidates"]) == (0, 1)


def test_an_uncounted_read1_leaves_no_trace(rule):
    prs = [pair(b"n%d" % i, 0, 100 + i, 900 + i) for i in range(300)]
    recs = [r for p in prs for r in p]
    rows = [(0 if i % 3 == 0 else -1) if k == 0 else -1 for i in range(300) for k in range(2)]
    got, want, counted, ms_ = check(rule, [("run", recs, rows)])
    assert len(want) == 200 and (ms_["wanted"], ms_["found"], ms_["candidates"]) == (100, 100, 300)
    got, want, counted, ms_ = check(rule, [("run", recs, [-1] * 600)])
    assert got == b"" and want == [] and ms_["candidates"] == 300


def test_equal_sort_keys_counted_first_then_mates_each_in_input_order(rule):
    prs = [(prec(0, 500, R1, b"e%d" % i, 0, 500), prec(0, 500, R2, b"e%d" % i, 0, 500)) for i in range(6)]
    order = [prs[0][1], prs[0][0], prs[1][0], prs[2][1], prs[1][1], prs[3][0], prs[2][0], prs[4][1], prs[5][1], prs[5][0], prs[4][0], prs[3][1]]
    got, want, counted, ms_ = check(rule, [("run", order[:5], hits(order[:5])), ("host", order[5:9], hits(order[5:9])), ("run", order[9:], hits(order[9:]))])
    assert want == [r for r in order if mc.fields(r)["flag"] & 0x40] + [r for r in order if mc.fields(r)["flag"] & 0x80]


def test_a_mate_of_three_payloads_and_17_bytes(rule):
    prs = [pair(b"l%d" % i, 0, 1000 + 10 * i, 50_000 + i, L2=300) for i in range(40)] + [pair(b"long", 0, 7, 20, L2=3 * P + 17)]
    recs = [r for p in prs for r in p]
    got, want, counted, ms_ = check(rule, [("run", recs, hits(recs))], first=3)
    assert want[1] == prs[-1][1] and len(want[1]) == 3 * P + 17 and ms_["found"] == 41


# ---- 70 001 records

def big_case():
    """70 001 records: 20 000 proper pairs whose READ1 is counted (some 800 of them have no mate in the input), READ2s, and single-end
    reads of which a third is counted, in a seeded shuffle so that a mate lies before or behind its READ1, often in another call; three
    `run` calls (4 096, 4 095 and 4 000 records) with host-route windows before, between and after them. Positions repeat, so that equal
    keys meet across the calls."""
    l_ref = [4_000_000, 1000, 3_700_000, 5_000_000]
    rng = np.random.default_rng(29)
    recs, rows = [], []
    for k in range(20_000):
        tid = (0, 2, 3)[int(rng.integers(3))]
        p1 = int(rng.integers(0, 30_000)) * 100
        p2 = max(0, p1 + int(rng.integers(-400, 400)))
        mtid = tid if k % 50 != 1 else (0, 2, 3)[int(rng.integers(3))]
        r1, r2 = pair(b"r%d" % k, tid, p1, p2, mtid=mtid, L2=90 + k % 160 if k % 3 == 0 else None)
        recs.append(r1)
        rows.append(k % 7)
        if k % 25:
            recs.append(r2)
            rows.append(-1)
    n_single = 70_001 - len(recs)
    for k in range(n_single):
        recs.append(prec((0, 2, 3)[int(rng.integers(3))], int(rng.integers(0, 30_000)) * 100, REV * int(rng.integers(2)), b"s%d" % k))
        rows.append(3 if k % 3 == 0 else -1)
    perm = rng.permutation(len(recs))
    recs, rows = [recs[i] for i in perm], [rows[i] for i in perm]
    cuts = [0, 18_000, 22_096, 40_096, 44_191, 62_191, 66_191, len(recs)]
    kinds = ["host", "run", "host", "run", "host", "run", "host"]
    steps = [(kind, recs[cuts[c]:cuts[c + 1]], rows[cuts[c]:cuts[c + 1]]) for c, kind in enumerate(kinds)]
    assert sum(len(s[1]) for s in steps) == 70_001
    return l_ref, steps


@pytest.fixture(scope="module")
def big(rule):
    l_ref, steps = big_case()
    first = 3000
    got, counted, rows, seen, status, idx, st, ss, ms_ = drive(steps, l_ref, first, cap=4096, stream_bytes=1)
    want, n_wanted, n_found = mc.expected(counted, seen)
    return l_ref, first, got, want, counted, seen, status, idx, st, ss, ms_, n_wanted, n_found


def test_three_runs_and_host_windows(rule, big):
    l_ref, first, got, want, counted, seen, status, idx, st, ss, ms_, n_wanted, n_found = big
    stream = b"".join(want)
    ms = bm.split_members(got)
    assert ms == rule.members(stream)
    assert split_records(b"".join(bm.check_member(m) for m in ms)) == want
    assert (ms_["wanted"], ms_["found"]) == (n_wanted, n_found) == (20_000, 19_200)
    assert len(want) == len(counted) + 19_200 and ss["records"] == len(want) and ss["rounds"] == -(-len(want) // 4096)
    assert st["batches"] == 3 and st["host_batches"] == 4
    assert ms_["grows"] >= 1 and st["grows"] >= 3 and ss["pool_grows"] >= 1, (ms_, st, ss)     # the candidate store from its minimum; the held stream; the pool
    assert ms_["gather_ms"] > 0 and ms_["join_ms"] > 0
    at = {bytes(r): i for i, r in enumerate(seen)}
    sides = [at[bytes(c)] < at[bytes(counted[i])] for c, i in mc.choose(counted, seen)[0]]
    assert sum(sides) > 5000 and len(sides) - sum(sides) > 5000            # mates on both sides of their READ1


def test_the_index_of_the_stream_with_mates(big):
    l_ref, first, got, want, counted, seen, status, idx, st, ss, ms_, n_wanted, n_found = big
    stream = b"".join(want)
    assert status == bai.OK
    assert (status, idx) == bai.expected(l_ref, stream, [len(m) for m in bm.split_members(got)], first)


def test_fetch_equivalence(big):
    """300 seeded regions through the index by the restatement's independent reader against a linear scan"""
    l_ref, first, got, want, counted, seen, status, idx, st, ss, ms_, n_wanted, n_found = big
    stream = b"".join(want)
    sizes = [size for off, size, isize in bai.member_walk(got)]
    coff = np.cumsum([0] + sizes)
    ustart = {first + int(coff[k]): min(k * P, len(stream)) for k in range(len(sizes) + 1)}
    parsed = bai.parse_bai(idx)
    recs = bai.records_of(stream)
    r_tid, r_pos, r_end, r_at, _ = np.array(recs, np.int64).T
    n_hit = 0
    for tid, beg, end in regions(l_ref, recs, seed=20):
        found = bai.fetch(parsed, stream, ustart, tid, beg, end)
        assert found == set(r_at[(r_tid == tid) & (r_pos < end) & (r_end > beg)].tolist()), (tid, beg, end)
        n_hit += bool(found)
    assert n_hit >= 150, n_hit


# ---- state and argument checks

def test_state_and_argument_checks(rule):
    L = eng.load()
    s = eng.BamoutMatesStats()
    assert L.itx_bamout_mates_enable(None) == -1 and L.itx_bamout_mates_append_host(None, b"", 0) == -1 and L.itx_bamout_mates_get_stats(None, C.byref(s)) == -1
    assert L.itx_bamout_mates_host_rows(None, None, 0) == -1
    bo = eng.Bamout(batch_capacity=16)
    assert L.itx_bamout_mates_get_stats(bo._h, None) == -1
    assert L.itx_bamout_mates_enable(bo._h) == -5 and b"sort_enable" in L.itx_last_error()         # without sort_enable
    one = prec(0, 5, R2 | REV, b"m", 0, 1)
    assert L.itx_bamout_mates_append_host(bo._h, one, len(one)) == -5 and b"mates_enable" in L.itx_last_error()
    bo.sort_enable()
    assert L.itx_bamout_mates_enable(bo._h) == 0
    assert L.itx_bamout_mates_enable(bo._h) == -5 and b"twice" in L.itx_last_error()
    assert L.itx_bamout_mates_append_host(bo._h, None, 5) == -1
    for bad in (one[:-1], one + b"\1\0", b"\xff\xff\xff\x7f" + one):       # not whole records: nothing is appended
        assert L.itx_bamout_mates_append_host(bo._h, bad, len(bad)) == -1 and b"whole records" in L.itx_last_error()
    assert bo.mates_stats()["candidates"] == 0
    bo.mates_append_host(one + prec(0, 6, 0, b"single") + one)
    assert bo.mates_stats()["candidates"] == 2 and bo.mates_stats()["candidate_bytes"] == 2 * len(one)
    r1 = prec(0, 1, R1 | MREV, b"m", 0, 5)
    bo.append_host(r1)
    assert bo.sort_next() is False
    assert bo.mates_stats()["found"] == 1
    assert L.itx_bamout_mates_append_host(bo._h, one, len(one)) == -5 and L.itx_bamout_mates_host_rows(bo._h, None, 0) == -5    # after the replay
    assert split_records(b"".join(bm.check_member(m) for m in bm.split_members(bytes(bo.out)))) == [r1, one]
    bo.close()
    late = eng.Bamout(batch_capacity=16)                                   # after the first batch
    late.sort_enable()
    late.append_host(r1)
    assert L.itx_bamout_mates_enable(late._h) == -5 and b"begun" in L.itx_last_error()
    late.close()
    ann = eng.Bamout(batch_capacity=16)                                    # with tags a host-route READ1 needs its row
    ann.sort_enable()
    ann.mates_enable()
    ann.annotate_enable(*TAB7)
    tagged = b"".join(mc.rt.annotate_rows([r1], [2], *TAB7))
    assert L.itx_bamout_append_host(ann._h, tagged, len(tagged)) == -5 and b"mates_host_rows" in L.itx_last_error()
    rows = np.array([7], np.int32)
    assert L.itx_bamout_mates_host_rows(ann._h, rows.ctypes.data, 1) == -1 and b"row 7" in L.itx_last_error()
    ann.mates_host_rows([2, 2])
    assert L.itx_bamout_append_host(ann._h, tagged, len(tagged)) == -1 and b"one per record" in L.itx_last_error()
    ann.mates_host_rows([2])
    ann.append_host(tagged)
    ann.mates_append_host(one)
    assert ann.sort_next() is False
    out = split_records(b"".join(bm.check_member(m) for m in bm.split_members(bytes(ann.out))))
    assert out == mc.rt.annotate_rows([r1, one], [2, 2], *TAB7)
    ann.close()
