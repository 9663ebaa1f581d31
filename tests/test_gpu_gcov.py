"""GPU: the genome coverage of `filter -G` at the C ABI (include/iteres_amd.h itx_gcov_*, csrc/itx_gcov.hip). Records go in as device
arrays with their chosen rows (itx_gcov_run) or as intervals the caller derived (itx_gcov_add_host); the two bedGraph texts are
compared byte for byte with the model of tests/gcovcase.py over the intervals that tests/goldencase.py derive_py gives (the
suite's own statement of generic.c:764-905). The cases sit on the kernels' constants: a tile of the dense pass is GC_TILE = 8192
slots swept in 8 rows of 1024 (one 16-byte vector of 4 slots per lane), a tile of text is 256 change points."""
import numpy as np
import pytest

import gcovcase as gv
import goldencase as gc
from iteres_amd import engine as eng

pytestmark = pytest.mark.gpu

TILE, SUB, VEC = 8192, 1024, 4                # csrc/itx_gcov.hip GC_TILE, GC_SUB, slots per 16-byte load
TXT_TILE = 256                                # GC_TXT_TILE
LINE_EXTRA = 34                               # GC_LINE_EXTRA: a round takes max(1, round_bytes // (longest name + 34)) change points
Q = gv.MAPQ_MIN
P0 = dict(extension=0, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False, mapq_min=Q)


def recs(rows):
    """rows: (tid, pos, tmpend, mapq, bam flag, mpos, isize, hit) -> dict of arrays"""
    a = np.asarray(rows, np.int64).reshape(-1, 8)
    return dict(tid=a[:, 0].astype(np.int32), pos=a[:, 1].astype(np.int32), tmpend=a[:, 2].astype(np.int32), mapq=a[:, 3].astype(np.uint8),
                flag=a[:, 4].astype(np.uint16), mpos=a[:, 5].astype(np.int32), isize=a[:, 6].astype(np.int32), hit=a[:, 7].astype(np.int32))


def se(tid, start, end, mapq=37, hit=0, flag=0):
    return (tid, start, end, mapq, flag, -1, 0, hit)


def counted(chroms, rd, p, t2c=None, nolookup=None):
    """the model's input: (chromosome, start, end, mapq) of every record that must add"""
    t2c = list(range(len(chroms))) if t2c is None else t2c
    size = [s for _, s in chroms]
    out = []
    for i in range(len(rd["tid"])):
        if rd["hit"][i] < 0 or (nolookup is not None and nolookup[i]):
            continue
        iv = gc.derive_py(p, t2c, size, rd, i)
        if iv is None:
            continue
        s, e, _ = iv
        c = t2c[int(rd["tid"][i])]
        if size[c] > 2 and 0 <= s < e <= size[c] - 1:
            out.append((chroms[c][0], s, e, int(rd["mapq"][i])))
    return out


def slices(rd, lo, hi):
    return {k: v[lo:hi] for k, v in rd.items()}


def feed_run(g, rd, nolookup=None):
    import torch
    f5 = eng.flag5(rd["flag"])
    if nolookup is not None:
        f5 = f5 | np.where(nolookup, eng.F5_NOLOOKUP, 0).astype(np.uint8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = [dev(rd[k]) for k in ("hit", "tid", "pos", "tmpend", "mapq")] + [dev(f5), dev(rd["mpos"]), dev(rd["isize"])]
    if len(rd["tid"]):
        g.run(*t)
        g.wait_kernels()


def feed_host(g, chroms, rd, p, t2c=None):
    idx = {n: i for i, (n, _) in enumerate(chroms)}
    c = counted(chroms, rd, p, t2c)
    g.add_host([idx[x[0]] for x in c], [x[1] for x in c], [x[2] for x in c], [x[3] >= Q for x in c])


def finish(g, chroms, round_bytes=0):
    names = [n for n, _ in chroms]
    order = sorted(range(len(names)), key=lambda i: names[i].encode())
    g.finish(order, names, round_bytes)
    (a, pa), (u, pu) = g.text(0), g.text(1)
    st = g.stats()
    g.close()
    return a, u, st, pa, pu


def cover(chroms, rd, p=P0, t2c=None, nolookup=None, round_bytes=0):
    g = eng.Gcov([s for _, s in chroms], dict(p), batch_capacity=max(len(rd["tid"]), 1))
    g.set_tidmap(list(range(len(chroms))) if t2c is None else t2c)
    feed_run(g, rd, nolookup)
    return finish(g, chroms, round_bytes)


def check(chroms, rd, p=P0, t2c=None, nolookup=None, round_bytes=0):
    a, u, st, pa, pu = cover(chroms, rd, p, t2c, nolookup, round_bytes)
    want = counted(chroms, rd, p, t2c, nolookup)
    wa, wu = gv.both(want)
    assert a == wa and u == wu
    assert st["records"] == len(want) and st["records_uniq"] == sum(c[3] >= Q for c in want)
    assert st["lines"] == [wa.count(b"\n"), wu.count(b"\n")] and st["bytes"] == [len(wa), len(wu)]
    return a, u, st, pa, pu


# ---- tile boundaries

def test_change_points_on_either_side_of_a_tile_boundary():
    ch = [("c", 5 * TILE + 100)]
    rows = [se(0, TILE - 1, TILE), se(0, 2 * TILE - 3, 2 * TILE - 1), se(0, 3 * TILE, 3 * TILE + 1), se(0, 4 * TILE - 1, 4 * TILE + 1),
            se(0, SUB - 1, SUB), se(0, 3 * SUB, 3 * SUB + 2), se(0, 0, 1), se(0, 5 * TILE + 90, 5 * TILE + 99)]
    a, u, st, _, _ = check(ch, recs(rows))
    assert b"c\t%d\t%d\t1\n" % (TILE - 1, TILE) in a and b"c\t%d\t%d\t1\n" % (4 * TILE - 1, 4 * TILE + 1) in a and a.startswith(b"c\t0\t1\t1\n")


def test_a_run_over_several_tiles_without_a_change_point_inside():
    ch = [("c", 7 * TILE)]
    rows = [se(0, TILE + 10, 5 * TILE + 3), se(0, 10, 6 * TILE), se(0, 5 * TILE + 3, 5 * TILE + 9)]
    a, _, st, _, _ = check(ch, recs(rows))
    assert a == b"c\t10\t%d\t1\nc\t%d\t%d\t2\nc\t%d\t%d\t1\n" % (TILE + 10, TILE + 10, 5 * TILE + 9, 5 * TILE + 9, 6 * TILE)
    assert st["points"][0] == 4


@pytest.mark.parametrize("base", [0, SUB - VEC, TILE - VEC, TILE])
def test_offsets_that_are_no_multiple_of_a_vector_next_to_ones_that_are(base):
    ch = [("c", 3 * TILE + 5)]
    rows = [se(0, base + 4 + k, base + 40 + 2 * k) for k in range(9)] + [se(0, base + 41, base + 42), se(0, base + 43, base + 44)]
    check(ch, recs(rows))


def test_random_reads_over_many_tiles():
    rng = np.random.default_rng(11)
    ch = [("b", 4 * TILE + 1), ("a", 9 * TILE - 1)]
    n = 3000
    tid = rng.integers(0, 2, n)
    size = np.array([s for _, s in ch])[tid]
    pos = (rng.random(n) * (size - 3)).astype(np.int64)
    end = np.minimum(pos + rng.integers(1, 300, n), size - 1)
    rows = [se(int(t), int(s), int(e), mapq=int(q), hit=int(h)) for t, s, e, q, h in zip(tid, pos, end, rng.choice([0, 9, 10, 37], n), rng.choice([-1, 0, 7], n))]
    a, u, st, _, _ = check(ch, recs(rows))
    assert a.startswith(b"a\t") and a.rstrip(b"\n").split(b"\n")[-1].startswith(b"b\t") and 0 < len(u) < len(a)


# ---- chromosome boundaries

def test_neighbouring_chromosomes_do_not_merge_and_a_missing_one_takes_no_slots():
    # in the array: A (1000), X (size 2: missing, no slots), T (size 3), B (1003, starts on a slot that follows T's padding), Z
    ch = [("zA", 1000), ("mX", 2), ("yT", 3), ("aB", 1003), ("kZ", 5000)]
    rows = [se(0, 990, 999), se(2, 0, 2), se(3, 0, 7), se(3, 1000, 1002), se(4, 0, 4999), se(4, 4990, 4999), se(1, 0, 1)]
    a, u, st, _, _ = cover(ch, recs(rows))
    assert a == (b"aB\t0\t7\t1\naB\t1000\t1002\t1\nkZ\t0\t4990\t1\nkZ\t4990\t4999\t2\nyT\t0\t2\t1\nzA\t990\t999\t1\n")
    assert a == gv.bedgraph([("zA", 990, 999), ("yT", 0, 2), ("aB", 0, 7), ("aB", 1000, 1002), ("kZ", 0, 4999), ("kZ", 4990, 4999)]) == u
    assert st["records"] == 6 and st["out_of_range"] == 1                   # the read on the missing chromosome has no interval
    assert st["slots"] == 1000 + 4 + 1004 + 5000


def test_a_chromosome_of_size_three_alone():
    a, u, st, _, _ = check([("c", 3)], recs([se(0, 0, 2), se(0, 1, 2)]))
    assert a == b"c\t0\t1\t1\nc\t1\t2\t2\n"
    assert check([("c", 3)], recs([se(0, 0, 2), se(0, 1, 2), se(0, 0, 1)]))[0] == b"c\t0\t2\t2\n"      # equal depths on both sides: one line


def test_lifecycle():
    """made and destroyed with no call between; then made, used at the smallest shape here (both routes, the text rounds, the bigWig
    content) and destroyed, twice in one process: what a double free or a buffer freed under a running stream would break"""
    eng.Gcov([3], dict(P0), batch_capacity=1).close()
    ch, rd = [("c", 3)], recs([se(0, 0, 2), se(0, 1, 2)])
    for _ in range(2):
        g = eng.Gcov([3], dict(P0), batch_capacity=2)
        g.set_tidmap([0])
        g.set_tidmap([0])                                                  # the map is replaced: the old one goes
        feed_run(g, rd)
        feed_host(g, ch, rd, P0)
        g.finish([0], ["c"])
        g.bigwig_build(0)
        assert g.bigwig(0)["n_items"] == 2
        assert g.text(0)[0] == g.text(1)[0] == b"c\t0\t1\t2\nc\t1\t2\t4\n"
        g.close()


# ---- abutting, identical, nested

def test_abutting_identical_and_nested_reads():
    ch = [("c", 1000)]
    assert check(ch, recs([se(0, 10, 20), se(0, 20, 35)]))[0] == b"c\t10\t35\t1\n"
    assert check(ch, recs([se(0, 10, 20), se(0, 10, 20)]))[0] == b"c\t10\t20\t2\n"
    assert check(ch, recs([se(0, 10, 40), se(0, 20, 30)]))[0] == b"c\t10\t20\t1\nc\t20\t30\t2\nc\t30\t40\t1\n"


def test_pile_up_and_depths_of_one_to_five_digits():
    ch = [("c", 2 * TILE)]
    rows = [se(0, 100, 150)] * 70000 + [se(0, 120, 130)]
    for k, depth in enumerate((1, 12, 345, 6789)):
        rows += [se(0, 1000 + 100 * k, 1050 + 100 * k)] * depth
    a, _, st, _, _ = check(ch, recs(rows))
    assert b"c\t120\t130\t70001\n" in a and b"c\t100\t120\t70000\n" in a
    assert [l.split(b"\t")[3] for l in a.splitlines()] == [b"70000", b"70001", b"70000", b"1", b"12", b"345", b"6789"]


def test_nine_digit_positions():
    size = 100_000_010
    ch = [("chrBig", size), ("chr0", 50)]
    rows = [se(0, 99_999_990, size - 1), se(0, 100_000_000, 100_000_005), se(0, 5, 12), se(1, 1, 49), se(0, 99_999_999, 100_000_001)]
    a, _, st, _, _ = check(ch, recs(rows))
    assert b"chrBig\t100000001\t100000005\t2\n" in a and a.endswith(b"chrBig\t100000005\t100000009\t1\n")


def test_unique_and_all_differ_at_the_threshold():
    ch = [("c", 500)]
    rows = [se(0, 10, 60, mapq=Q - 1), se(0, 10, 60, mapq=Q), se(0, 30, 90, mapq=0), se(0, 200, 210, mapq=255)]
    a, u, _, _, _ = check(ch, recs(rows))
    assert a == b"c\t10\t30\t2\nc\t30\t60\t3\nc\t60\t90\t1\nc\t200\t210\t1\n" and u == b"c\t10\t60\t1\nc\t200\t210\t1\n"


# ---- records that must add nothing

def test_no_hit_and_nolookup_add_nothing():
    ch = [("c", 500)]
    rd = recs([se(0, 10, 60, hit=-1), se(0, 20, 70, hit=3), se(0, 30, 80, hit=5), se(0, 40, 90, hit=-1)])
    a, u, st, _, _ = check(ch, rd, nolookup=np.array([False, False, True, False]))
    assert a == b"c\t20\t70\t1\n" and st["records"] == 1 and st["out_of_range"] == 0


def test_intervals_out_of_range_through_add_host_are_counted_and_write_nothing():
    ch = [("c", 100), ("d", 2), ("e", 40)]
    g = eng.Gcov([s for _, s in ch], dict(P0))
    g.set_tidmap([0, 1, 2])
    chrom = [0, 0, 0, 0, -1, 3, 1, 2, 2, 0, 2]
    start = [10, 5, 50, 0xfffffff0, 1, 1, 0, 39, 0, 98, 30]
    end = [100, 5, 40, 0xfffffff8, 2, 2, 1, 40, 0xffffffff, 99, 39]
    ok = [False] * 9 + [True, True]                                          # end > size - 1; empty; reversed; far outside; no such chromosome (twice);
    g.add_host(chrom, start, end, [1] * len(chrom))                         # a missing chromosome; end == size; end 2^32 - 1
    assert g.stats()["out_of_range"] == 9 and g.stats()["records"] == 2
    a, u, st, _, _ = finish(g, ch)
    assert a == u == b"c\t98\t99\t1\ne\t30\t39\t1\n" and st["out_of_range"] == 9 and ok.count(True) == st["records"]


def test_a_hit_whose_record_has_no_interval_is_counted_as_out_of_range():
    ch = [("c", 100)]
    rd = recs([se(0, 10, 20), se(0, 10, 20, flag=0x4), se(5, 10, 20), se(0, 50, 50), se(0, 99, 120)])    # unmapped; no such tid; empty; start == size - 1
    a, _, st, _, _ = cover(ch, rd)
    assert a == b"c\t10\t20\t1\n" and st["records"] == 1 and st["out_of_range"] == 4


# ---- paired reads, -T, -E

def paired_rows():
    R1, R2, PAIRED, REV, MUN = 0x40, 0x80, 0x1, 0x10, 0x8
    return [
        (0, 1000, 1050, 37, PAIRED | R1, 1200, 250, 0),                     # isize > 0: [pos, pos + isize)
        (0, 1200, 1250, 37, PAIRED | R1 | REV, 1000, -250, 0),              # isize < 0: starts at mpos
        (0, 3000, 3050, 3, PAIRED | R2, 2800, -250, 0),                     # READ2 of a proper pair: only with -T
        (0, 4000, 4050, 37, PAIRED | R1, 4100, 600, 0),                     # insert longer than -I
        (0, 5000, 5050, 37, PAIRED | R1 | MUN, -1, 0, 0),                   # mate unmapped: single end unless -D
        (0, 60, 100, 37, REV, -1, 0, 0),                                    # '-' strand, -E 150 clamps the start to 0
        (0, 7000, 7036, 9, 0, -1, 0, 0),                                    # '+' strand, extended
        (0, 9950, 9990, 37, 0, -1, 0, 0),                                   # '+' strand, the extension is cut at size - 1
        (0, 8000, 8040, 37, PAIRED | R1, 7800, 0, 0),                       # isize 0
        (0, 9900, 9950, 37, PAIRED | R1, 9990, 400, 0),                     # pos + isize beyond the chromosome: cut at size - 1
    ]


@pytest.mark.parametrize("p", [dict(), dict(extension=150), dict(treat_pe_as_se=True), dict(treat_pe_as_se=True, extension=150), dict(discard_half_mapped=True),
                               dict(isize_max=700, extension=30)], ids=["E0", "E150", "T", "T_E150", "D", "I700_E30"])
def test_paired_reads_treat_and_extension(p):
    ch = [("c", 10_000)]
    q = dict(P0, **p)
    a, u, st, _, _ = check(ch, recs(paired_rows()), q)
    if p == dict():
        assert b"c\t1000\t1250\t2\n" in a                                   # both mates of the first pair name one fragment
    if p == dict(extension=150):
        assert a.startswith(b"c\t0\t100\t1\n") and b"c\t7000\t7150\t1\n" in a and a.endswith(b"c\t9950\t9999\t2\n") and b"7000" not in u
    assert st["out_of_range"] == len(paired_rows()) - st["records"]          # (every row carries a hit: a record without an interval is counted)


# ---- both add routes

def test_run_and_add_host_interleaved_equal_one_route():
    rng = np.random.default_rng(3)
    ch = [("b", 3 * TILE), ("a", 2 * TILE + 7)]
    n = 900
    tid = rng.integers(0, 2, n)
    size = np.array([s for _, s in ch])[tid]
    pos = (rng.random(n) * (size - 3)).astype(np.int64)
    rows = [se(int(t), int(s), int(min(s + w, z - 1)), mapq=int(q), hit=int(h))
            for t, s, w, z, q, h in zip(tid, pos, rng.integers(1, 200, n), size, rng.choice([0, 10, 37], n), rng.choice([-1, 2], n))]
    rd = recs(rows)
    one = check(ch, rd)
    g = eng.Gcov([s for _, s in ch], dict(P0), batch_capacity=400)
    g.set_tidmap([0, 1])
    feed_run(g, slices(rd, 0, 300))
    feed_host(g, ch, slices(rd, 300, 650), P0)
    feed_run(g, slices(rd, 650, n))
    a, u, st, _, _ = finish(g, ch)
    assert (a, u) == one[:2] and st["batches"] == 2 and st["host_batches"] == 1 and st["records"] == one[2]["records"]
    g = eng.Gcov([s for _, s in ch], dict(P0))
    g.set_tidmap([0, 1])
    feed_host(g, ch, rd, P0)
    assert finish(g, ch)[:2] == one[:2]


# ---- rounds

def test_rounds_are_cut_at_line_ends_and_change_nothing():
    ch = [("c", 4 * TILE)]
    rows = [se(0, 100 + 150 * k, 160 + 150 * k + (k % 7)) for k in range(200)]          # 200 lines, 400 change points
    rd = recs(rows)
    one = check(ch, rd)
    assert one[0].count(b"\n") == 200 and one[2]["rounds"] == [1, 1] and one[2]["points"] == [400, 400]
    per = 199                                                               # rounds of 199, 199 and 2 points: the last one is a start and its end
    a, u, st, pa, pu = check(ch, rd, round_bytes=per * (1 + LINE_EXTRA))
    assert (a, u) == one[:2] and st["rounds"] == [3, 3] and len(pa) == 3
    assert one[0][:pa[0]].endswith(b"\n") and one[0][:pa[0] + pa[1]].endswith(b"\n") and one[0][pa[0] + pa[1]:].count(b"\n") == 1
    assert one[0][:pa[0]].count(b"\n") == 100                                # (the line of point 198 ends at point 199, in the next round)
    a, u, st, pa, pu = check(ch, rd, round_bytes=1)                          # a round is one change point: a line, or nothing
    assert (a, u) == one[:2] and st["rounds"] == [400, 400] and sorted(set(pa)) == sorted({0} | {len(l) + 1 for l in one[0].splitlines()})


def test_more_lines_than_a_tile_of_text():
    ch = [("chrLongerName_1", 6 * TILE)]
    rows = [se(0, 10 + 40 * k, 30 + 40 * k + (k % 11), mapq=37 if k % 3 else 0) for k in range(3 * TXT_TILE + 5)]
    check(ch, recs(rows))
    check(ch, recs(rows), round_bytes=(TXT_TILE + 1) * (15 + LINE_EXTRA))


# ---- degenerate cases, state and argument checks

def test_no_counted_reads_gives_zero_bytes():
    a, u, st, pa, pu = cover([("c", 1000), ("d", 2)], recs([se(0, 10, 20, hit=-1)]))
    assert a == b"" and u == b"" and st["points"] == [0, 0] and pa == [0] and st["records"] == 0
    g = eng.Gcov([], dict(P0))
    assert finish(g, [])[:2] == (b"", b"")


def test_state_checks():
    ch = [("c", 1000), ("d", 300)]
    rd = recs([se(0, 10, 20), se(1, 5, 9)])
    g = eng.Gcov([1000, 300], dict(P0))
    with pytest.raises(eng.ItxError, match="rc=-5"):                        # no tid map yet
        feed_run(g, rd)
    with pytest.raises(eng.ItxError, match="rc=-5"):                        # next before finish
        g.next(0)
    g.set_tidmap([0, 1])
    feed_run(g, rd)
    for order in ([0, 0], [0, 2], [7]):                                     # twice; no such chromosome
        with pytest.raises(eng.ItxError, match="rc=-1"):
            g.finish(order, ["c", "d"])
    g.finish([0, 1], ["c", "d"], 1)                                         # (the refused calls left the arrays as they were)
    with pytest.raises(eng.ItxError, match="rc=-5"):                        # a second finish
        g.finish([0, 1], ["c", "d"])
    with pytest.raises(eng.ItxError, match="rc=-5"):
        feed_run(g, rd)
    with pytest.raises(eng.ItxError, match="rc=-5"):
        g.add_host([0], [1], [2], [1])
    with pytest.raises(eng.ItxError, match="rc=-5"):
        g.set_tidmap([0, 1])
    assert g.next(0) == (b"c\t10\t20\t1\n", True)
    with pytest.raises(eng.ItxError, match="rc=-5"):                        # file 0 has rounds left
        g.next(1)
    assert g.next(0) == (b"", True) and g.next(0) == (b"d\t5\t9\t1\n", True) and g.next(0) == (b"", False)
    with pytest.raises(eng.ItxError, match="rc=-5"):                        # file 0 has been handed out
        g.next(0)
    assert g.text(1)[0] == b"c\t10\t20\t1\nd\t5\t9\t1\n"
    with pytest.raises(eng.ItxError, match="rc=-1"):
        g.next(2)
    g.close()


def test_argument_checks():
    import ctypes as C
    L = eng.load()
    h = C.c_void_p()
    p = eng.Params(10, 1e-4, 0, 500, 0, 0, eng.MODE_FILTER, eng.ACCUM_DEFAULT)
    cs = np.array([100, 200], np.int64)
    big = np.array([100, 1 << 31], np.int64)
    assert L.itx_gcov_create(0, eng._p(cs), -1, C.byref(p), 16, C.byref(h)) == -1
    assert L.itx_gcov_create(0, eng._p(cs), 2, C.byref(p), 0, C.byref(h)) == -1
    assert L.itx_gcov_create(0, None, 2, C.byref(p), 16, C.byref(h)) == -1
    assert L.itx_gcov_create(0, eng._p(cs), 2, None, 16, C.byref(h)) == -1
    assert L.itx_gcov_create(0, eng._p(cs), 2, C.byref(p), 16, None) == -1
    assert L.itx_gcov_create(0, eng._p(big), 2, C.byref(p), 16, C.byref(h)) == -6 and not h.value
    assert L.itx_gcov_set_tidmap(None, None, 0) == -1 and L.itx_gcov_wait_kernels(None) == -1 and L.itx_gcov_get_stats(None, None) == -1
    assert L.itx_gcov_run(None, None, None, 0, None) == -1 and L.itx_gcov_add_host(None, None, None, None, None, 0) == -1
    assert L.itx_gcov_finish(None, None, 0, None, None, 0) == -1 and L.itx_gcov_next(None, 0, None) == -1
    assert L.itx_gcov_hits(None) is None and L.itx_gcov_stream(None) is None
    g = eng.Gcov(cs, dict(P0))
    assert L.itx_gcov_run(g._h, None, None, 0, None) == -1 and L.itx_gcov_add_host(g._h, None, None, None, None, 3) == -1
    assert L.itx_gcov_set_tidmap(g._h, None, 2) == -1 and L.itx_gcov_finish(g._h, None, 2, None, None, 0) == -1
    assert L.itx_gcov_hits(g._h) and L.itx_gcov_stream(g._h)
    g.close()
