"""The restatements the BAM output is tested with, pinned against the code that defines the operations: the samtools 0.1.18 the
reference vendors, driven by oracle/_ref/bamcheck (oracle/bamcheck.c; tests/refbam.py runs it). No GPU; every file here is written
by tests/baicase.bam_file in the product's layout, with the bin of each record's own interval in it.
1. the index: bam_index_build's bytes equal baicase.expected_for_file's after refbam.normalise, which takes two places of the
   library's index to ours, each under its condition ("The index against the reference's own indexer"), and with the
   bins in ascending order (the library writes them in its hash table's order);
2. = and X operations: the library's bam_calend does not count them, the restatement does as the specification says;
3. fetch: bam_fetch through the restatement's .bai returns the records of baicase.linear_scan;
4. the sort: bam_sort_core is a stable sort on tid << 32 | pos + 1, without the strand that the project's rule has, and with
   pos + 1 computed in 32 bits."""
import struct

import numpy as np
import pytest

import baicase as bai
import baishapes as shapes
import bedcase as bc
import refbam
from baishapes import M, N, P, rec

pytestmark = pytest.mark.skipif(not refbam.present, reason="oracle/_ref/bamcheck is not built (make -C oracle ref needs the reference tree)")

I, D, S, EQ, X = 1, 2, 4, 7, 8


def header(l_ref):
    return [("ref%d" % t, ln) for t, ln in enumerate(l_ref)]


def counted(steps):
    return [r for s in steps for r, h in zip(s[1], s[2] if s[0] == "run" else [0] * len(s[1])) if h >= 0]


def draw(seed, n=3000):
    """n sorted records on two of three references: 50M, soft clips and indels, 40 kb splices; names of 2 to 9 bytes, so that the
    records begin at every alignment"""
    rng = np.random.default_rng(seed)
    l_ref = [1 << 22, 5000, 1 << 24]
    l_ref = [l_ref[(t + seed) % 3] for t in range(3)]                      # the reference without records: in front, between, behind
    recs = []
    for tid in [t for t in range(3) if l_ref[t] != 5000]:
        for k, pos in enumerate(sorted(int(x) for x in rng.integers(0, l_ref[tid] - 50_000, n // 2))):
            cig = (((M, 50),), ((S, 5), (M, 20), (I, 3), (M, 22)), ((M, 25), (D, 7), (M, 25)), ((M, 10), (N, 40_000), (M, 40)))[int(rng.integers(4)) if k % 5 == 0 else 0]
            recs.append(bc.record(tid=tid, pos=pos, flag=16 * (k & 1), qname=b"r%d" % (k * 7 ** (k % 8) % 10 ** (1 + k % 8)) + b"\0", cigar=cig, l_qseq=k % 3))
    return l_ref, recs


EDGE_FILES = {
    "window_and_bin_edges": lambda: shapes.tile_boundaries(257, "all"),
    "a_record_starts_on_the_last_byte_of_a_payload": shapes.last_byte_of_a_payload,
    "a_record_ends_on_a_payload_boundary": lambda: shapes.ends_on_a_payload_boundary(1),
    "the_last_record_ends_on_a_payload_boundary": lambda: shapes.ends_on_a_payload_boundary(0),
    "a_record_of_three_payloads": shapes.three_payloads_and_17_bytes,
    "chunks_merge": lambda: shapes.bin_parent_bin_again(80),
    "chunks_do_not_merge": lambda: shapes.bin_parent_bin_again(P + 900),
    "a_splice_then_short_records_that_end_before_it": lambda: shapes.one_run([60_000_000], [rec(0, 900), rec(0, 1000, ((M, 10), (N, 50_000_000), (M, 10))), rec(0, 2000),
                                                                                             rec(0, 30_000_000)]),
    "a_splice_then_a_record_behind_its_end": shapes.spliced_over_3000_windows,
    "references_without_records_in_front_and_between": shapes.references_without_records,
    "references_without_records_behind": lambda: shapes.one_run([1000, 50_000, 0, 70_000, 2000, 0], [rec(1, 100), rec(1, 40_000), rec(3, 0), rec(3, 69_950)]),
    "one_record": lambda: shapes.one_run([100_000], [rec(0, 20_000)]),
}


def write_case(tmp_path, l_ref, recs, name="case.bam"):
    data = bai.bam_file(header(l_ref), recs)
    path = tmp_path / name
    path.write_bytes(data)
    return path, data


def check_file(path, data):
    """the library's index of the file against the restatement's; returns (ours, the library's as it wrote it), both parsed"""
    status, ours = bai.expected_for_file(data)
    assert status == bai.OK
    lib = refbam.check_index(path, ours)
    ours = bai.parse_bai(ours)
    ends = [r["meta"][1] for r in lib if r["meta"] is not None]
    assert ends[-1] == len(data) << 16                                     # where the difference comes from: the end of the file
    assert [r["meta"][1] for r in ours if r["meta"] is not None][:-1] == ends[:-1]
    return ours, lib


# ---- 1. the index

@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_index_of_a_seeded_draw(seed, tmp_path):
    l_ref, recs = draw(seed)
    ours, lib = check_file(*write_case(tmp_path, l_ref, recs))
    assert sum(len(r["bins"]) for r in ours) > 300 and {sum(b >= f for f in (1, 9, 73, 585, 4681)) for r in ours for b in r["bins"]} >= {4, 5}


@pytest.mark.parametrize("name", list(EDGE_FILES))
def test_index_of_an_edge_file(name, tmp_path):
    l_ref, steps = EDGE_FILES[name]()
    path, data = write_case(tmp_path, l_ref, counted(steps))
    ours, lib = check_file(path, data)
    # the second rule is met where it must be: the library's linear index ends with the window of the reference's last record
    recs = bai.records_of(bai.split_bam(data)[1])
    last_window = {tid: (end - 1) >> 14 for tid, pos, end, at, ln in recs}
    assert [len(r["lin"]) for r in lib] == [last_window.get(tid, -1) + 1 for tid in range(len(l_ref))]
    shorter = any(len(a["lin"]) < len(b["lin"]) for a, b in zip(lib, ours))
    assert shorter == (name in ("a_splice_then_short_records_that_end_before_it", "chunks_merge", "chunks_do_not_merge"))


def test_normalise_takes_nothing_else():
    """the conditions are conditions: a chunk end below ours, an end that differs in an earlier reference, a linear index that is
    longer or differs inside the shared part are all refused"""
    ref = {"bins": {4681: [(100 << 16, 200 << 16)]}, "meta": (100 << 16, 200 << 16, 3, 0), "lin": [100 << 16]}
    two = {"bins": {4681: [(200 << 16, 300 << 16 | 7)]}, "meta": (200 << 16, 300 << 16 | 7, 2, 0), "lin": [200 << 16, 200 << 16]}
    ours = [ref, two]

    def lib(**kw):
        t, field, value = kw["t"], kw["field"], kw["value"]
        out = [dict(ref), dict(two)]
        out[t] = dict(out[t], **{field: value})
        return out
    far = {"bins": {4681: [(200 << 16, 400 << 16)]}, "meta": (200 << 16, 400 << 16, 2, 0)}
    assert refbam.bai_bytes(refbam.normalise([ref, dict(two, **far)], ours)) == refbam.bai_bytes(ours)
    assert refbam.bai_bytes(refbam.normalise(lib(t=1, field="lin", value=[200 << 16]), ours)) == refbam.bai_bytes(ours)
    near = {"bins": {4681: [(200 << 16, 300 << 16 | 6)]}, "meta": (200 << 16, 300 << 16 | 6, 2, 0)}
    with pytest.raises(AssertionError):
        refbam.normalise([ref, dict(two, **near)], ours)
    early = {"bins": {4681: [(100 << 16, 201 << 16)]}, "meta": (100 << 16, 201 << 16, 3, 0)}
    assert refbam.bai_bytes(refbam.normalise([dict(ref, **early), two], ours)) != refbam.bai_bytes(ours)
    with pytest.raises(AssertionError):
        refbam.normalise(lib(t=1, field="lin", value=[200 << 16] * 3), ours)
    assert refbam.bai_bytes(refbam.normalise(lib(t=1, field="lin", value=[201 << 16]), ours)) != refbam.bai_bytes(ours)


# ---- 2. = and X

def test_eq_and_x_operations_end_per_the_specification_on_our_side_only(tmp_path):
    """30= 30000X 20= at 20 000 covers the windows 1 .. 3; a 50M record follows in window 3. Ours: the linear index gives window 3
    the first record's offset, and a region inside the X stretch fetches it. The library's bam_calend adds nothing for = and X, so
    for it the record ends where it starts: its windows 2 and 3 come from the fill and from the second record, and its fetch of
    that region, through our index, returns nothing. The bins are equal: the library takes them from the records."""
    recs = [bc.record(tid=0, pos=20_000, qname=b"eqx\0", cigar=((EQ, 30), (X, 30_000), (EQ, 20))), bc.record(tid=0, pos=50_040, qname=b"m\0", cigar=((M, 50),))]
    path, data = write_case(tmp_path, [100_000], recs)
    status, ours = bai.expected_for_file(data)
    first = bai.split_bam(data)[3]
    v0, v1 = first << 16, first << 16 | len(recs[0])
    o, = bai.parse_bai(ours)
    assert status == bai.OK and o["lin"] == [0, v0, v0, v0] and sorted(o["bins"]) == [bai.reg2bin(20_000, 50_050), 4681 + 3] == [585, 4684]
    lib, = bai.parse_bai(refbam.library_index(path))
    assert lib["lin"] == [0, v0, v0, v1] and lib["bins"].keys() == o["bins"].keys() and lib["meta"][2:] == o["meta"][2:] == (2, 0)
    with pytest.raises(AssertionError):
        refbam.check_index(path, ours)
    l_ref, stream, sizes, first, raw, ustart = bai.split_bam(data)
    inside = (0, 40_000, 40_100)
    assert bai.fetch(bai.parse_bai(ours), raw, ustart, *inside) == bai.linear_scan(raw, len(raw) - len(stream), *inside) == {len(raw) - len(stream)}
    (path.parent / "case.bam.bai").write_bytes(ours)
    assert refbam.run("fetch", path, *inside).stdout == b""
    assert refbam.run("fetch", path, 0, 20_000, 20_001).stdout == b""       # (rend == pos: only a region that begins below pos finds it)
    assert refbam.run("fetch", path, 0, 19_999, 20_001).stdout.startswith(b"eqx\t0\tref0\t20001\t37\t30=30000X20=\t")


# ---- 3. fetch

FETCH_FILES = {
    "draw": (lambda: draw(2), [(0, 0, 1 << 24), (1, 0, 1 << 22), (2, 0, 5000), (2, 100, 200)]),
    "window_and_bin_edges": (lambda: shapes.tile_boundaries(257, "all"),
                             [(t, e - a, e + b) for t in (0, 1, 2) for e in (1 << 17, (1 << 17) - (1 << 14), (1 << 17) + (1 << 14)) for a, b in ((1, 0), (0, 1), (1, 1), (50, 0))]),
    "splice": (EDGE_FILES["a_splice_then_short_records_that_end_before_it"],
               [(0, 25_000_000, 25_000_100), (0, 50_001_009, 50_001_010), (0, 50_001_019, 50_001_020), (0, 50_001_020, 50_001_021), (0, 50_001_020, 60_000_000),
                (0, 2049, 2050), (0, 2050, 2051), (0, 899, 900), (0, 0, 900), (0, 1 << 14, (1 << 14) + 1), (0, (1 << 26) - 1, (1 << 26) + 1)]),
    "empty_references": (EDGE_FILES["references_without_records_behind"], [(0, 0, 1000), (2, 0, 1), (4, 0, 2000), (5, 0, 1), (1, 40_050, 50_000), (3, 70_000, 80_000)]),
}


@pytest.mark.parametrize("name", list(FETCH_FILES))
def test_fetch_through_the_restatements_index(name, tmp_path):
    """regions one base on either side of window and bin edges, whole references, references without records, a region behind the
    last record and one that only a splice reaches"""
    make, regions = FETCH_FILES[name]
    l_ref, recs = make()
    if recs and isinstance(recs[0], tuple):
        recs = counted(recs)
    path, data = write_case(tmp_path, l_ref, recs)
    status, ours = bai.expected_for_file(data)
    regions = regions + refbam.edge_regions(path)
    hits = refbam.check_fetch(path, ours, regions)
    assert 8 <= hits <= len(regions) - 8, (hits, len(regions))             # regions with records and regions without


# ---- 4. the sort

def lib_key(r):
    """bam_sort.c's bam1_lt: (uint64_t)tid << 32 | (pos + 1), tid and pos + 1 being int32_t. tid -1 makes the upper half all
    ones: unmapped records go last. pos + 1 is a 32-bit sum that the | widens with its sign: it is pos + 1 for every position
    the specification has (up to 2^31 - 2); at pos 2^31 - 1 it wraps to -2^31 and sets every upper bit, whatever the tid is"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    low = (pos + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31
    return ((tid % 2 ** 32) << 32 | low % 2 ** 64) % 2 ** 64


def issue_key(r):
    """(tid as unsigned, pos + 1): what lib_key comes to wherever pos + 1 fits 32 bits"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    return tid % 2 ** 32, pos + 1


def project_key(r):
    """itx_bamsortrule.h: tid, pos, reverse"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    return tid, pos, struct.unpack_from("<H", r, 18)[0] >> 4 & 1


def sort_input(seed, n=3000, unmapped=True, top=2 ** 31 - 1):
    """n records in a seeded order over three references: 40 positions per reference, so that every (tid, pos) has many records
    of both strands; pos 0 and `top` on every reference; unmapped records (tid -1, pos -1) in between. Names are unique"""
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(n):
        tid = int(rng.integers(3))
        pos = (0, top)[k % 2] if k % 50 < 2 else int(rng.integers(40)) * 1000
        if unmapped and k % 17 == 0:
            recs.append(bc.record(tid=-1, pos=-1, flag=4, qname=b"u%d\0" % k, cigar=()))
        else:
            recs.append(bc.record(tid=tid, pos=pos, flag=16 * int(rng.integers(2)), qname=b"s%d\0" % k))
    return recs


L_REF_SORT = [2 ** 31 - 1] * 3


def lib_sorted(tmp_path, recs):
    path = tmp_path / "in.bam"
    path.write_bytes(bai.bam_file(header(L_REF_SORT), recs, sorted_=False))
    head, out = refbam.library_sort(path, tmp_path / "out")
    assert sorted(out) == sorted(bai.with_bin(r) for r in recs)
    return out


@pytest.mark.parametrize("seed", [11, 12])
def test_sort_is_stable_by_tid_and_pos_plus_one(seed, tmp_path):
    """(a). The library's order is a stable sort by lib_key; that is the stable sort by (tid as unsigned, pos + 1) for all records
    below pos 2^31 - 1, and the records at 2^31 - 1 follow everything else in input order, the unmapped ones included"""
    recs = [bai.with_bin(r) for r in sort_input(seed)]
    out = lib_sorted(tmp_path, recs)
    assert out == sorted(recs, key=lib_key)
    top = [r for r in recs if issue_key(r)[1] == 2 ** 31]
    assert len(top) >= 30 and len({issue_key(r)[0] for r in top}) == 3
    assert out == sorted([r for r in recs if r not in top], key=issue_key) + top
    keys = [issue_key(r) for r in out]
    assert sum(a == b for a, b in zip(keys, keys[1:])) > 2000               # equal keys: the stability is tested


@pytest.mark.parametrize("top", [2 ** 31 - 2, 2 ** 31 - 1])
def test_a_file_in_the_projects_order_comes_back_unchanged(top, tmp_path):
    """(b). Up to pos 2^31 - 2, the last position the specification has (POS is 1-based and at most 2^31 - 1), the project's order
    is one of the orders the library's rule allows, and its stable sort leaves it alone. At pos 2^31 - 1 the library's 32-bit
    pos + 1 wraps (above): it moves those records of every reference to the end of the file, where the project keeps them as the
    last of their reference."""
    recs = sorted((bai.with_bin(r) for r in sort_input(21, unmapped=False, top=top)), key=project_key)
    out = lib_sorted(tmp_path, recs)
    if top == 2 ** 31 - 2:
        assert out == recs
    else:
        last = [r for r in recs if project_key(r)[1] == top]
        assert out == [r for r in recs if r not in last] + last and out != recs


@pytest.mark.parametrize("seed", [31, 32])
def test_the_two_orders_agree_up_to_the_strand(seed, tmp_path):
    """(c). The project's order and the library's have the same (tid, pos) sequence and the same records inside every run of equal
    (tid, pos); inside a run the project puts the forward strand first and the library keeps the input order. Records at pos
    2^31 - 1 are left to the test above."""
    recs = [bai.with_bin(r) for r in sort_input(seed, unmapped=False, top=2 ** 31 - 2)]
    ours = sorted(recs, key=project_key)
    out = lib_sorted(tmp_path, recs)
    assert_same_up_to_the_strand(ours, out)
    assert ours != out


def assert_same_up_to_the_strand(ours, lib):
    assert [project_key(r)[:2] for r in ours] == [project_key(r)[:2] for r in lib]
    runs, at = 0, 0
    while at < len(ours):
        end = at
        while end < len(ours) and project_key(ours[end])[:2] == project_key(ours[at])[:2]:
            end += 1
        assert sorted(ours[at:end]) == sorted(lib[at:end])
        runs += end - at > 1
        at = end
    return runs
