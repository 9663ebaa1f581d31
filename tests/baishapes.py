"""The record shapes that the index tests drive through engine.Bamout, as inputs alone: tests/test_gpu_bamidx.py holds the device's
index of them against the restatement (tests/baicase.py), tests/test_gpu_bam_vs_reference.py against the reference's own indexer.
Every record carries the bin of its own interval, which the reference's indexer trusts.

A case is (l_ref, steps); steps: ("run", records, rows) for a device batch with the chosen row per record (-1: not counted), or
("host", records) for a host append."""
import baicase as bai
import bedcase as bc

P = bai.PAYLOAD
M, I, D, N, S = 0, 1, 2, 3, 4
_BASE = len(bc.record(qname=b"q\0", cigar=((M, 50),), aux=bc.tag("ZZ", "Z", b"\0")))


def rec(tid, pos, cigar=((M, 50),), L=None):
    """a record at (tid, pos); L: its exact length in bytes (block_size field included), made up by a Z tag"""
    extra = 4 * (len(cigar) - 1)
    if L is None:
        return bai.with_bin(bc.record(tid=tid, pos=pos, qname=b"q\0", cigar=cigar))
    pad = L - _BASE - extra
    assert pad >= 0, L
    r = bc.record(tid=tid, pos=pos, qname=b"q\0", cigar=cigar, aux=bc.tag("ZZ", "Z", bytes([65 + pos % 23]) * pad + b"\0"))
    assert len(r) == L
    return bai.with_bin(r)


def all_hit(recs):
    return [0] * len(recs)


def one_run(l_ref, recs):
    return l_ref, [("run", recs, all_hit(recs))]


def tile_boundaries(n, hit):
    """records on both sides of a 16 KiB window and of a 128 KiB bin boundary, so that chunks start inside a tile and at its edge"""
    recs = [rec(i * 3 // n, (1 << 17) - 64 * (n // 2) + 64 * i, L=60 + i % 90) for i in range(n)]
    rows = [0 if hit == "all" or i % 3 == 0 else -1 for i in range(n)]
    return [1 << 20, 1 << 20, 1 << 20], [("run", recs, rows)]


def last_byte_of_a_payload():
    return one_run([100_000], [rec(0, 10, L=P - 1), rec(0, 20, L=100), rec(0, 30, L=P - 100), rec(0, 40_000, L=77)])


def ends_on_a_payload_boundary(tail):
    return one_run([1000, 1000], [rec(0, 10, L=P // 2), rec(0, 20, L=P // 2), rec(1, 5, L=P)] + ([rec(1, 9, L=50)] if tail else []))


def three_payloads_and_17_bytes():
    return one_run([100_000], [rec(0, 5, L=300), rec(0, 6, L=3 * P + 17), rec(0, 7, L=300), rec(0, 20_000, L=300)])


def references_without_records():
    l_ref = [50_000, 70_000, 1 << 29, 0, 90_000, 20_000, 16_384]
    recs = [rec(1, 100), rec(1, 60_000, ((M, 10), (D, 9_000), (M, 10))), rec(2, (1 << 29) - 50), rec(4, 0), rec(4, 16_383, ((S, 5), (M, 1))), rec(4, 16_383, ((M, 2),)),
            rec(6, 16_334)]
    return l_ref, [("host", recs[:2]), ("run", recs[2:], all_hit(recs[2:]))]


def bin_parent_bin_again(L):
    """bin X, its parent, bin X again: inside one member the two runs of X merge into one chunk; when every record fills more
    than a member, the second run begins in a later member than the first ended in, and they stay two chunks"""
    return one_run([1 << 20], [rec(0, 100, L=L), rec(0, 110, L=L), rec(0, 200, ((M, 20_000),), L=L), rec(0, 300, L=L), rec(0, 310, L=L)])


def spliced_over_3000_windows():
    return one_run([60_000_000], [rec(0, 900), rec(0, 1000, ((M, 10), (N, 50_000_000), (M, 10))), rec(0, 2000), rec(0, 30_000_000), rec(0, 50_001_015)])


def big_case():
    """70 001 records for three `run` calls (every third is counted) and 404 for three host appends, all in coordinate order over
    references 0, 2 and 3; now and then a spliced or a long record, so that every bin level has chunks"""
    l_ref = [40_000_000, 1000, 30_000_000, 5_000_000]
    n = 70_001 + 404
    recs = []
    for k in range(n):
        tid, pos = (0, k * 500) if k < 30_000 else (2, (k - 30_000) * 500) if k < 60_000 else (3, (k - 60_000) * 400)
        cig = ((M, 30), (N, 20_000 << (k % 7)), (M, 20)) if k % 101 == 0 and tid != 3 else ((M, 20 + k % 80),) if k % 13 else ((S, 4), (M, 300), (I, 2), (M, 300))
        recs.append(rec(tid, pos, cig, L=60 + 4 * (len(cig) - 1) + (k * 7) % 90))
    cuts = [0, 3, 3 + 32768, 3 + 32768 + 400, 3 + 32768 + 400 + 32767, n - 1, n]
    kinds = ["host", "run", "host", "run", "run", "host"]
    steps = []
    for c, kind in enumerate(kinds):
        part = recs[cuts[c]:cuts[c + 1]]
        steps.append(("host", part) if kind == "host" else ("run", part, [2 if (cuts[c] + i) % 3 == 0 else -1 for i in range(len(part))]))
    assert sum(len(s[1]) for s in steps if s[0] == "run") == 70_001
    return l_ref, steps
