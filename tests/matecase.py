"""The mates of `filter -b -s -m`, restated in Python for the tests (the product's statement is iteres_amd/csrc/itx_materule.h; this file
shares no code with it). Records are bytes from their block_size field on and are parsed with struct alone.

    wanted(r)      PAIRED (0x1) set and MUNMAP (0x8) clear, the fixed part there
    candidate(c)   PAIRED set, READ1 (0x40) clear; UNMAP (0x4), MUNMAP (0x8), 0x100, 0x800 clear; tid >= 0, pos >= 0; whole
    match(r, c)    c.tid == r.mtid, c.pos == r.mpos, equal names
    key            (tid, pos, h32(name)) of a candidate, (mtid, mpos, h32(name)) of a wanted record; h32: 32-bit FNV-1a, no NUL
    chosen         per wanted record the first matching candidate in stream order; a candidate chosen twice is written once, under -a
                   with the tags of the earliest counted record that chose it
    expected       stable sorted(counted + chosen mates in input order, key=(tid, pos, reverse))
"""
import struct

import reptagcase as rt

PAIRED, UNMAP, MUNMAP, READ1, SECONDARY, SUPPLEMENTARY = 0x1, 0x4, 0x8, 0x40, 0x100, 0x800
FIXED = 36


def avail(rec, n=None):
    """the bytes of the record that may be looked at when n of them are there: min(n, 4 + block_size)"""
    n = len(rec) if n is None else n
    if n < 4:
        return 0
    return min(n, 4 + struct.unpack_from("<I", rec, 0)[0])


def fields(rec):
    bs, tid, pos, l_name, mapq, bn, n_cigar, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<IiiBBHHHiiii", rec, 0)
    return dict(tid=tid, pos=pos, l_name=l_name, flag=flag, mtid=mtid, mpos=mpos, tlen=tlen)


def fixed(rec, n=None):
    return avail(rec, n) >= FIXED


def whole(rec, n=None):
    return fixed(rec, n) and rec[12] >= 1 and FIXED + rec[12] <= avail(rec, n)


def wanted(rec, n=None):
    if not fixed(rec, n):
        return False
    f = fields(rec)["flag"]
    return bool(f & PAIRED) and not f & MUNMAP


def candidate(rec, n=None):
    if not whole(rec, n):
        return False
    f = fields(rec)
    if not f["flag"] & PAIRED or f["flag"] & READ1:
        return False
    if f["flag"] & (UNMAP | MUNMAP | SECONDARY | SUPPLEMENTARY):
        return False
    return f["tid"] >= 0 and f["pos"] >= 0


def name(rec):
    return bytes(rec[FIXED:FIXED + rec[12] - 1])


def h32(nm):
    h = 2166136261
    for b in nm:
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


def key_candidate(rec):
    f = fields(rec)
    return f["tid"] & 0xffffffff, f["pos"] & 0xffffffff, h32(name(rec))


def key_wanted(rec):
    f = fields(rec)
    return f["mtid"] & 0xffffffff, f["mpos"] & 0xffffffff, h32(name(rec))


def match(r, c, rn=None, cn=None):
    if not whole(r, rn) or not whole(c, cn):
        return False
    fr, fc = fields(r), fields(c)
    return fc["tid"] == fr["mtid"] and fc["pos"] == fr["mpos"] and r[12] == c[12] and name(r) == name(c)


def sort_key(rec):
    f = fields(rec)
    return f["tid"], f["pos"], (f["flag"] >> 4) & 1


def collide(prefix=b"c"):
    """two different names of equal length with equal h32, by a birthday search over `prefix` + a decimal counter padded to 7 digits"""
    seen = {}
    k = 0
    while True:
        nm = prefix + b"%07d" % k
        h = h32(nm)
        if h in seen:
            return seen[h], nm
        seen[h] = nm
        k += 1


def choose(counted, seen):
    """counted: the counted records in stream order; seen: every record that passed (device windows and host-route windows) in stream
    order. -> ([(candidate record, index of the earliest counted record that chose it)] in stream order, wanted, found)"""
    cands = [c for c in seen if candidate(c)]
    by_key = {}
    for j, c in enumerate(cands):
        by_key.setdefault((fields(c)["tid"], fields(c)["pos"], name(c)), []).append(j)
    sel = {}
    n_wanted = n_found = 0
    for i, r in enumerate(counted):
        if not wanted(r):
            continue
        n_wanted += 1
        if not whole(r):
            continue
        f = fields(r)
        for j in by_key.get((f["mtid"], f["mpos"], name(r)), []):
            assert match(r, cands[j])
            n_found += 1
            sel[j] = min(sel.get(j, i), i)
            break
    return [(cands[j], sel[j]) for j in sorted(sel)], n_wanted, n_found


def expected(counted, seen, rows=None, tab=None):
    """the sorted output stream's records. rows / tab (rows, reps, clas, fams): under -a counted[i] was counted for rows[i]; the counted
    records and the mates leave with their row's tags"""
    mates, n_wanted, n_found = choose(counted, seen)

    def tagged(rec, row):
        if tab is None:
            return rec
        t, reps, clas, fams = tab
        w = t[int(row)]
        return rt.annotate(rec, reps[int(w["rep"])], clas[int(w["cla"])], fams[int(w["fam"])], int(w["start"]), int(w["end"]))
    pool = [tagged(r, rows[i] if rows is not None else None) for i, r in enumerate(counted)]
    pool += [tagged(c, rows[i] if rows is not None else None) for c, i in mates]
    return sorted(pool, key=sort_key), n_wanted, n_found
