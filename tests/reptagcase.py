"""The tags of `filter -b -a` restated in Python from the rule's text (no code shared with iteres_amd/csrc/itx_reptag.h): the annotated
record is the input record with
    ZN:Z:repName  ZC:Z:repClass  ZF:Z:repFamily  ZS:I:genoStart  ZE:I:genoEnd
behind its bytes, both integers as uint32 whatever their value, and block_size increased by the tags' length (26 + the three names).
Also the way back: the aux fields of a record walked by the SAM specification's types, the last five taken off."""
import struct

KEYS = (b"ZN", b"ZC", b"ZF", b"ZS", b"ZE")


def tags(rep, cla, fam, start, end):
    out = b""
    for key, name in zip(KEYS[:3], (rep, cla, fam)):
        assert b"\0" not in name
        out += key + b"Z" + name + b"\0"
    for key, v in zip(KEYS[3:], (start, end)):
        out += key + b"I" + struct.pack("<I", v)
    assert len(out) == 26 + len(rep) + len(cla) + len(fam)
    return out


def annotate(rec, rep, cla, fam, start, end):
    """rec: one record from its block_size field on"""
    bs, = struct.unpack_from("<I", rec, 0)
    assert len(rec) == 4 + bs
    t = tags(rep, cla, fam, start, end)
    return struct.pack("<I", bs + len(t)) + rec[4:] + t


def annotate_rows(recs, hit_row, rows, reps, clas, fams):
    """the counted records (hit_row >= 0) of recs, each with the tags of its row; rows: a structured array with start, end, rep, cla, fam"""
    out = []
    for r, h in zip(recs, hit_row):
        if h >= 0:
            w = rows[int(h)]
            out.append(annotate(r, reps[int(w["rep"])], clas[int(w["cla"])], fams[int(w["fam"])], int(w["start"]), int(w["end"])))
    return out


_FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def aux_fields(rec):
    """[(offset, key, type, value bytes)] of the record's aux fields, by the specification's types"""
    bs, = struct.unpack_from("<I", rec, 0)
    assert len(rec) == 4 + bs
    l_name = rec[12]
    n_cigar, = struct.unpack_from("<H", rec, 16)
    l_seq, = struct.unpack_from("<i", rec, 20)
    at = 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    out = []
    while at < len(rec):
        key, ty = rec[at:at + 2], rec[at + 2:at + 3]
        v = at + 3
        if ty in _FIXED:
            end = v + _FIXED[ty]
        elif ty in (b"Z", b"H"):
            end = rec.index(b"\0", v) + 1
        elif ty == b"B":
            n, = struct.unpack_from("<I", rec, v + 1)
            end = v + 5 + n * _FIXED[rec[v:v + 1]]
        else:
            raise AssertionError("aux type %r at byte %d" % (ty, at))
        assert end <= len(rec)
        out.append((at, key, ty, rec[v:end]))
        at = end
    assert at == len(rec)
    return out


def strip(rec):
    """(the record without its last five aux fields and block_size restored, (repName, repClass, repFamily, genoStart, genoEnd));
    the five must be ZN:Z, ZC:Z, ZF:Z, ZS:I, ZE:I in this order"""
    f = aux_fields(rec)
    assert len(f) >= 5 and tuple(k for _, k, _, _ in f[-5:]) == KEYS and [t for _, _, t, _ in f[-5:]] == [b"Z", b"Z", b"Z", b"I", b"I"], f[-5:]
    cut = f[-5][0]
    vals = tuple(v[:-1] for _, _, _, v in f[-5:-2]) + tuple(struct.unpack("<I", v)[0] for _, _, _, v in f[-2:])
    return struct.pack("<I", cut - 4) + rec[4:cut], vals
