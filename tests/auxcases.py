"""BAM records, as raw bytes, whose optional fields probe the walk of bam_aux_get and the XA / NM veto: deliberate cases and seeded
random tag sequences, sorted by what the reference (tests/auxmodel.py) makes of them into

    ref_safe      the reference is defined on the record and survives it: the model is never UNDEF, a found XA is a string, every
                  non-empty alternative has its four fields and no number the device leaves to the host
    all_defined   ref_safe, plus XA tags that are no strings and the alternatives that go to the host
    undefined     the records on which the reference leaves the record: the project's own rule answers

Record k of a list lies on chr1 at 1000 k + 200 inside a repeat row [1000 k, 1000 k + 500) whose repName R<k> no other row of
chr1 carries, so the row a read chooses is known and its name's count tells whether the read was kept. chr2 has a row r<k> (the
same word in another case) at the same coordinates and one row TAIL that ends with the chromosome; chrEmpty has no rows."""
import struct

import numpy as np

import auxmodel as am
from bedcase import record, tag

SLOT, ROW_LEN, READ_AT = 1000, 500, 200
I8, U8, I16, U16, I32, U32 = (struct.Struct("<" + c).pack for c in "bBhHiI")


def chroms(n):
    return [("chr1", SLOT * (n + 2)), ("chr2", SLOT * (n + 2)), ("chrEmpty", 50_000)]


def table(n):
    """rows (chrom index, start, end, name) in file order, and the same as the model's Table"""
    size2 = SLOT * (n + 2)
    rows = [(0, SLOT * k, SLOT * k + ROW_LEN, b"R%d" % k) for k in range(n + 1)]
    rows += [(1, SLOT * k, SLOT * k + ROW_LEN, b"r%d" % k) for k in range(n + 1)]
    rows.append((1, size2 - 100, size2, b"TAIL"))
    names = [c.encode() for c, _ in chroms(n)]
    by = {}
    for c, s, e, nm in rows:
        by.setdefault(names[c], []).append((s, e, nm))
    return rows, am.Table({nm.encode(): sz for nm, sz in chroms(n)}, by)


# ---- alternatives of record k, by where they point

def alt(k, n, kind, nm2=b"0", sign=b"+", cigar=b"36M"):
    size2 = SLOT * (n + 2)
    c, p = {"other": (b"chr1", SLOT * (k + 1) + 220), "own": (b"chr1", SLOT * k + 210), "twin": (b"chr2", SLOT * k + 230),
            "twin-other": (b"chr2", SLOT * (k + 1) + 240), "norow": (b"chr1", SLOT * k + 700), "unknown": (b"chrU", 300),
            "prefix": (b"chr", SLOT * (k + 1) + 220), "upper": (b"CHR1", SLOT * (k + 1) + 220), "noname": (b"", SLOT * (k + 1) + 220),
            "empty-chrom": (b"chrEmpty", 100), "past-end": (b"chr2", size2 + 40), "at-end": (b"chr2", size2), "into-end": (b"chr2", size2 - 10),
            "zero": (b"chr1", 0)}[kind]
    return b"%s,%s%d,%s,%s" % (c, sign, p, cigar, nm2)


KINDS = ["other", "own", "twin", "twin-other", "norow", "unknown", "prefix", "upper", "noname", "empty-chrom", "past-end", "at-end", "into-end", "zero"]


def xa_z(s, ty="Z"):
    return tag("XA", ty, s + b"\0")


def nm_tag(v=1, ty="C"):
    return tag("NM", ty, {"c": I8, "C": U8, "s": I16, "S": U16, "i": I32, "I": U32}[ty](v))


# ---- fillers: one tag of every type (B of every subtype with 0, 1 and 3 elements), values that are themselves tag-like

def fillers():
    F = [("A", tag("XT", "A", b"U")), ("c", tag("X1", "c", I8(-3))), ("C", tag("X0", "C", U8(7))), ("s", tag("XS", "s", I16(-300))),
         ("S", tag("XS", "S", U16(40000))), ("i", tag("AS", "i", I32(-70000))), ("I", tag("AS", "I", U32(3000000000))),
         ("f", tag("XF", "f", struct.pack("<f", 1.5))), ("f0", tag("XF", "f", bytes(4))), ("d", tag("XD", "d", struct.pack("<d", 2.25))),
         ("Z", tag("MD", "Z", b"10A25\0")), ("Z-empty", tag("MD", "Z", b"\0")), ("H", tag("XH", "H", b"1AE3\0")), ("unknown", tag("Xq", "?", b"")),
         ("unknown-v", tag("Xq", "!", b"ab"))]
    for sub, w in (("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4), ("A", 1), ("d", 8), ("q", 3)):
        for cnt in (0, 1, 3):
            F.append(("B%s%d" % (sub, cnt), tag("ZB", "B", sub.encode() + I32(cnt) + bytes(range(1, 1 + w * cnt)))))
    # floats whose bytes spell tags: the reference walks INTO the value
    for label, v in (("f=XA", b"XAZ\0"), ("f=NM", b"NMC\5"), ("f=Z", b"abZ\0"), ("f=B", b"abBC"), ("f=C", b"abCx"), ("d=XA", b"XAZq,+1\0")):
        F.append((label, tag("XF", label[0], v)))
    F.append(("Z-holds-tags", tag("MD", "Z", b"xXAZchr1,+5,3M,0;NMC\7yy\0")))
    return F


def deliberate(n_hint):
    """[(label, function k -> aux bytes, keyword arguments of record())]"""
    D = []
    add = lambda label, f, **kw: D.append((label, f, kw))
    veto_xa = lambda k: xa_z(alt(k, n_hint, "other", b"1") + b";")
    for name, f in fillers():
        add("front-of-NM:" + name, lambda k, f=f: f + nm_tag(2) + veto_xa(k))
        add("front-of-XA:" + name, lambda k, f=f: nm_tag(2) + f + veto_xa(k))
        add("XA-then:" + name + ":NM", lambda k, f=f: veto_xa(k) + f + nm_tag(2))
        add("last:" + name, lambda k, f=f: nm_tag(2) + veto_xa(k) + f)
        add("alone:" + name, lambda k, f=f: f)
    add("NM-after-XA", lambda k: veto_xa(k) + nm_tag(1))
    add("two-XA", lambda k: nm_tag(1) + xa_z(alt(k, n_hint, "own", b"0") + b";") + veto_xa(k))
    add("two-XA-rev", lambda k: nm_tag(1) + veto_xa(k) + xa_z(alt(k, n_hint, "own", b"0") + b";"))
    add("two-NM", lambda k: nm_tag(0) + nm_tag(5) + veto_xa(k))
    add("two-NM-rev", lambda k: nm_tag(5) + nm_tag(0) + veto_xa(k))
    for ty, vals in (("c", (-128, -1, 0, 127)), ("C", (0, 1, 255)), ("s", (-32768, -1, 32767)), ("S", (0, 65535)), ("i", (-2**31, -1, 0, 2**31 - 1)),
                     ("I", (0, 2**31 - 1, 2**31, 2**32 - 1))):
        for v in vals:
            add("NM:%s:%d" % (ty, v), lambda k, ty=ty, v=v: nm_tag(v, ty) + veto_xa(k))
    add("NM:A", lambda k: tag("NM", "A", b"7") + veto_xa(k))
    add("NM:f", lambda k: tag("NM", "f", struct.pack("<f", 2.5)) + veto_xa(k))
    add("NM:f-benign", lambda k: tag("NM", "f", b"abCx") + veto_xa(k))
    add("NM:Z", lambda k: tag("NM", "Z", b"12\0") + veto_xa(k))
    add("no-NM", veto_xa)
    add("XA:H", lambda k: nm_tag(1) + xa_z(alt(k, n_hint, "other", b"1") + b";", "H"))
    add("XA:i", lambda k: nm_tag(1) + tag("XA", "i", I32(7)))
    add("XA:A", lambda k: nm_tag(1) + tag("XA", "A", b"x"))
    add("XA:f", lambda k: nm_tag(1) + tag("XA", "f", bytes(4)) + nm_tag(3))
    add("no-aux", lambda k: b"")
    # the record's shape in front of the tags
    for label, kw in (("l_qseq-0", dict(l_qseq=0)), ("l_qseq-odd", dict(l_qseq=7)), ("l_qseq-even", dict(l_qseq=8)), ("no-cigar", dict(cigar=(), l_qseq=51)),
                      ("no-cigar-no-seq", dict(cigar=(), l_qseq=0)), ("3-cigar", dict(cigar=((0, 20), (1, 5), (0, 30)), l_qseq=55)), ("reverse", dict(flag=16)),
                      ("mapq-0", dict(mapq=0))):
        add("shape:" + label, lambda k: nm_tag(2) + veto_xa(k), **kw)
        add("shape:" + label + ":f", lambda k: tag("XF", "f", bytes(4)) + nm_tag(2) + veto_xa(k), **kw)
        add("shape:" + label + ":bare", lambda k: b"", **kw)
    # what an XA string may hold
    for kind in KINDS:
        for nm2 in (b"0", b"2", b"3"):
            add("alt:%s:%s" % (kind, nm2.decode()), lambda k, kind=kind, nm2=nm2: nm_tag(2) + xa_z(alt(k, n_hint, kind, nm2, b"-" if nm2 == b"2" else b"+") + b";"))
    A = lambda k, kind="other", nm2=b"1": alt(k, n_hint, kind, nm2)
    QUIET = b"chrU,+1,1M,0"                                       # (the reference copies the string into 2000 bytes: keep it short)
    strings = {
        "no-trailing-semicolon": lambda k: A(k, "own") + b";" + A(k),
        "empty-alternatives": lambda k: b";;" + A(k, "own") + b";;" + A(k) + b";",
        "empty-string": lambda k: b"",
        "only-semicolons": lambda k: b";;;",
        "more-than-100": lambda k: b";".join([QUIET] * 100 + [A(k)] * 5) + b";",
        "exactly-100-then-veto": lambda k: b";".join([QUIET] * 99 + [A(k)]) + b";",
        "empties-count-among-the-100": lambda k: b";" * 99 + A(k) + b";" + A(k, "twin-other"),
        "empties-fill-the-100": lambda k: b";" * 100 + A(k) + b";",
        "five-fields": lambda k: A(k) + b",extra;",
        "five-fields-number-cut": lambda k: A(k, "other", b"9") + b";" + alt(k, n_hint, "other", b"1,9") + b";",
        "first-keeps-second-vetoes": lambda k: A(k, "own", b"0") + b";" + A(k, "norow", b"0") + b";" + A(k, "other", b"2") + b";",
        "nm2-above": lambda k: A(k, "other", b"3") + b";",
        "minus-zero": lambda k: alt(k, n_hint, "zero", b"1", b"-") + b";" + A(k, "own"),
        "sign-alone": lambda k: b"chr1,+,36M,1;",
        "empty-field-3": lambda k: b"chr1,+%d,36M,;" % (SLOT * (k + 1) + 220),
        "empty-field-1": lambda k: b"chr1,,36M,1;",
        "nine-digits": lambda k: b"chr1,+999999999,36M,1;" + A(k),
        "nine-digits-nm2": lambda k: b"chr1,+%d,36M,100000000;" % (SLOT * (k + 1) + 220),
        "number-then-text": lambda k: b"chr1,+%dabc,36M,1x;" % (SLOT * (k + 1) + 220),
        "negative-nm2": lambda k: b"chr1,+%d,36M,-1;" % (SLOT * (k + 1) + 220),
    }
    for label, f in strings.items():
        add("xa:" + label, lambda k, f=f: nm_tag(2) + xa_z(f(k)))
    add("xa:negative-nm2:NM-1", lambda k: nm_tag(-1, "c") + xa_z(b"chr1,+%d,36M,-1;" % (SLOT * (k + 1) + 220)))
    add("xa:negative-nm2:NM-2", lambda k: nm_tag(-2, "c") + xa_z(b"chr1,+%d,36M,-1;" % (SLOT * (k + 1) + 220)))
    # for the host: numbers strtol reads differently from plain decimal, alternatives without their four fields
    hard = {
        "ten-digits": lambda k: b"chr1,+1234567890,36M,1;",
        "ten-digits-nm2": lambda k: b"chr1,+%d,36M,1234567890;" % (SLOT * (k + 1) + 220),
        "octal": lambda k: b"chr1,+0644,36M,1;",
        "hex": lambda k: b"chr1,-0x1f40,36M,0;",
        "blank": lambda k: b"chr1, 812,36M,0;",
        "octal-nm2": lambda k: A(k, "other", b"010") + b";",
        "three-fields": lambda k: b"chr1,+5,36M;",
        "one-field": lambda k: b"x;",
        "three-fields-behind-a-veto": lambda k: A(k) + b";chr1,+5,36M;",
        "octal-behind-nm2-above": lambda k: b"chr1,+0644,36M,7;",
    }
    for label, f in hard.items():
        add("host:" + label, lambda k, f=f: nm_tag(2) + xa_z(f(k)))
    # the record ends inside a tag
    cut = {
        "XA-no-NUL": lambda k: nm_tag(2) + tag("XA", "Z", b"chr1,+5,36M,0;"),
        "XA-name-last": lambda k: nm_tag(2) + b"XA",
        "XA-type-last": lambda k: nm_tag(2) + b"XAZ",
        "one-byte": lambda k: b"X",
        "name-only": lambda k: b"Xy",
        "NM-name-last": lambda k: veto_xa(k) + b"NM",
        "NM-type-last": lambda k: veto_xa(k) + b"NMi",
        "NM-value-cut": lambda k: veto_xa(k) + b"NMi\1\0",
        "Z-no-NUL-in-front": lambda k: tag("MD", "Z", b"10A") + b"",
        "B-header-cut": lambda k: nm_tag(2) + veto_xa(k) + b"ZBBc\1\0",
        "B-negative-count": lambda k: tag("ZB", "B", b"c" + I32(-4)) + nm_tag(2) + veto_xa(k),
        "B-overruns": lambda k: tag("ZB", "B", b"i" + I32(1000) + bytes(8)) + veto_xa(k),
        "B-huge-count": lambda k: tag("ZB", "B", b"i" + I32(0x40000001)) + veto_xa(k),
        "i-overruns": lambda k: veto_xa(k) + b"ASi\1\2",
        "float-last-misaligns": lambda k: veto_xa(k) + tag("XF", "f", b"\0\0\0\0") + b"N",
    }
    for label, f in cut.items():
        add("cut:" + label, f)
    return D


# ---- seeded random tag sequences

_NAMES = [b"X0", b"X1", b"XM", b"XO", b"XG", b"XT", b"MD", b"AS", b"RG", b"ZB"]


def _filler(rng):
    nm = _NAMES[int(rng.integers(0, len(_NAMES)))]
    r = rng.random()
    if r < 0.62:
        ty = "AcCsSiI"[int(rng.integers(0, 7))]
        w = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4}[ty]
        return nm + ty.encode() + (b"U" if ty == "A" else bytes(int(x) for x in rng.integers(0, 256, w)))
    if r < 0.80:
        body = bytes(int(x) for x in rng.choice(np.frombuffer(b"0123456789ACGT^,;XANMZ", np.uint8), int(rng.integers(0, 12))))
        return nm + (b"Z" if rng.random() < 0.8 else b"H") + body + b"\0"
    if r < 0.90:
        sub = "cCsSiIfAdq"[int(rng.integers(0, 10))]
        w = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "A": 1, "d": 8, "q": 2}[sub]
        cnt = int(rng.choice([0, 1, 3]))
        return nm + b"B" + sub.encode() + I32(cnt) + bytes(int(x) for x in rng.integers(0, 256, w * cnt))
    if r < 0.965:
        # a float: any bytes, a round value, or bytes that spell a tag
        k = rng.random()
        v = bytes(int(x) for x in rng.integers(0, 256, 4)) if k < 0.3 else struct.pack("<f", float(rng.choice([0.0, 1.0, 1.5, 48.25, -3.0]))) if k < 0.6 else \
            [b"XAZ\0", b"NMC\3", b"abZ\0", b"abCx", b"abAx", b"abBC"][int(rng.integers(0, 6))]
        return nm + b"f" + v
    if r < 0.985:
        return nm + b"d" + (struct.pack("<d", float(rng.choice([0.0, 2.25, 1e10]))) if rng.random() < 0.6 else b"abZ\0abCx")
    return nm + bytes([int(rng.choice(np.frombuffer(b"?!FDxq", np.uint8)))]) + bytes(int(x) for x in rng.integers(0, 256, int(rng.integers(0, 3))))


def random_aux(rng, k, n):
    items = [_filler(rng) for _ in range(int(rng.integers(0, 4)))]
    if rng.random() < 0.8:
        alts = [alt(k, n, KINDS[int(rng.integers(0, len(KINDS)))] if rng.random() < 0.5 else ["other", "own", "twin"][int(rng.integers(0, 3))],
                    b"%d" % int(rng.integers(0, 5)), b"+-"[int(rng.integers(0, 2)):][:1]) for _ in range(int(rng.integers(1, 4)))]
        items.insert(int(rng.integers(0, len(items) + 1)), xa_z(b";".join(alts) + (b";" if rng.random() < 0.8 else b"")))
    if rng.random() < 0.8:
        ty = "cCsSiI"[int(rng.integers(0, 6))]
        items.insert(int(rng.integers(0, len(items) + 1)), nm_tag(int(rng.integers(0, 5)), ty))
    return b"".join(items)


# ---- the lists

class Rec:
    def __init__(self, k, label, rec, kw):
        self.k, self.label, self.rec, self.kw = k, label, rec, kw
        self.aux = am.aux_region(rec)
        self.a = am.Answer(self.aux)
        self.qname = b"q%d" % k


def _make(k, label, aux, kw):
    q = dict(tid=0, pos=SLOT * k + READ_AT, mapq=37, flag=0, qname=b"q%d\0" % k, cigar=((0, 50),), l_qseq=0)
    q.update(kw)
    return Rec(k, label, record(aux=aux, **q), kw)


def _is_host_business(a):
    """an alternative among the first 100 without its four fields, or with a number the device leaves to the host"""
    for f in am.chop(a.p_xa, b";", 100):
        if f:
            r = am.chop(f, b",", 4)
            if len(r) != 4 or am.number_is_hard(r[1]) or am.number_is_hard(r[3]):
                return True
    return False


def classify(r):
    if r.a.undefined:
        return "undefined"
    if r.a.found is True and (r.a.xa is None or _is_host_business(r.a) or len(r.a.xa) >= 1990):
        return "all_defined"
    return "ref_safe"


_CACHE = {}


def cases(n_random=5800, seed=20240611):
    """every record, numbered in one sequence: (records, n)"""
    if (n_random, seed) not in _CACHE:
        D = deliberate(0)
        n = len(D) + n_random
        D = deliberate(n)
        rng = np.random.default_rng(seed)
        R = [_make(k, label, f(k), kw) for k, (label, f, kw) in enumerate(D)]
        for k in range(len(D), n):
            shape = {} if rng.random() < 0.7 else [dict(l_qseq=7), dict(cigar=(), l_qseq=51), dict(cigar=((0, 20), (1, 5), (0, 30)), l_qseq=55), dict(flag=16), dict(mapq=0)][int(rng.integers(0, 5))]
            R.append(_make(k, "random", random_aux(rng, k, n), shape))
        for r in R:
            r.set = classify(r)
        _CACHE[(n_random, seed)] = (R, n)
    return _CACHE[(n_random, seed)]


def subset(which):
    """the records of the named sets, in order (each keeps its number k, and with it its place and its row)"""
    return [r for r in cases()[0] if r.set in which]


def interval(r, size, extension=150):
    """(start, end) of a single-end mapped record (generic.c:889-903), None when it is unmapped"""
    tid, pos, x1, x2, l_qseq = struct.unpack_from("<iiIIi", r.rec, 4)
    flag, ncig = x2 >> 16, x2 & 0xffff
    if flag & 4:
        return None
    e = pos
    for j in range(ncig):
        c, = struct.unpack_from("<I", r.rec, 36 + (x1 & 0xff) + 4 * j)
        if c & 0xf in (0, 2, 3):
            e += c >> 4
    cend = size - 1
    start, end = pos, min(cend, e if ncig else pos + l_qseq)
    if extension:
        if flag & 16:
            start = 0 if end < extension else end - extension
        else:
            end = min(start + extension, cend)
    return start, end


def verdict(r, tab, n, extension=150, device=False):
    """(the record chooses its row, what the veto says: False / True / am.HARD / am.ASSERT)"""
    start, end = interval(r, SLOT * (n + 2), extension)
    chosen = min(end, SLOT * r.k + ROW_LEN) - max(start, SLOT * r.k) > 0
    if not chosen or not r.a.has_xa:
        return chosen, False
    return chosen, am.veto(tab, b"R%d" % r.k, r.a.p_nm, r.a.p_xa, end - start, device=device)


# ---- the files of a run of the command

def reads(recs, n):
    """the records as synth.Reads (write_bam lays the same optional fields behind a sequence of its own)"""
    from iteres_amd import synth
    f = lambda key, default: [r.kw.get(key, default) for r in recs]
    cig = [[("MIDNSHP=X"[op], ln) for op, ln in r.kw.get("cigar", ((0, 50),))] for r in recs]
    z = np.zeros(len(recs), np.int32)
    return synth.Reads(chroms(n), z.copy(), np.array([SLOT * r.k + READ_AT for r in recs], np.int32), np.array(f("flag", 0), np.uint16), np.array(f("mapq", 37), np.uint8),
                       np.array(f("l_qseq", 0), np.int32), z - 1, z - 1, z.copy(), cig, [r.qname.decode() for r in recs], [r.aux for r in recs])


def write_inputs(d, recs, n):
    """chrom.sizes, rep.sizes, rmsk.txt and reads.bam of the records in directory d"""
    from iteres_amd import synth
    rows, _ = table(n)
    names = [c for c, _ in chroms(n)]
    synth.write_sizes(str(d / "chrom.sizes"), chroms(n))
    synth.write_sizes(str(d / "rep.sizes"), [(nm.decode(), 600) for _, _, _, nm in rows])
    with open(d / "rmsk.txt", "w") as f:
        for i, (c, s, e, nm) in enumerate(rows):
            f.write(f"585\t1000\t10\t5\t5\t{names[c]}\t{s}\t{e}\t-1\t+\t{nm.decode()}\tCls{i % 3}\tFam{i % 7}\t1\t{e - s}\t-99\t{i % 9 + 1}\n")
    synth.write_bam(str(d / "reads.bam"), reads(recs, n), with_seq=True)
