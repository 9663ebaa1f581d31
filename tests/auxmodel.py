"""The reference's reading of a BAM record's optional fields, written down literally — what the suite holds the shared walk
(iteres_amd/csrc/itx_auxwalk.h) and its four users to:

    aux_get      bam_aux_get with __skip_tag and bam_aux_type2size (cussamtools/bam_aux.c:28-48, bam.h:754-760)
    aux2i, aux2Z bam_aux.c:159-170, 199-206
    chop         chopByChar (cuskent/common.c:2029-2053)
    strtol0      strtol(s, 0, 0) followed by the cast to int
    veto         mapped2diffSubfam behind its gate (generic.c:303-341, 972-982) over a Table that answers as binKeeperFind does
    bed_tail     the trailing columns of a `stat -B` line (generic.c:925-931)

The reference's walk is not the SAM specification's: behind a tag of type f, d or of an unknown type it advances by 0 bytes and
reads the value's bytes as the next tags; array elements are sized by the raw subtype byte. Where it would read a byte at or
past the record's end the result is UNDEF here (its answer there depends on stale bytes of its buffer). `Answer` gives both
readings of a record: the reference's, with UNDEF in it, and the project's, which is the reference's wherever that is defined
and else follows the rule DESIGN.md states: the walk stops and the tag counts as not found, a value or string that would run
past the end reads as 0 or empty."""
import struct


class _Undef:
    def __repr__(self):
        return "UNDEF"


UNDEF = _Undef()


def type2size(x):
    """bam_aux_type2size, bam.h:754-760"""
    if x in (ord("C"), ord("c"), ord("A")):
        return 1
    if x in (ord("S"), ord("s")):
        return 2
    if x in (ord("I"), ord("i"), ord("f")):
        return 4
    return 0


def _toupper(c):
    return c - 32 if ord("a") <= c <= ord("z") else c


def aux_get(aux, tag):
    """bam_aux_get over the bytes [bam1_aux, data + data_len): the type byte's position (which may be len(aux): the reference
    returns it unread), None when the loop ends without a match, UNDEF when a byte at or past the end would be read"""
    n = len(aux)
    y = tag[0] << 8 | tag[1]
    s = 0
    while s < n:
        if s + 1 >= n:
            return UNDEF                                  # s[1]
        x = aux[s] << 8 | aux[s + 1]
        s += 2
        if x == y:
            return s
        # __skip_tag
        if s >= n:
            return UNDEF                                  # the type byte
        ty = _toupper(aux[s])
        s += 1
        if ty in (ord("Z"), ord("H")):
            z = aux.find(b"\0", s)
            if z < 0:
                return UNDEF                              # no NUL inside the record
            s = z + 1
        elif ty == ord("B"):
            if s + 5 > n:
                return UNDEF                              # the array's header
            cnt, = struct.unpack_from("<i", aux, s + 1)
            step = type2size(aux[s]) * cnt                # the raw subtype byte, a signed count, int arithmetic
            if cnt < 0 or step > 0x7fffffff - 5:
                return UNDEF                              # steps backwards / overflows int
            s += 5 + step
        else:
            s += type2size(ty)
    return None


def aux2i(aux, s):
    """bam_aux2i of what aux_get returned"""
    if s is None:
        return 0
    if s >= len(aux):
        return UNDEF
    ty = chr(aux[s])
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<i"}.get(ty)
    if fmt is None:
        return 0
    if s + 1 + struct.calcsize(fmt) > len(aux):
        return UNDEF
    return struct.unpack_from(fmt, aux, s + 1)[0]


def aux2Z(aux, s):
    """bam_aux2Z of a found tag: the string (as the reference's strcpy / %s reads it), None for a type that has none"""
    if s >= len(aux):
        return UNDEF
    if aux[s] not in (ord("Z"), ord("H")):
        return None
    z = aux.find(b"\0", s + 1)
    return UNDEF if z < 0 else aux[s + 1:z]


def aux_region(rec):
    """[bam1_aux, data + data_len) of a record given with its block_len"""
    bl, = struct.unpack_from("<i", rec, 0)
    x1, x2, l_qseq = struct.unpack_from("<IIi", rec, 12)
    data = rec[36:4 + bl]
    off = (x1 & 0xff) + 4 * (x2 & 0xffff) + (max(l_qseq, 0) + 1) // 2 + max(l_qseq, 0)
    return data[off:] if off < len(data) else b""


class Answer:
    """found / nm / xa: what the reference makes of the record where it prints or judges it (nm and xa only when found is True);
    any of them may be UNDEF, xa is None for an XA tag that is no string. has_xa / p_nm / p_xa: the project's reading."""

    def __init__(self, aux):
        s = aux_get(aux, b"XA")
        self.found = UNDEF if s is UNDEF else s is not None
        self.nm = self.xa = None
        self.has_xa, self.p_nm, self.p_xa = self.found is True, 0, b""
        if self.found is True:
            t = aux_get(aux, b"NM")
            self.nm = UNDEF if t is UNDEF else aux2i(aux, t)
            self.xa = aux2Z(aux, s)
            self.p_nm = 0 if self.nm is UNDEF else self.nm
            self.p_xa = b"" if self.xa is UNDEF or self.xa is None else self.xa

    @property
    def undefined(self):
        return self.found is UNDEF or self.nm is UNDEF or self.xa is UNDEF

    def old_walk_differs(self, aux):
        """does the walk this project shipped before (the SAM specification's sizes) read the record differently?"""
        return _old_answer(aux) != (self.has_xa, self.p_nm, self.p_xa)


def answer(rec):
    return Answer(aux_region(rec))


def bed_tail(a):
    """what `stat -B` prints behind the strand (generic.c:927-929), by the project's reading"""
    return b"\t%i\t%s" % (a.p_nm, a.p_xa) if a.has_xa else b""


# ---- the veto

def chop(s, sep, size):
    """chopByChar(in, chopper, outArray, outSize): the fields; the last one of `size` ends at the next separator"""
    if not s:
        return []
    out, at = [], 0
    while len(out) < size:
        k = s.find(sep, at)
        if k < 0:
            out.append(s[at:])
            return out
        out.append(s[at:k])
        at = k + 1
    return out


def strtol0(b):
    """(int)strtol(b, 0, 0) with a 64-bit long"""
    i, n = 0, len(b)
    while i < n and b[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < n and b[i] in b"+-":
        neg = b[i] == ord("-")
        i += 1
    base = 10
    if i < n and b[i] == ord("0"):
        if i + 2 < n and b[i + 1] in b"xX" and chr(b[i + 2]) in "0123456789abcdefABCDEF":
            base, i = 16, i + 2
        else:
            base = 8
    v = 0
    while i < n:
        d = int(chr(b[i]), 36) if chr(b[i]).isalnum() and b[i] < 128 else 99
        if d >= base:
            break
        v = v * base + d
        i += 1
    v = -v if neg else v
    v = max(-2**63, min(2**63 - 1, v))
    return ((v + 2**31) % 2**32) - 2**31


def number_is_hard(b):
    """the device's rule for a number it leaves to the host (csrc/itx_xaveto.hip xa_number): a leading blank, a leading 0 with a digit
    or x behind it, more than nine digits"""
    i = 0
    if b[:1] and b[0] in b" \t\n\v\f\r":
        return True
    if b[i:i + 1] in (b"+", b"-"):
        i += 1
    if b[i:i + 1] == b"0" and b[i + 1:i + 2] and (chr(b[i + 1]).isdigit() or b[i + 1] in b"xX"):
        return True
    nd = 0
    while i + nd < len(b) and chr(b[i + nd]).isdigit() and b[i + nd] < 128:
        nd += 1
    return nd > 9


class Table:
    """The repeat rows as the veto asks for them: rows[chrom name] = [(start, end, repName)], size[chrom name]"""

    def __init__(self, size, rows):
        self.size, self.rows = size, rows

    def any_other(self, chrom, start, end, name):
        """binKeeperFind(bs2, start, end) (binRange.c:196-227: clipped to [0, size)), then any hit whose name is not sameWord"""
        if chrom not in self.rows:                                  # hashLookup(hashRmsk, row2[0]): only chromosomes that have rows
            return False
        start, end = max(start, 0), min(end, self.size[chrom])
        if start >= end:
            return False
        return any(min(e, end) - max(s, start) > 0 and nm.upper() != name.upper() for s, e, nm in self.rows[chrom])


ASSERT, HARD = "assert", "hard"


def veto(table, name, nm, xa, qlen, device=False):
    """mapped2diffSubfam(hashRmsk, ss->name, nm, ahstring, qlen): True / False, or ASSERT where the reference's assert(num2 == 4)
    fails. device=True: the same parse as the device runs it, which answers HARD where it would have to leave the record to the
    host: fewer than four fields, a number strtol may read differently from plain decimal — in the order the parse meets them."""
    for f in chop(xa, b";", 100):
        if not f:
            continue
        r = chop(f, b",", 4)
        if len(r) != 4:
            return HARD if device else ASSERT
        if device and number_is_hard(r[3]):
            return HARD
        if strtol0(r[3]) <= nm:
            if device and number_is_hard(r[1]):
                return HARD
            start = abs(strtol0(r[1]))
            if start == -2**31:
                start = -2**31                                      # abs(INT_MIN) stays INT_MIN
            end = ((start + qlen + 2**31) % 2**32) - 2**31
            if table.any_other(r[0], start, end, name):
                return True
    return False


# ---- the walk the project shipped before this module existed, to count the records that tell the two apart

def _old_answer(aux):
    xa = nmv = None
    s, n = 0, len(aux)
    while s + 3 <= n and (xa is None or nmv is None):
        if xa is None and aux[s:s + 2] == b"XA":
            xa = s + 2
        if nmv is None and aux[s:s + 2] == b"NM":
            nmv = s + 2
        ty = chr(_toupper(aux[s + 2]))
        s += 3
        if ty in "AC":
            s += 1
        elif ty == "S":
            s += 2
        elif ty in "IF":
            s += 4
        elif ty == "D":
            s += 8
        elif ty in "ZH":
            z = aux.find(b"\0", s)
            s = n + 1 if z < 0 else z + 1
        elif ty == "B":
            if s + 5 > n:
                break
            sub = chr(_toupper(aux[s]))
            cnt, = struct.unpack_from("<I", aux, s + 1)
            esz = 1 if sub in "CA" else 2 if sub == "S" else 4
            if cnt * esz > n - s:
                break
            s += 5 + cnt * esz
        else:
            break
    if xa is None:
        return (False, 0, b"")
    nm = 0
    if nmv is not None:
        fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<i"}.get(chr(aux[nmv]))
        if fmt and nmv + 1 + struct.calcsize(fmt) <= n:
            nm = struct.unpack_from(fmt, aux, nmv + 1)[0]
    st = b""
    if chr(aux[xa]) in "ZH":
        z = aux.find(b"\0", xa + 1)
        st = aux[xa + 1:] if z < 0 else aux[xa + 1:z]
    return (True, nm, st)
