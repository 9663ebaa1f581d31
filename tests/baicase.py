"""The .bai index of `filter -b -i`, restated in Python from the rule alone (SAM v1 section 5.2 and the canonical choices the
project documents); it shares no code with the product.

  expected(l_ref, stream, member_sizes, first)   the index a record stream must get: (status, bytes or None)
  expected_for_file(bam bytes)                   the same for an emitted BAM file: its BGZF members are walked for their file offsets
  parse_bai / reg2bins / fetch                   an independent BAI reader and a region fetch the specification's way: the chunks of
                                                 the region's bins, the linear index's minimum offset, then reading from the virtual
                                                 offset
  linear_scan                                    the records that overlap a region, found by walking all of them
  with_bin / bam_file                            a record with the bin of its own interval, and a BAM file in the product's layout
                                                 from a header and a record list, for readers that trust the bin field"""
import bisect
import struct

import refio
from iteres_amd import synth

PAYLOAD = 8192                      # bytes of the record stream per member (csrc/itx_bgzfmember.h ITX_BAMOUT_PAYLOAD)
MAX_END = 1 << 29
PSEUDO = 37450
OK, UNSORTED, BEYOND_MAX, BEYOND_REF, TOO_MANY_REFS = 0, 1, 2, 3, 4
REF_CONSUMING = (0, 2, 3, 7, 8)     # M D N = X


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def record_fields(buf, at):
    """(tid, pos, end, length) of the record whose block_size field is at buf[at]"""
    bs, tid, pos = struct.unpack_from("<Iii", buf, at)
    l_name = buf[at + 12]
    n_cigar, = struct.unpack_from("<H", buf, at + 16)
    ref = 0
    for v in struct.unpack_from("<%dI" % n_cigar, buf, at + 36 + l_name):
        if v & 15 in REF_CONSUMING:
            ref += v >> 4
    return tid, pos, pos + (ref or 1), 4 + bs


def records_of(stream):
    """[(tid, pos, end, stream offset, length)] of whole records one behind the other"""
    out, at = [], 0
    while at < len(stream):
        tid, pos, end, ln = record_fields(stream, at)
        out.append((tid, pos, end, at, ln))
        at += ln
    assert at == len(stream)
    return out


def with_bin(rec):
    """the record with reg2bin(pos, end) in its bin field (bedcase.record stores 4681 whatever the interval)"""
    tid, pos, end, ln = record_fields(rec, 0)
    assert ln == len(rec)
    out = bytearray(rec)
    struct.pack_into("<H", out, 14, reg2bin(pos, end))
    return bytes(out)


def bam_file(header, records, payload=PAYLOAD, sorted_=True):
    """the bytes of a BAM file laid out as `filter -b` lays it out: the header in members of its own, the records' stream cut every
    `payload` bytes whatever the records' boundaries, the EOF member. header: [(name, length)]; every record gets its own bin"""
    text = ("@HD\tVN:1.0\tSO:%s\n" % ("coordinate" if sorted_ else "unsorted") + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in header)).encode()
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(header))
    for n, l in header:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    stream = b"".join(with_bin(r) for r in records)
    return b"".join(synth.bgzf_block(part[i:i + payload]) for part in (head, stream) for i in range(0, len(part), payload)) + synth.BGZF_EOF


def member_walk(data):
    """[(file offset, compressed size, ISIZE)] of the BGZF members of data"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04", at
        xlen, = struct.unpack_from("<H", data, at + 10)
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2) == (66, 67):
                bsize, = struct.unpack_from("<H", data, x + 4)
            x += 4 + slen
        assert bsize is not None
        size = bsize + 1
        isize, = struct.unpack_from("<I", data, at + size - 4)
        out.append((at, size, isize))
        at += size
    assert at == len(data)
    return out


def expected(l_ref, stream, member_sizes, first, payload=PAYLOAD):
    """(status, the .bai bytes or None) for the record stream `stream`, cut into members of these compressed sizes, the first of
    which starts at file offset `first`"""
    if len(l_ref) >= 1 << 16:
        return TOO_MANY_REFS, None
    assert len(member_sizes) == -(-len(stream) // payload)
    coff = [0]
    for z in member_sizes:
        coff.append(coff[-1] + z)

    def voff(s):
        return (first + coff[s // payload]) << 16 | s % payload

    recs = records_of(stream)
    why = set()
    for i, (tid, pos, end, s, ln) in enumerate(recs):
        if i and (tid, pos) < recs[i - 1][:2]:
            why.add(UNSORTED)
        if not 0 <= tid < len(l_ref) or pos < 0:
            why.add(BEYOND_REF)
        elif end > MAX_END:
            why.add(BEYOND_MAX)
        elif end > l_ref[tid]:
            why.add(BEYOND_REF)
    if why:
        return min(why), None
    bins = [dict() for _ in l_ref]         # bin -> chunks [beg, end] in file order
    lin = [dict() for _ in l_ref]
    span = [None] * len(l_ref)             # [first voff, last end voff, records]
    prev = None
    for tid, pos, end, s, ln in recs:
        b = reg2bin(pos, end)
        beg_v, end_v = voff(s), voff(s + ln)
        chunks = bins[tid].setdefault(b, [])
        if prev == (tid, b):
            chunks[-1][1] = end_v          # the run goes on: one chunk
        elif chunks and chunks[-1][1] >> 16 >= beg_v >> 16:
            chunks[-1][1] = end_v          # a new run, merged into the bin's chunk before it
        else:
            chunks.append([beg_v, end_v])
        prev = (tid, b)
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            if w not in lin[tid] or beg_v < lin[tid][w]:
                lin[tid][w] = beg_v
        if span[tid] is None:
            span[tid] = [beg_v, end_v, 0]
        span[tid][1] = end_v
        span[tid][2] += 1
    out = [b"BAI\1", struct.pack("<i", len(l_ref))]
    for tid in range(len(l_ref)):
        out.append(struct.pack("<i", len(bins[tid]) + (span[tid] is not None)))
        for b in sorted(bins[tid]):
            out.append(struct.pack("<Ii", b, len(bins[tid][b])))
            for c in bins[tid][b]:
                out.append(struct.pack("<QQ", *c))
        if span[tid] is not None:
            out.append(struct.pack("<IiQQQQ", PSEUDO, 2, span[tid][0], span[tid][1], span[tid][2], 0))
        n_intv = max(lin[tid]) + 1 if lin[tid] else 0
        out.append(struct.pack("<i", n_intv))
        last = 0
        for w in range(n_intv):
            last = lin[tid].get(w, last)
            out.append(struct.pack("<Q", last))
    out.append(struct.pack("<Q", 0))
    return OK, b"".join(out)


def split_bam(data):
    """an emitted BAM file -> (l_ref, the record stream, the record members' sizes, the first record member's file offset, the
    whole inflated text, {file offset of a member: where its text starts in the inflated text})"""
    mem = member_walk(data)
    raw = refio.bgzf_decompress(data)
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    l_ref = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        l_ref.append(struct.unpack_from("<i", raw, at + 4 + l_name)[0])
        at += 8 + l_name
    ustart, u = {}, 0
    for off, size, isize in mem:
        ustart[off] = u
        u += isize
    assert u == len(raw)
    # the header lies in members of its own: the first record member is the one whose text starts where the header ends
    first = next(off for off, size, isize in mem if ustart[off] == at and (isize or at == len(raw)))
    sizes = [size for off, size, isize in mem if off >= first and isize]
    return l_ref, raw[at:], sizes, first, raw, ustart


def expected_for_file(data):
    l_ref, stream, sizes, first, raw, ustart = split_bam(data)
    return expected(l_ref, stream, sizes, first)


# ---- an independent reader

def parse_bai(b):
    """[{"bins": {bin: [(beg, end)]}, "meta": (first, last, n, 0) or None, "lin": [ioffset]}] per reference"""
    assert b[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", b, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", b, at)
        at += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            bn, n_chunk = struct.unpack_from("<Ii", b, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", b, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if bn == PSEUDO:
                assert n_chunk == 2 and meta is None
                meta = chunks[0] + chunks[1]
            else:
                assert bn not in bins and bn < PSEUDO
                bins[bn] = chunks
        n_intv, = struct.unpack_from("<i", b, at)
        at += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, b, at))
        at += 8 * n_intv
        refs.append({"bins": bins, "meta": meta, "lin": lin})
    n_no_coor, = struct.unpack_from("<Q", b, at)
    assert at + 8 == len(b) and n_no_coor == 0
    return refs


def fetch(idx, raw, ustart, tid, beg, end):
    """the records (their offsets in the inflated text `raw`) of [beg, end) on tid, found through the parsed index `idx`:
    the chunks of the region's bins whose end lies above the linear index's minimum offset, read record by record from each
    chunk's virtual offset up to its end"""
    ref = idx[tid]
    lin = ref["lin"]
    min_off = lin[min(beg >> 14, len(lin) - 1)] if lin else 0
    found = set()
    for bn in reg2bins(beg, end):
        for cb, ce in ref["bins"].get(bn, ()):
            if ce <= min_off:
                continue
            u = ustart[cb >> 16] + (cb & 0xffff)
            u_end = ustart[ce >> 16] + (ce & 0xffff)
            while u < u_end:
                rt, rp, re_, ln = record_fields(raw, u)
                if rt == tid and rp < end and re_ > beg:
                    found.add(u)
                u += ln
            assert u == u_end
    return found


def linear_scan(raw, at, tid, beg, end):
    """the same set by walking every record of the inflated text from the header's end"""
    found = set()
    while at < len(raw):
        rt, rp, re_, ln = record_fields(raw, at)
        if rt == tid and rp < end and re_ > beg:
            found.add(at)
        at += ln
    return found
