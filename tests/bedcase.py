"""Records with awkward names and tags as raw BAM bytes, an independent reading of them (the tags: tests/auxmodel.py), and the bed lines of `stat -B / -V`
formatted from that reading with Python's own `%` — what tests/test_bedline.py and tests/test_gpu_bed.py hold the shared line
rule (iteres_amd/csrc/itx_bedline.h) and the device build (csrc/itx_bed.hip) against. The derivation of (start, end, strand)
is goldencase.derive_py, the suite's own statement of generic.c:764-905."""
import struct

import numpy as np

import auxmodel
import goldencase as gc
import refio
from iteres_amd import synth


def record(tid=0, pos=100, mapq=37, flag=0, qname=b"r1\0", cigar=((0, 50),), l_qseq=0, mtid=-1, mpos=-1, isize=0, aux=b"", l_qname=None):
    """One BAM record (block_len included). qname: the bytes as they lie in the record (the NUL is the caller's); cigar: (op, len)."""
    lq = len(qname) if l_qname is None else l_qname
    body = struct.pack("<iiIIiiii", tid, pos, (4681 << 16) | (mapq << 8) | lq, (flag << 16) | len(cigar), l_qseq, mtid, mpos, isize)
    body += qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    body += bytes((l_qseq + 1) // 2) + bytes([30]) * l_qseq + aux
    return struct.pack("<i", len(body)) + body


def tag(name, ty, payload):
    return name.encode() + ty.encode() + payload


def bam_bytes(header, records, block=0xff00):
    text = "@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in header)
    buf = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(header))
    for n, l in header:
        nb = n.encode() + b"\0"
        buf += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
    buf += b"".join(records)
    return b"".join(synth.bgzf_block(buf[i:i + block]) for i in range(0, len(buf), block)) + synth.BGZF_EOF


# ---- the independent reading

def read_record(rec):
    """qname / XA / NM of one record the way the reference takes them: bam1_qname up to its NUL; XA and NM by the literal model of
    bam_aux_get, bam_aux2Z and bam_aux2i (tests/auxmodel.py), with the project's rule where the reference leaves the record"""
    bl, = struct.unpack_from("<i", rec, 0)
    tid, pos, x1, x2, l_qseq, mtid, mpos, isize = struct.unpack_from("<iiIIiiii", rec, 4)
    lq, mapq, flag, ncig = x1 & 0xff, (x1 >> 8) & 0xff, x2 >> 16, x2 & 0xffff
    data = rec[36:4 + bl]
    qname = b""
    if lq and lq <= len(data):
        z = data.find(b"\0")
        assert z >= 0, "a name that runs out of its record is not a case of these tests"
        qname = data[:z]
    e = pos
    for k in range(ncig):
        c, = struct.unpack_from("<I", data, lq + 4 * k)
        if c & 0xf in (0, 2, 3):
            e += c >> 4
    tmpend = e if ncig else pos + l_qseq
    a = auxmodel.answer(rec)
    return dict(tid=tid, pos=pos, tmpend=tmpend, mapq=mapq, flag=flag,
                mpos=mpos, isize=isize, qname=qname, has_xa=a.has_xa, xa=a.p_xa, nm=a.p_nm)


def soa(recs):
    rd = [read_record(r) for r in recs]
    return rd, {k: np.array([x[k] for x in rd], np.int64) for k in ("tid", "pos", "tmpend", "mapq", "flag", "mpos", "isize")}


def params(**kw):
    p = dict(mapq_min=10, min_cov=1e-4, extension=150, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False)
    p.update(kw)
    return p


def lines(p, header, chrom_names, chrom_size, recs, add_chr=False, skip=None):
    """(-B text, -V text) the reference prints for these records (generic.c:925-936); skip[i]: record i left through -R"""
    names = [gc.rename_chr(n, add_chr) for n, _ in header]
    t2c = [(-2 if nm is None else (chrom_names.index(nm) if nm in chrom_names and chrom_size[chrom_names.index(nm)] != 2 else -1)) for nm in names]
    rd, arr = soa(recs)
    b, v = [], []
    for i, r in enumerate(rd):
        d = gc.derive_py(p, t2c, chrom_size, arr, i)
        if d is None or (skip is not None and skip[i]):
            continue
        start, end, strand = d
        base = b"%s\t%u\t%u\t%s\t%i\t%c" % (names[r["tid"]].encode(), start, end, r["qname"], r["mapq"], strand.encode())
        b.append(base + (b"\t%i\t%s" % (r["nm"], r["xa"]) if r["has_xa"] else b"") + b"\n")
        if r["mapq"] >= p["mapq_min"]:
            v.append(base + b"\n")
    return b"".join(b), b"".join(v), t2c, names


def corner_records(n_chrom_tids=4):
    """The content the line rule has to get right, as records on tids 0 .. n_chrom_tids - 1"""
    R = []
    xa1 = tag("XA", "Z", b"chr1,+100,36M,0;\0")
    for k, qn in enumerate([b"\0", b"a\0", b"q" * 254 + b"\0", b"ab\0cd\0", b"name\0"]):
        R.append(record(tid=k % n_chrom_tids, pos=10 + k, qname=qn, aux=xa1 if k & 1 else b""))
    R.append(record(qname=b"", l_qname=0, pos=7))                                         # l_qname == 0: an empty name
    for mq in (0, 9, 10, 255):
        R.append(record(mapq=mq, pos=1000, flag=16, aux=xa1))
    for pos in (0, 1, 9, 10, 99, 12345, 999999, 1234567, 99999999, 123456789, 1999999999, 2147483000, 2147483647):
        R.append(record(tid=3 % n_chrom_tids, pos=pos, cigar=((0, 1),), qname=b"p%d\0" % pos))
        R.append(record(tid=3 % n_chrom_tids, pos=pos, cigar=((0, 36),), flag=16, qname=b"m%d\0" % pos))
    nms = [("c", struct.pack("<b", -5)), ("C", struct.pack("<B", 200)), ("s", struct.pack("<h", -30000)), ("S", struct.pack("<H", 65535)),
           ("i", struct.pack("<i", -2147483648)), ("I", struct.pack("<I", 4000000000)), ("i", struct.pack("<i", 2147483647)), ("f", struct.pack("<f", 2.5)),
           ("Z", b"12\0"), ("A", b"7")]
    for ty, payload in nms:
        R.append(record(pos=500, aux=tag("NM", ty, payload) + xa1))
        R.append(record(pos=501, aux=xa1 + tag("NM", ty, payload)))
    R.append(record(pos=600, aux=tag("NM", "C", b"\3")))                                   # NM without XA: not printed
    R.append(record(pos=601, aux=tag("XA", "Z", b"\0")))                                   # an empty XA
    R.append(record(pos=602, aux=tag("X0", "i", struct.pack("<i", 1)) + tag("XA", "Z", b"chr2,-5,10M,1;" * 400 + b"\0") + tag("NM", "C", b"\1")))
    R.append(record(pos=603, aux=tag("NM", "C", b"\2") + tag("XA", "Z", b"no terminating NUL;")))
    R.append(record(pos=604, aux=tag("XA", "i", struct.pack("<i", 7)) + tag("NM", "C", b"\4")))
    R.append(record(pos=605, aux=tag("ZB", "B", b"S" + struct.pack("<I", 3) + bytes(6)) + tag("XA", "Z", b"after,+1,2M,0;\0") + tag("NM", "s", struct.pack("<h", 300))))
    R.append(record(pos=606, aux=tag("ZB", "B", b"i" + struct.pack("<I", 1000) + bytes(8)) + tag("XA", "Z", b"unreachable\0")))   # an array that overruns the record
    R.append(record(pos=607, aux=tag("XA", "H", b"1AE301\0") + tag("XA", "Z", b"second\0")))
    R.append(record(pos=608, aux=tag("Zq", "?", b"xx") + tag("XA", "Z", b"behind an unknown type\0")))
    R.append(record(pos=609, flag=4, aux=xa1))                                             # unmapped: no line
    R.append(record(tid=-1, pos=-1, flag=4, qname=b"un\0"))
    R.append(record(pos=700, flag=0x1 | 0x40, mtid=0, mpos=900, isize=250, l_qseq=40, aux=xa1))
    R.append(record(pos=900, flag=0x1 | 0x40 | 0x10, mtid=0, mpos=700, isize=-250, l_qseq=40))
    R.append(record(pos=900, flag=0x1 | 0x80, mtid=0, mpos=700, isize=-250))
    R.append(record(pos=950, flag=0x1 | 0x40 | 0x8, mtid=-1, mpos=-1, isize=0, aux=xa1))
    R.append(record(pos=960, flag=0x1 | 0x40, mtid=0, mpos=99000, isize=5000))
    R.append(record(pos=970, cigar=(), l_qseq=25, qname=b"nocigar\0"))
    return R
