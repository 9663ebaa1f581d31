// itx_bedline.h — one bed line of `iteres stat -B / -V` from one BAM record (generic.c:925-936):
//
//   -B   "%s\t%u\t%u\t%s\t%i\t%c"  chr start end qname mapq strand, then iff the record has an XA tag "\t%i\t%s" NM XA, "\n"
//   -V   "%s\t%u\t%u\t%s\t%i\t%c\n"                                  (the caller asks for it only when MAPQ >= -Q)
//
// stated once for the device (csrc/itx_bed.hip) and for the host build the tests hold against an independent parse
// (tests/bedline_host.cpp). Three steps, all plain C++ over bytes:
//   itx_bed_scan    what the line takes from the record's own bytes: the read name, the first XA tag and the first NM tag as
//                   bam_aux_get finds them and bam_aux2Z / bam_aux2i read them (itx_auxwalk.h)
//   itx_bed_len     the byte length of the line
//   itx_bed_write   the bytes [lo, hi) of the line, so that a line may be laid down piece by piece (a tile of lines is staged
//                   in LDS a window at a time, and a long XA string spans windows)
// Numbers are printed digit by digit, every digit from its own division by a constant power of ten (a multiply and a shift
// each, independent of one another): no chain of dependent divisions, and any digit can be had without the ones before it.
#pragma once
#include <stdint.h>

#include "itx_auxwalk.h"

#ifndef ITX_BED_FN
#ifdef __HIPCC__
#define ITX_BED_FN static __host__ __device__ inline
#else
#define ITX_BED_FN static inline
#endif
#endif

#define ITX_BED_NO_XA 0xffffffffu

// What a line is made of. chr / qname / xa point at the bytes; start, end, strand come from itx_derive (itx_derive.h).
struct ItxBedLine {
    const uint8_t *chr, *qname, *xa;
    uint32_t chr_len, qname_len, xa_len;
    uint32_t start, end, mapq, strand;     // strand: 0 '+', 1 '-'
    int32_t nm;
    bool has_xa;
};

// What itx_bed_scan finds in a record: offsets are relative to the record's first byte (its block_len field).
struct ItxBedScan {
    uint32_t qname_len;                    // bytes up to the first NUL; 0 when l_qname == 0 or l_qname > the data length
    uint32_t xa_off, xa_len;               // xa_off == ITX_BED_NO_XA: no XA tag; a tag that has no string (itx_aux_str): length 0
    int32_t nm;
    bool hard;                             // the name has no NUL before the record ends: not modelled, the host has to look
};

ITX_BED_FN uint32_t itx_bed_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

ITX_BED_FN ItxBedScan itx_bed_scan(const uint8_t *p, bool want_xa)
{
    ItxBedScan r;
    r.qname_len = 0;
    r.xa_off = ITX_BED_NO_XA;
    r.xa_len = 0;
    r.nm = 0;
    r.hard = false;
    const uint32_t block_len = itx_bed_ld32(p);
    const uint8_t *data = p + 36;
    const uint32_t dlen = block_len - 32u;
    const uint8_t *end = data + dlen;
    const uint32_t l_qname = p[12];
    if (l_qname && l_qname <= dlen) {
        const uint8_t *z = data;
        while (z < end && *z) ++z;
        if (z == end) r.hard = true;
        r.qname_len = (uint32_t)(z - data);
    }
    if (!want_xa) return r;
    const uint8_t *as, *ae, *xa, *nmv;                              // the TYPE byte of the tag
    if (!itx_aux_bounds(p, &as, &ae)) return r;
    itx_aux_find(as, ae, ITX_AUX_TAG('X', 'A'), &xa, ITX_AUX_TAG('N', 'M'), &nmv);
    if (!xa) return r;                                              // NM is printed only next to XA
    r.nm = itx_aux_int(nmv, ae);
    r.xa_off = (uint32_t)(itx_aux_str(xa, ae, &r.xa_len) - p);
    return r;
}

ITX_BED_FN uint32_t itx_bed_declen(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
ITX_BED_FN uint32_t itx_bed_ilen(int32_t v) { return v < 0 ? 1u + itx_bed_declen(0u - (uint32_t)v) : itx_bed_declen((uint32_t)v); }

ITX_BED_FN uint32_t itx_bed_len(const ItxBedLine *L, bool with_xa)
{
    uint32_t n = L->chr_len + 1u + itx_bed_declen(L->start) + 1u + itx_bed_declen(L->end) + 1u + L->qname_len + 1u + itx_bed_declen(L->mapq) + 3u;
    if (with_xa && L->has_xa) n += 1u + itx_bed_ilen(L->nm) + 1u + L->xa_len;
    return n;
}

// ---- the bytes [lo, hi) of a line into dst[0 .. hi - lo); `pos` runs over the line
#define ITX_BED_PUT(b)                                                  \
    do {                                                                \
        if (pos >= lo && pos < hi) dst[pos - lo] = (uint8_t)(b);        \
        pos++;                                                          \
    } while (0)

ITX_BED_FN uint32_t itx_bed_put_str(uint8_t *dst, uint32_t lo, uint32_t hi, uint32_t pos, const uint8_t *s, uint32_t n)
{
    const uint32_t a = pos > lo ? pos : lo, b = pos + n < hi ? pos + n : hi;
    for (uint32_t k = a; k < b; k++) dst[k - lo] = s[k - pos];
    return pos + n;
}

ITX_BED_FN uint32_t itx_bed_put_u32(uint8_t *dst, uint32_t lo, uint32_t hi, uint32_t pos, uint32_t v)
{
    const uint32_t nd = itx_bed_declen(v);
    if (pos + nd <= lo || pos >= hi) return pos + nd;
#define ITX_BED_DIGIT(k, p10) \
    if (nd > k) ITX_BED_PUT('0' + (v / p10) % 10u);
    ITX_BED_DIGIT(9, 1000000000u)
    ITX_BED_DIGIT(8, 100000000u)
    ITX_BED_DIGIT(7, 10000000u)
    ITX_BED_DIGIT(6, 1000000u)
    ITX_BED_DIGIT(5, 100000u)
    ITX_BED_DIGIT(4, 10000u)
    ITX_BED_DIGIT(3, 1000u)
    ITX_BED_DIGIT(2, 100u)
    ITX_BED_DIGIT(1, 10u)
    ITX_BED_DIGIT(0, 1u)
#undef ITX_BED_DIGIT
    return pos;
}

ITX_BED_FN void itx_bed_write(const ItxBedLine *L, bool with_xa, uint8_t *dst, uint32_t lo, uint32_t hi)
{
    uint32_t pos = 0;
    pos = itx_bed_put_str(dst, lo, hi, pos, L->chr, L->chr_len);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_u32(dst, lo, hi, pos, L->start);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_u32(dst, lo, hi, pos, L->end);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_str(dst, lo, hi, pos, L->qname, L->qname_len);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_u32(dst, lo, hi, pos, L->mapq);
    ITX_BED_PUT('\t');
    ITX_BED_PUT(L->strand ? '-' : '+');
    if (with_xa && L->has_xa) {
        ITX_BED_PUT('\t');
        if (L->nm < 0) ITX_BED_PUT('-');
        pos = itx_bed_put_u32(dst, lo, hi, pos, L->nm < 0 ? 0u - (uint32_t)L->nm : (uint32_t)L->nm);
        ITX_BED_PUT('\t');
        pos = itx_bed_put_str(dst, lo, hi, pos, L->xa, L->xa_len);
    }
    ITX_BED_PUT('\n');
}
