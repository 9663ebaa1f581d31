// itx_bamsortrule.h — the coordinate order of `iteres filter -b -s`, stated once for the device (csrc/itx_bamout_sort.hip), for the host
// (host/stream.c) and for the host build the tests hold against a Python restatement (tests/bamsortrule_host.cpp). Plain C over bytes
// and integers, valid as C and as C++.
//
//   key      (tid, pos, reverse) read from the record's bytes (rec points at its block_size field), reverse = (flag >> 4) & 1.
//            Records ascend by tid, then pos, then reverse: the coordinate comparison of `samtools sort` 1.x. The samtools 0.1.18
//            that the reference vendors compares tid and pos alone (bam_sort.c bam1_lt), so this order is one of those its rule
//            allows, and its stable sort leaves a file in this order as it is (tests/test_bam_vs_reference.py). Records with equal
//            keys stay in input order (the sort is stable). Every counted record is mapped, so tid >= 0 and pos >= 0 hold; a record
//            that breaks this (or has no fixed part) is reported and no sorted file is written.
//   low key  pos << 1 | reverse, 32 bits; high key: tid. The radix sort runs over the low key's 4 bytes, then over as many bytes
//            of tid as n_ref - 1 has (itx_bamsort_high_passes).
//   header   the text of the BAM header under -s: an @HD line at the start keeps its fields in order except SO, GO and SS, and
//            SO:coordinate becomes its last field; without one, "@HD\tVN:1.6\tSO:coordinate\n" is put in front. Everything behind
//            the first line stays byte for byte, trailing NULs included.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef ITX_BSR_FN
#ifdef __HIPCC__
#define ITX_BSR_FN static __host__ __device__ inline
#else
#define ITX_BSR_FN static inline
#endif
#endif

typedef struct ItxBamSortKey {
    int32_t tid, pos;
    uint32_t reverse;
} ItxBamSortKey;

ITX_BSR_FN uint32_t itx_bamsort_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* rec: the record from its block_size field on, `len` = 4 + block_size bytes. Returns 0, or 1 when the record cannot take part in
 * a coordinate sort of mapped records (no fixed part, tid < 0 or pos < 0); the fields are filled either way. */
ITX_BSR_FN int itx_bamsort_key(const uint8_t *rec, uint32_t len, ItxBamSortKey *k)
{
    if (len < 36u) {
        k->tid = k->pos = -1;
        k->reverse = 0;
        return 1;
    }
    k->tid = (int32_t)itx_bamsort_u32(rec + 4);
    k->pos = (int32_t)itx_bamsort_u32(rec + 8);
    k->reverse = (((uint32_t)rec[18] | (uint32_t)rec[19] << 8) >> 4) & 1u;
    return k->tid < 0 || k->pos < 0;
}

ITX_BSR_FN uint32_t itx_bamsort_low(const ItxBamSortKey *k) { return (uint32_t)k->pos << 1 | k->reverse; }
ITX_BSR_FN uint32_t itx_bamsort_high(const ItxBamSortKey *k) { return (uint32_t)k->tid; }

/* 8-bit passes over the high key for n_ref references: ceil(bits(n_ref - 1) / 8); none for one reference */
ITX_BSR_FN uint32_t itx_bamsort_high_passes(uint32_t n_ref)
{
    uint32_t bits = 0, v;
    for (v = n_ref > 0 ? n_ref - 1u : 0u; v; v >>= 1) bits++;
    return (bits + 7u) / 8u;
}

#define ITX_BAMSORT_HD "@HD\tVN:1.6\tSO:coordinate\n"
#define ITX_BAMSORT_SO "\tSO:coordinate"
#define ITX_BAMSORT_HEADER_GROWTH 32u    /* the new text is at most this much longer than the old */

/* The header text under -s. text[0 .. len) -> out, which has room for len + ITX_BAMSORT_HEADER_GROWTH bytes (out may be NULL: only
 * the length is wanted); returns the new length. The first line ends before the first '\n' or NUL, or where the text ends. */
static inline size_t itx_bamsort_header_text(const char *text, size_t len, char *out)
{
    size_t n = 0, eol = 0, at = 0;
    const size_t l_hd = sizeof(ITX_BAMSORT_HD) - 1, l_so = sizeof(ITX_BAMSORT_SO) - 1;
    while (eol < len && text[eol] != '\n' && text[eol] != '\0') eol++;
    if (!(eol >= 3 && text[0] == '@' && text[1] == 'H' && text[2] == 'D' && (eol == 3 || text[3] == '\t'))) {
        if (out) {
            memcpy(out, ITX_BAMSORT_HD, l_hd);
            if (len) memcpy(out + l_hd, text, len);
        }
        return l_hd + len;
    }
    while (at < eol) {                                                     /* field by field; every one but the first begins with its tab */
        size_t end = at + 1;
        while (end < eol && text[end] != '\t') end++;
        const int tagged = at != 0 && end - at >= 4 && text[at + 3] == ':';
        const int drop = tagged && ((text[at + 1] == 'S' && text[at + 2] == 'O') || (text[at + 1] == 'G' && text[at + 2] == 'O') ||
                                    (text[at + 1] == 'S' && text[at + 2] == 'S'));
        if (!drop) {
            if (out) memcpy(out + n, text + at, end - at);
            n += end - at;
        }
        at = end;
    }
    if (out) {
        memcpy(out + n, ITX_BAMSORT_SO, l_so);
        if (len > eol) memcpy(out + n + l_so, text + eol, len - eol);
    }
    return n + l_so + (len - eol);
}
