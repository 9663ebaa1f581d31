// itx_bairule.h — what one BAM record contributes to the .bai index of `iteres filter -b -i` (SAM v1 section 5.2), stated once for
// the device (csrc/itx_bamidx.hip), for the host and for the host build the tests hold against a Python restatement
// (tests/bairule_host.cpp). Plain C over bytes and integers, valid as C and as C++.
//
//   fields   tid, pos, n_cigar_op and the CIGAR are read from the record's bytes (rec points at its block_size field)
//   end      pos + the lengths of the M, D, N, = and X operations; pos + 1 when they add up to 0
//   bin      reg2bin(pos, end) of the specification: computed, the record's own bin field is not looked at
//   windows  the 16 KiB windows pos >> 14 .. (end - 1) >> 14 of the linear index
//   voff     the virtual offset of byte s of the record stream: the stream is cut into payloads of P bytes, payload k is the
//            member that starts coff[k] bytes behind the first record member, which starts at byte F of the file:
//            (F + coff[s / P]) << 16 | s % P. coff has one more element than there are members: the members' total, so that
//            a record that ends exactly on a payload boundary ends at the start of whatever follows.
//   a record's chunk is [voff(s), voff(s + 4 + block_size))
// An index can be made for coordinates up to ITX_BAI_MAX_END = 2^29 (the bins' six levels end there).
#pragma once
#include <stdint.h>

#ifndef ITX_BAI_FN
#ifdef __HIPCC__
#define ITX_BAI_FN static __host__ __device__ inline
#else
#define ITX_BAI_FN static inline
#endif
#endif

#define ITX_BAI_MAX_END (1ll << 29)
#define ITX_BAI_PSEUDO_BIN 37450u
#define ITX_BAI_WIN_SHIFT 14
#define ITX_BAI_MAX_REFS 65536       /* the sort key is tid << 16 | bin in 32 bits */

/* why no index was made (itx_bamout_index_result.status) */
#define ITX_BAI_OK 0
#define ITX_BAI_UNSORTED 1           /* some (tid, pos) is below its predecessor's */
#define ITX_BAI_BEYOND_MAX 2         /* a record ends beyond 2^29 */
#define ITX_BAI_BEYOND_REF 3         /* a record ends beyond its reference's l_ref (or names no reference of the header) */
#define ITX_BAI_TOO_MANY_REFS 4      /* n_ref >= 2^16 */

typedef struct ItxBaiRec {
    int32_t tid, pos;
    uint32_t n_cigar;
    int64_t end;
} ItxBaiRec;

ITX_BAI_FN uint32_t itx_bai_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* the specification's reg2bin over [beg, end), end <= 2^29 */
ITX_BAI_FN uint32_t itx_bai_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

/* the reference bases of a CIGAR of n operations at c (4 bytes each, length << 4 | op): M = 0, D = 2, N = 3, '=' = 7, X = 8 */
ITX_BAI_FN int64_t itx_bai_ref_len(const uint8_t *c, uint32_t n)
{
    int64_t sum = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t v = itx_bai_u32(c + 4u * k), op = v & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) sum += (int64_t)(v >> 4);
    }
    return sum;
}

/* rec: the record from its block_size field on, `len` = 4 + block_size bytes. A CIGAR that would reach beyond the record is cut
 * where the record ends (such a record is malformed; nothing outside it is read). */
ITX_BAI_FN void itx_bai_fields(const uint8_t *rec, uint32_t len, ItxBaiRec *o)
{
    if (len < 36u) {                                                       /* no fixed part: names no reference */
        o->tid = o->pos = -1;
        o->n_cigar = 0;
        o->end = 0;
        return;
    }
    o->tid = (int32_t)itx_bai_u32(rec + 4);
    o->pos = (int32_t)itx_bai_u32(rec + 8);
    const uint32_t l_name = rec[12];
    uint32_t n = (uint32_t)rec[16] | (uint32_t)rec[17] << 8;
    const uint32_t at = 36u + l_name;
    if (at > len) n = 0;
    else if (n > (len - at) / 4u) n = (len - at) / 4u;
    o->n_cigar = n;
    const int64_t ref = n ? itx_bai_ref_len(rec + at, n) : 0;
    o->end = (int64_t)o->pos + (ref ? ref : 1);
}

/* 0, or why the record cannot be indexed; l_ref: the header's reference lengths */
ITX_BAI_FN int itx_bai_refuses(const ItxBaiRec *r, int32_t n_ref, const int32_t *l_ref)
{
    if (r->tid < 0 || r->tid >= n_ref || r->pos < 0) return ITX_BAI_BEYOND_REF;
    if (r->end > ITX_BAI_MAX_END) return ITX_BAI_BEYOND_MAX;
    if (r->end > (int64_t)l_ref[r->tid]) return ITX_BAI_BEYOND_REF;
    return ITX_BAI_OK;
}

ITX_BAI_FN uint32_t itx_bai_key(int32_t tid, uint32_t bin) { return (uint32_t)tid << 16 | bin; }
ITX_BAI_FN uint32_t itx_bai_win_first(int32_t pos) { return (uint32_t)pos >> ITX_BAI_WIN_SHIFT; }
ITX_BAI_FN uint32_t itx_bai_win_last(int64_t end) { return (uint32_t)((end - 1) >> ITX_BAI_WIN_SHIFT); }

/* the windows a reference of l_ref bases can have: what sizes its part of the linear index */
ITX_BAI_FN uint32_t itx_bai_windows(int32_t l_ref)
{
    int64_t l = l_ref < 0 ? 0 : l_ref;
    if (l > ITX_BAI_MAX_END) l = ITX_BAI_MAX_END;
    return (uint32_t)((l + (1 << ITX_BAI_WIN_SHIFT) - 1) >> ITX_BAI_WIN_SHIFT);
}

ITX_BAI_FN uint64_t itx_bai_voff(uint64_t first_member_offset, const uint64_t *coff, uint64_t s, uint32_t payload)
{
    return (first_member_offset + coff[s / payload]) << 16 | (s % payload);
}
