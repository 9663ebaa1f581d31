// itx_derive.h — the record derivation (generic.c:764-905): does a record reach the lookup, and with which start,
// end and strand. Stated twice, both here:
//   itx_derive()             the rule as the reference branches it, for every user off the hot path (-R, the XA veto,
//                            the host's bed lines). Plain C: the host program (gcc, C11) includes this file too.
//   lut_entry + derive_one   the form k_stream runs: what the flag bits decide tabulated once per workgroup, the
//                            coordinates without branches. C++ only.
// tests/test_derive.py builds both for the host and holds them equal, and equal to the test suite's own statement.
#pragma once
#include <stdint.h>

// Function attributes; an including file may set its own (cf. ITXI_FN of itx_inflate_core.h).
#ifndef ITX_DERIVE_FN
#ifdef __HIPCC__
#define ITX_DERIVE_FN static __host__ __device__ inline
#else
#define ITX_DERIVE_FN static inline
#endif
#endif

// flag5 bits (include/iteres_amd.h)
#define F5_PAIRED 1u
#define F5_UNMAP 2u
#define F5_MUNMAP 4u
#define F5_REVERSE 8u
#define F5_READ1 16u
#define F5_NOLOOKUP 32u

// The options the rule reads (-Q, -E, -I, -T, -D).
typedef struct ItxDeriveOpts {
    uint32_t mapq_min, extension, isize_max;
    int32_t treat, discard;
} ItxDeriveOpts;

// generic.c:764-905 for one record. chrom: the record's chromosome in the size file, < 0 when it has none (dropped by
// -C, not in the file); size: that chromosome's size. Returns whether the record reaches reads_mapped++; then *start,
// *end are the reference's unsigned coordinates and *strand is 0 for '+', 1 for '-'.
ITX_DERIVE_FN int itx_derive(const ItxDeriveOpts *o, int32_t chrom, int32_t size, uint32_t flag5, int32_t pos, int32_t tmpend, int32_t mpos,
                             int32_t isize, uint32_t *start, uint32_t *end, uint32_t *strand)
{
    if (flag5 & F5_UNMAP) return 0;                                    // generic.c:764
    if (chrom < 0) return 0;                                           // generic.c:781-801
    const uint32_t cend = (uint32_t)(size - 1);                        // generic.c:796
    if (cend == 1u) return 0;
    int se;
    if (o->treat || !(flag5 & F5_PAIRED)) {
        se = 1;
    } else if (!(flag5 & F5_MUNMAP)) {                                 // generic.c:836-860
        if (!(flag5 & F5_READ1)) return 0;
        const uint32_t a = isize < 0 ? 0u - (uint32_t)isize : (uint32_t)isize;
        if (a > o->isize_max || isize == 0) return 0;
        se = 0;
    } else {
        if (o->discard) return 0;                                      // generic.c:862-863
        se = 1;
    }
    uint32_t st, en, sd;
    if (se) {                                                          // generic.c:819-833
        st = (uint32_t)pos;
        en = cend < (uint32_t)tmpend ? cend : (uint32_t)tmpend;
        sd = (flag5 & F5_REVERSE) ? 1u : 0u;
        if (o->extension) {
            if (!sd) {
                const uint32_t e2 = st + o->extension;
                en = e2 < cend ? e2 : cend;
            } else {
                st = en < o->extension ? 0u : en - o->extension;
            }
        }
    } else if (isize > 0) {                                            // generic.c:845-855
        st = (uint32_t)pos;
        const uint32_t e2 = st + (uint32_t)isize;
        en = cend < e2 ? cend : e2;
        sd = 0u;
    } else {
        st = (uint32_t)mpos;
        const uint32_t e2 = st - (uint32_t)isize;
        en = cend < e2 ? cend : e2;
        sd = 1u;
    }
    *start = st;
    *end = en;
    *strand = sd;
    return 1;
}

#ifdef __cplusplus
#include "itx_common.h"

// One record's raw fields as the host decoder hands them over.
struct ItxRaw {
    int32_t tid, pos, tmpend;
    uint32_t mapq, fl;
};

__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t imin32(int32_t a, int32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t imax32(int32_t a, int32_t b) { return a > b ? a : b; }

// Everything generic.c:748-922 decides from a record's flag bits alone, tabulated once per workgroup.
// Index: flag5 (6 bits) | 64 the reference is known and usable (generic.c:781-801) | 128 a proper-pair insert size
// (generic.c:838-840) | 256 MAPQ >= -Q. Entry: bit 3k set => cnt[k] += 1 for k in 0..7 (generic.c:1048-1055;
// cnt[11] == cnt[7] without -R), LUT_OK the record goes on to the lookup, LUT_SE it is measured as a single end.
#define LUT_OK (1u << 24)
#define LUT_SE (1u << 25)
__device__ __forceinline__ uint32_t lut_entry(const ItxRunParams &P, uint32_t idx)
{
    const bool paired = idx & F5_PAIRED, unmap = idx & F5_UNMAP, munmap = idx & F5_MUNMAP, read1 = idx & F5_READ1;
    const bool ref_ok = idx & 64u, isz_ok = idx & 128u, uniq = idx & 256u;
    const bool treat = P.treat != 0;
    const bool end1 = !paired || read1 || treat;                                   // generic.c:748-759
    const bool mapped = !unmap;                                                    // generic.c:764
    const bool chrom_ok = mapped && ref_ok;                                        // generic.c:781-801
    const bool se = treat || !paired || munmap;                                    // generic.c:815,836-837,885
    const bool pe_ok = read1 && isz_ok;                                            // generic.c:838-840,858-860
    const bool se_ok = treat || !paired || P.discard == 0;                         // generic.c:862-863
    const bool ok = chrom_ok && (se ? se_ok : pe_ok);
    uint32_t e = end1 ? 1u : 1u << 3;
    e |= mapped ? (end1 ? 1u << 6 : 1u << 9) : 0u;
    e |= chrom_ok ? (end1 ? 1u << 12 : 1u << 15) : 0u;
    e |= ok ? 1u << 18 : 0u;
    e |= (ok && uniq) ? 1u << 21 : 0u;
    return e | ((ok && !(idx & F5_NOLOOKUP)) ? LUT_OK : 0u) | (se ? LUT_SE : 0u);      // the caller's -R / XA `continue`
}

// generic.c:748-922 for one record. (tx, ty) = chrom and size of the record's ItxTidRec, has_rows = its reference
// has table rows. Out: the flag table's entry, the reference's unsigned start/end, binKeeperFind's clipped query
// (binRange.c:204-206), whether the record goes on to the lookup, and MAPQ >= -Q.
// The caller's contract: s_lut[i] = lut_entry(P, i) for i < 512 and 0 above; tile_pe may be false only when no
// record of the tile has F5_PAIRED set (iz and mpos are then not looked at), and is true otherwise.
__device__ __forceinline__ void derive_one(const ItxRunParams &P, const uint32_t *s_lut, const ItxRaw &r, int32_t iz, int32_t mpos, bool tile_pe,
                                           uint32_t tx, uint32_t ty, bool has_rows, uint32_t &lut, uint32_t &st, uint32_t &en, int32_t &qs,
                                           int32_t &qe, bool &q, bool &uq)
{
    const uint32_t cend = ty - 1u;                                                 // generic.c:796
    uq = r.mapq >= P.mapq_min;
    uint32_t idx = r.fl | (((int32_t)tx >= 0 && cend != 1u) ? 64u : 0u) | (uq ? 256u : 0u);
    // generic.c:819-833
    uint32_t s_se = (uint32_t)r.pos;
    uint32_t e_se = umin32(cend, (uint32_t)r.tmpend);
    if (P.extension) {                                                             // wave-uniform
        const bool rev = r.fl & F5_REVERSE;
        const uint32_t e_plus = umin32(s_se + P.extension, cend);
#ifndef __HIPCC__
        const uint32_t s_minus = e_se > P.extension ? e_se - P.extension : 0u;     // host builds (tests): no clang builtin
#else
        const uint32_t s_minus = __builtin_elementwise_sub_sat(e_se, P.extension);
#endif
        s_se = rev ? s_minus : s_se;
        e_se = rev ? e_se : e_plus;
    }
    st = s_se;
    en = e_se;
    if (tile_pe) {                                                                 // wave-uniform; generic.c:838-855
        const uint32_t aisz = iz < 0 ? 0u - (uint32_t)iz : (uint32_t)iz;
        idx |= (aisz <= P.isize_max && iz != 0) ? 128u : 0u;
        lut = s_lut[idx];
        const bool se = lut & LUT_SE;
        const bool fwd = iz > 0;
        const uint32_t s_pe = fwd ? (uint32_t)r.pos : (uint32_t)mpos;
        const uint32_t e_pe = umin32(cend, fwd ? s_pe + (uint32_t)iz : s_pe - (uint32_t)iz);
        st = se ? s_se : s_pe;
        en = se ? e_se : e_pe;
    } else {
        lut = s_lut[idx];
    }
    qs = imax32((int32_t)st, 0);
    qe = imin32((int32_t)en, (int32_t)ty);
    q = (lut & LUT_OK) && qs < qe && has_rows;
}
#endif
