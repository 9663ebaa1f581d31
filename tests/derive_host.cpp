// Host build of the record derivation (iteres_amd/csrc/itx_derive.h): the branchy rule the cold users call and the
// fast form k_stream runs, each over arrays. Test infrastructure only — tests/test_derive.py holds the two equal,
// and equal to the suite's own statement of the rule, before either runs on a GPU. The functions are the product's
// text: only the HIP headers' host definitions of __device__ / __forceinline__ stand between it and g++.
#include <stddef.h>
#include <stdint.h>
#include "../iteres_amd/csrc/itx_derive.h"

extern "C" void itx_derive_host(const ItxDeriveOpts *o, size_t n, const int32_t *chrom, const int32_t *size, const uint8_t *flag5, const int32_t *pos,
                                const int32_t *tmpend, const int32_t *mpos, const int32_t *isize, uint8_t *keep, uint32_t *start, uint32_t *end,
                                uint8_t *strand)
{
    for (size_t i = 0; i < n; i++) {
        uint32_t st = 0, en = 0, sd = 0;
        keep[i] = (uint8_t)itx_derive(o, chrom[i], size[i], flag5[i], pos[i], tmpend[i], mpos[i], isize[i], &st, &en, &sd);
        start[i] = st;
        end[i] = en;
        strand[i] = (uint8_t)sd;
    }
}

// lut_entry into a 1024-entry table exactly as k_stream fills it, then derive_one per record. (chrom, size) stand for
// the record's ItxTidRec; the reference has table rows.
extern "C" void itx_derive_fast_host(const ItxDeriveOpts *o, int tile_pe, size_t n, const int32_t *chrom, const int32_t *size, const uint8_t *flag5,
                                     const uint8_t *mapq, const int32_t *pos, const int32_t *tmpend, const int32_t *mpos, const int32_t *isize,
                                     uint32_t *lut, uint32_t *start, uint32_t *end, uint8_t *uq)
{
    ItxRunParams P = {};
    P.mapq_min = o->mapq_min;
    P.extension = o->extension;
    P.isize_max = o->isize_max;
    P.treat = o->treat;
    P.discard = o->discard;
    uint32_t s_lut[1024];
    for (uint32_t t = 0; t < 256; t++) {
        s_lut[t] = lut_entry(P, t);
        s_lut[256 + t] = lut_entry(P, 256 + t);
        s_lut[512 + t] = 0;
        s_lut[768 + t] = 0;
    }
    for (size_t i = 0; i < n; i++) {
        const ItxRaw r = {0, pos[i], tmpend[i], mapq[i], flag5[i]};
        int32_t qs, qe;
        bool q, u;
        derive_one(P, s_lut, r, isize[i], mpos[i], tile_pe != 0, (uint32_t)chrom[i], (uint32_t)size[i], true, lut[i], start[i], end[i], qs, qe, q, u);
        uq[i] = u;
    }
}
