// itx_bwfold.h — one step of the fold that makes a bigWig zoom summary (cuskent/bbiWrite.c:370-421 bbiAddToSummary), stated once for
// the host (host/bw_sum.c) and the device (k_bw_level0, k_bw_levelk of csrc/itx_bigwig.hip; k_ch_fold of csrc/itx_gcovbw.hip). The
// five updates are double operations with a float (or u32) store after each, in this order, and a product is never fused into the
// sum that takes it. A site keeps what differs: where the items come from, and what f is (overlap / what is left of the item; 1.0
// where items never straddle a boundary: x * 1.0 is exact). The accumulator is the record; chrom_id, start and end are the site's.
// Contraction is off in here for the device and for clang. gcc has no pragma for one function: the host program is built for
// baseline x86-64, which has no fused multiply-add, and a gcc target that has one is refused below.
#ifndef ITX_BWFOLD_H
#define ITX_BWFOLD_H
#include "../../include/iteres_amd.h"

#ifdef __HIPCC__
#define ITX_BWFOLD_FN static __host__ __device__ inline
#else
#define ITX_BWFOLD_FN static inline
#endif
#ifdef __clang__
#define ITX_BWFOLD_NO_FMA _Pragma("clang fp contract(off)")
#else
#define ITX_BWFOLD_NO_FMA
#if defined(__FP_FAST_FMA) && !defined(ITX_BWFOLD_CONTRACT_OFF)
#error "itx_bwfold.h: this target fuses multiply-add: build with -ffp-contract=off -DITX_BWFOLD_CONTRACT_OFF"
#endif
#endif

/* a new summary: it starts from the extremes of the item that opens it, which is then added like every other */
ITX_BWFOLD_FN void itx_bwfold_open(itx_bw_summary *a, double min_val, double max_val)
{
    a->valid_count = 0;
    a->min_val = (float)min_val;
    a->max_val = (float)max_val;
    a->sum_data = a->sum_squares = 0.0f;
}

ITX_BWFOLD_FN void itx_bwfold_add(itx_bw_summary *a, double f, double valid_count, double min_val, double max_val, double sum_data, double sum_squares)
{
    ITX_BWFOLD_NO_FMA
    a->valid_count = (uint32_t)(a->valid_count + f * valid_count);
    if (a->min_val > min_val) a->min_val = (float)min_val;
    if (a->max_val < max_val) a->max_val = (float)max_val;
    a->sum_data = (float)(a->sum_data + f * sum_data);
    a->sum_squares = (float)(a->sum_squares + f * sum_squares);
}

#endif
