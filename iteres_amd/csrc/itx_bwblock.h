// itx_bwblock.h — device only: what the two bigWig builders (itx_bigwig.hip: dense data from the engine's coverage;
// itx_gcovbw.hip: sparse data from the genome coverage) share. A block is a section's payload or 1024 zoom summaries, assembled
// in LDS by one wave and deflated there (itx_deflate_device.h); the compressed blocks are then packed one after the other
// (k_size_scan / k_pack_blocks, itx_textpack.h).
#pragma once
#include "itx_deflate_device.h"
#include "itx_textpack.h"

constexpr uint32_t kItems = 1024;        // items per slot (stat.c:157-158)
constexpr uint32_t kZoomMax = 32 * kItems;

// last c with first[c] <= i
__device__ static inline uint32_t find_chrom(const uint64_t *first, uint32_t n, uint64_t i)
{
    uint32_t lo = 0, hi = n;                     // first[lo] <= i < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (first[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// LDS of one block's encoder, sized for inputs of up to MAXN bytes (itx_deflate_device.h, which has ws_of)
template <uint32_t MAXN>
using BwLds = ItxdLds<MAXN>;

// one wave, one zoom block: cnt (<= 1024) summaries from sum into LDS, deflated to dst; the compressed size goes to *csize
__device__ static inline void bw_zoom_block(BwLds<kZoomMax> &s, const itx_bw_summary *sum, uint32_t cnt, uint8_t *dst, uint32_t *csize)
{
    const uint32_t lane = threadIdx.x, n = 32 * cnt;
    const uint32_t *src = (const uint32_t *)sum;
    for (uint32_t i = lane; i < kZoomMax / 4 + 4; i += 64) s.in[i] = i < n / 4 ? src[i] : 0u;
    __syncthreads();
    const uint32_t z = itxd_deflate(ws_of(s), n, dst, lane, 64);
    if (lane == 0) *csize = z;
}
