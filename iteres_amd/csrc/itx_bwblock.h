// itx_bwblock.h — device only: what the two bigWig builders (itx_bigwig.hip: dense data from the engine's coverage;
// itx_gcovbw.hip: sparse data from the genome coverage) share. A block is a section's payload or 1024 zoom summaries, assembled
// in LDS by one wave and deflated there (itx_deflate_core.h); the compressed blocks are then packed one after the other.
#pragma once
#include "itx_device.h"

#define ITXD_FN __device__ static inline
#define ITXD_SYNC() __syncthreads()
#define ITXD_AMAX(p, v) atomicMax((p), (v))
#define ITXD_CTZ(x) ((uint32_t)__builtin_ctz(x))
#include "itx_deflate_core.h"

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

// LDS of one block's encoder, sized for inputs of up to MAXN bytes
template <uint32_t MAXN>
struct BwLds {
    uint32_t in[MAXN / 4 + 4];
    uint32_t head[1u << ITXD_HBITS];
    uint16_t md[MAXN];
    uint8_t ml[MAXN];
    uint32_t fq[ITXD_NSYM], key[ITXD_NSYM];
    uint16_t srt[ITXD_NSYM], code[ITXD_NSYM];
    uint8_t len[ITXD_NSYM];
    uint32_t clfq[20];
    uint16_t clcode[20];
    uint8_t cllen[20];
    uint64_t red[128];
    uint32_t misc[16];
};

template <uint32_t MAXN>
__device__ static inline itxd_ws ws_of(BwLds<MAXN> &s)
{
    return itxd_ws{s.in, s.head, s.ml, s.md, s.fq, s.key, s.srt, s.len, s.code, s.clfq, s.cllen, s.clcode, s.red, s.misc};
}

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

// exclusive prefix sum of the compressed sizes: poff[0..n] (one workgroup, itx_device.h)
static __global__ __launch_bounds__(ITX_SCAN_WG) void k_bw_scan(const uint32_t *csize, uint64_t n, uint64_t *poff)
{
    __shared__ uint64_t s[ITX_SCAN_WG];
    uint64_t lo, hi;
    itx_scan_chunk(n, &lo, &hi);
    uint64_t a = 0, total;
    for (uint64_t i = lo; i < hi; i++) a += csize[i];
    uint64_t e = itx_scan_wg(a, s, &total);
    for (uint64_t i = lo; i < hi; i++) {
        poff[i] = e;
        e += csize[i];
    }
    if (threadIdx.x == 0) poff[n] = total;
}

static __global__ __launch_bounds__(256) void k_bw_gather(const uint8_t *out, const uint64_t *out_off, const uint32_t *csize, const uint64_t *poff,
                                                          uint8_t *packed)
{
    const uint64_t b = blockIdx.x;
    const uint8_t *src = out + out_off[b];
    uint8_t *dst = packed + poff[b];
    for (uint32_t i = threadIdx.x; i < csize[b]; i += 256) dst[i] = src[i];
}
