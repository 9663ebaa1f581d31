// itx_bwblock.h — what the two bigWig builders (itx_bigwig.hip: dense data from the engine's coverage; itx_gcovbw.hip: sparse data
// from the genome coverage) share. A block is a section's payload or 1024 zoom summaries, assembled in LDS by one wave and deflated
// there (itx_deflate_device.h). BwPack is a build's blocks: blocks 0 .. n_sec - 1 are the sections (the builder's own kernel deflates
// them to out + out_off[b] and stores csize[b]), then each level's zoom blocks (k_bw_zoom, all levels in one launch); bw_pack_layout
// gives every block the worst case's room, bw_pack_run deflates the zoom blocks and packs all of them (k_size_scan / k_pack_blocks,
// itx_textpack.h), bw_pack_collect brings back the offsets, the packed bytes and the summaries: nothing else crosses the bus.
#pragma once
#include "itx_deflate_device.h"
#include "itx_devbuf.h"
#include "itx_textpack.h"
#include <vector>

constexpr uint32_t kItems = 1024;        // items per slot (stat.c:157-158)
constexpr uint32_t kZoomMax = 32 * kItems;
constexpr uint32_t kBwMaxLevels = 10;

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

// the levels of a build: level k's n_sum[k] summaries lie at sum[k], its zoom blocks are slot_first[k] .. slot_first[k + 1] - 1
struct BwLevels {
    uint32_t n;
    const itx_bw_summary *sum[kBwMaxLevels];
    uint64_t n_sum[kBwMaxLevels], slot_first[kBwMaxLevels + 1];
};

// one wave per zoom block of 1024 summaries, all levels: block slot_first[0] + blockIdx.x belongs to the last level that starts at or before it (a
// level without a summary has no block and is stepped over)
static __global__ __launch_bounds__(64) void k_bw_zoom(BwLevels L, const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out, uint32_t *__restrict__ csize)
{
    __shared__ BwLds<kZoomMax> s;
    const uint64_t b = L.slot_first[0] + blockIdx.x;
    uint32_t k = 0;
    while (k + 1 < L.n && L.slot_first[k + 1] <= b) k++;
    const uint64_t n_sum = L.n_sum[k], first = (b - L.slot_first[k]) * kItems;
    const uint32_t lane = threadIdx.x, n = 32 * (n_sum - first < kItems ? (uint32_t)(n_sum - first) : kItems);
    const uint32_t *src = (const uint32_t *)(L.sum[k] + first);
    for (uint32_t i = lane; i < kZoomMax / 4 + 4; i += 64) s.in[i] = i < n / 4 ? src[i] : 0u;
    __syncthreads();
    const uint32_t z = itxd_deflate(ws_of(s), n, out + out_off[b], lane, 64);
    if (lane == 0) csize[b] = z;
}

struct BwPack {
    BwLevels L = {};                         // (sum[] is the builder's to fill in before bw_pack_run)
    uint64_t room = 0, sum_base[kBwMaxLevels + 1] = {0};
    ItxBuf out, packed, out_off, poff, csize;
    std::vector<uint64_t> h_out_off, h_poff; // h_poff: block i is h_packed[h_poff[i] .. h_poff[i + 1])
    std::vector<uint8_t> h_packed;
    std::vector<itx_bw_summary> h_sums;      // level k from sum_base[k] on
};

// payload[s]: the bytes section s deflates; n_sum[k]: the summaries of level k
static inline int bw_pack_layout(BwPack &P, const char *who, hipStream_t st, const uint32_t *payload, uint64_t n_sec, uint32_t n_levels, const uint64_t *n_sum)
{
    int rc;
    uint64_t at = 0, nb = n_sec;
    P.L.n = n_levels;
    for (uint32_t k = 0; k < n_levels; k++) {
        P.L.n_sum[k] = n_sum[k];
        P.L.slot_first[k] = nb;
        nb += (n_sum[k] + kItems - 1) / kItems;
        P.sum_base[k + 1] = P.sum_base[k] + n_sum[k];
    }
    P.L.slot_first[n_levels] = nb;
    P.h_out_off.resize((size_t)nb + 1);
    for (uint64_t b = 0; b < nb; b++) {
        uint32_t k = 0;
        while (k + 1 < n_levels && P.L.slot_first[k + 1] <= b) k++;
        const uint64_t left = b < n_sec ? 0 : n_sum[k] - (b - P.L.slot_first[k]) * kItems;
        P.h_out_off[(size_t)b] = at;
        at += ITXD_OUT_CAP(b < n_sec ? payload[b] : 32u * (uint32_t)(left < kItems ? left : kItems));
    }
    P.h_out_off[(size_t)nb] = P.room = at;
    if ((rc = itx_buf_need(who, P.out, (size_t)at + 16)) || (rc = itx_buf_need(who, P.packed, (size_t)at + 16)) ||
        (rc = itx_buf_need(who, P.out_off, 8 * ((size_t)nb + 1))) || (rc = itx_buf_need(who, P.poff, 8 * ((size_t)nb + 1))) ||
        (rc = itx_buf_need(who, P.csize, 4 * ((size_t)nb + 1))))
        return rc;
    ITX_HIP(hipMemcpyAsync(P.out_off.p, P.h_out_off.data(), 8 * ((size_t)nb + 1), hipMemcpyHostToDevice, st));
    return ITX_OK;
}

static inline int bw_pack_run(BwPack &P, hipStream_t st)
{
    const uint64_t n_sec = P.L.slot_first[0], nb = P.L.slot_first[P.L.n];
    if (nb > n_sec) hipLaunchKernelGGL(k_bw_zoom, dim3((uint32_t)(nb - n_sec)), dim3(64), 0, st, P.L, P.out_off.as<uint64_t>(), P.out.as<uint8_t>(), P.csize.as<uint32_t>());
    if (nb) {
        hipLaunchKernelGGL(k_size_scan, dim3(1), dim3(ITX_SCAN_WG), 0, st, P.csize.as<uint32_t>(), nb, P.poff.as<uint64_t>());
        hipLaunchKernelGGL(k_pack_blocks, dim3((uint32_t)nb), dim3(256), 0, st, P.out.as<uint8_t>(), P.out_off.as<uint64_t>(), 0u, P.csize.as<uint32_t>(),
                           P.poff.as<uint64_t>(), P.packed.as<uint8_t>());
    }
    ITX_HIP(hipGetLastError());
    return ITX_OK;
}

// waits for the stream
static inline int bw_pack_collect(BwPack &P, const char *who, hipStream_t st)
{
    const size_t nb = (size_t)P.L.slot_first[P.L.n];
    ITX_HIP(hipStreamSynchronize(st));
    P.h_poff.assign(nb + 1, 0);
    if (nb) ITX_HIP(hipMemcpy(P.h_poff.data(), P.poff.p, 8 * (nb + 1), hipMemcpyDeviceToHost));
    if (P.h_poff[nb] > P.room) {
        itx_set_error("%s: %llu packed bytes in room for %llu", who, (unsigned long long)P.h_poff[nb], (unsigned long long)P.room);
        return ITX_E_LIMIT;
    }
    P.h_packed.resize((size_t)P.h_poff[nb] + 1);
    if (P.h_poff[nb]) ITX_HIP(hipMemcpy(P.h_packed.data(), P.packed.p, (size_t)P.h_poff[nb], hipMemcpyDeviceToHost));
    P.h_sums.resize((size_t)P.sum_base[P.L.n] + 1);
    for (uint32_t k = 0; k < P.L.n; k++)
        if (P.L.n_sum[k]) ITX_HIP(hipMemcpy(P.h_sums.data() + P.sum_base[k], P.L.sum[k], 32 * (size_t)P.L.n_sum[k], hipMemcpyDeviceToHost));
    return ITX_OK;
}

// itx_bw_result and itx_gcov_bw_result name these alike
template <class R>
static inline void bw_pack_result(const BwPack &P, R *out)
{
    out->n_sec = P.L.slot_first[0];
    out->n_blocks = P.L.slot_first[P.L.n];
    out->n_levels = P.L.n;
    for (uint32_t k = 0; k < P.L.n; k++) {
        out->n_sum[k] = P.L.n_sum[k];
        out->slot_first[k] = P.L.slot_first[k];
        out->sum[k] = P.h_sums.data() + P.sum_base[k];
    }
    out->block_off = P.h_poff.data();
    out->blocks = P.h_packed.data();
}
