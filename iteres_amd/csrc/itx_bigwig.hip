// itx_bigwig.hip — the blocks of the two bigWig files of `iteres stat`, built in HBM from the engine's coverage.
//
// host/bigwig.c lays a file down around three kinds of content; this builds all of it on the device:
//   sections     a 24-byte header and (float)(double)cov[i] for up to 1024 bases (cmd_stat.c's conversion, bigwig.c's
//                section writer), one wave per section, assembled straight into LDS and deflated there (itx_deflate_core.h)
//   summaries    every zoom level with the arithmetic of bigwig.c reduce_sections / reduce_summaries / add_to_summary: one
//                lane per output summary, the same sequential fold (double operations, a float store after each step).
//                Every chromosome is covered base by base from 0, so the summaries of a level tile it in steps of the
//                reduction, and each one of level k takes whole summaries of level k - 1 (the reductions are power-of-4
//                multiples of each other): f = overlap / item size is exactly 1.0 everywhere.
//   zoom blocks  1024 summaries of 32 bytes, one wave per block, deflated like the sections
// Then the compressed blocks are packed one after the other, and the host copies back only them and the summaries.
#include "itx_bwblock.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxLevels = 10;

struct BwDev {
    uint32_t n_chrom, n_levels;
    uint64_t n_sec, n_blocks;
    const uint32_t *cov;
    const uint64_t *cov_off;             // [n_chrom]
    const uint32_t *size;                // [n_chrom]
    const uint64_t *sec_first;           // [n_chrom + 1]
    const uint64_t *sum_first[kMaxLevels];   // [n_chrom + 1] per level, index into that level's summaries
    itx_bw_summary *sum[kMaxLevels];
    uint32_t reduction[kMaxLevels];
    uint64_t slot_first[kMaxLevels + 1]; // block index of each level's first zoom block (and the end)
    const uint64_t *out_off;             // [n_blocks]
    uint8_t *out;
    uint32_t *csize;                     // [n_blocks]
};

constexpr uint32_t kSecMax = 24 + 4 * kItems;

// one wave per data section: header + floats into LDS, deflated
__global__ __launch_bounds__(64) void k_bw_sections(BwDev d)
{
    __shared__ BwLds<kSecMax> s;
    const uint64_t b = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t c = find_chrom(d.sec_first, d.n_chrom, b);
    const uint32_t start = (uint32_t)(b - d.sec_first[c]) * kItems, size = d.size[c];
    const uint32_t cnt = size - start < kItems ? size - start : kItems;
    const uint32_t n = 24 + 4 * cnt, words = n / 4;
    const uint32_t *cov = d.cov + d.cov_off[c] + start;
    for (uint32_t i = lane; i < kSecMax / 4 + 4; i += 64) {
        uint32_t v = 0;
        if (i == 0) v = c;
        else if (i == 1) v = start;
        else if (i == 2) v = start + cnt;
        else if (i == 3 || i == 4) v = 1;                             // step, span
        else if (i == 5) v = 3u | cnt << 16;                          // bwgTypeFixedStep, reserved, item count
        else if (i < words) v = __float_as_uint((float)(double)cov[i - 6]);
        s.in[i] = v;
    }
    __syncthreads();
    const uint32_t z = itxd_deflate(ws_of(s), n, d.out + d.out_off[b], lane, 64);
    if (lane == 0) d.csize[b] = z;
}

// one wave per zoom block: 1024 summaries of one level
__global__ __launch_bounds__(64) void k_bw_zoom(BwDev d)
{
    __shared__ BwLds<kZoomMax> s;
    const uint64_t b = d.n_sec + blockIdx.x;
    uint32_t k = 0;
    while (k + 1 < d.n_levels && d.slot_first[k + 1] <= b) k++;
    const uint64_t n_sum = d.sum_first[k][d.n_chrom];
    const uint64_t first = (b - d.slot_first[k]) * kItems;
    const uint32_t cnt = n_sum - first < kItems ? (uint32_t)(n_sum - first) : kItems;
    bw_zoom_block(s, d.sum[k] + first, cnt, d.out + d.out_off[b], &d.csize[b]);
}

// zoom level 0 from the bases: bigwig.c reduce_sections
__global__ void k_bw_level0(BwDev d)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t *first = d.sum_first[0];
    if (i >= first[d.n_chrom]) return;
    const uint32_t c = find_chrom(first, d.n_chrom, i), r = d.reduction[0], size = d.size[c];
    const uint32_t start = (uint32_t)(i - first[c]) * r;
    const uint32_t end = size - start < r ? size : start + r;
    const uint32_t *cov = d.cov + d.cov_off[c];
    const double v0 = (double)(float)(double)cov[start];
    uint32_t vc = 0;
    float mn = (float)v0, mx = (float)v0, sd = 0.0f, sq = 0.0f;
    for (uint32_t p = start; p < end; p++) {
        const double val = (double)(float)(double)cov[p];
        vc = (uint32_t)((double)vc + 1.0);
        if (mn > val) mn = (float)val;
        if (mx < val) mx = (float)val;
        sd = (float)((double)sd + val);
        sq = (float)((double)sq + val * val);
    }
    d.sum[0][i] = itx_bw_summary{c, start, end, vc, mn, mx, sd, sq};
}

// zoom level k from level k - 1: bigwig.c reduce_summaries (add_to_summary with f = 1.0)
__global__ void k_bw_levelk(BwDev d, uint32_t k)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t *first = d.sum_first[k], *pfirst = d.sum_first[k - 1];
    if (i >= first[d.n_chrom]) return;
    const uint32_t c = find_chrom(first, d.n_chrom, i), r = d.reduction[k], size = d.size[c];
    const uint32_t q = r / d.reduction[k - 1];
    const uint32_t start = (uint32_t)(i - first[c]) * r;
    const uint32_t end = size - start < r ? size : start + r;
    const uint64_t a = pfirst[c] + (i - first[c]) * q, e0 = a + q;
    const uint64_t e = e0 < pfirst[c + 1] ? e0 : pfirst[c + 1];
    const itx_bw_summary *in = d.sum[k - 1];
    uint32_t vc = 0;
    float mn = in[a].min_val, mx = in[a].max_val, sd = 0.0f, sq = 0.0f;
    const double f = 1.0;
    for (uint64_t j = a; j < e; j++) {
        const itx_bw_summary t = in[j];
        vc = (uint32_t)((double)vc + f * (double)t.valid_count);
        if ((double)mn > (double)t.min_val) mn = t.min_val;
        if ((double)mx < (double)t.max_val) mx = t.max_val;
        sd = (float)((double)sd + f * (double)t.sum_data);
        sq = (float)((double)sq + f * (double)t.sum_squares);
    }
    d.sum[k][i] = itx_bw_summary{c, start, end, vc, mn, mx, sd, sq};
}

}  // namespace

struct itx_bigwig {
    int device;
    hipStream_t st;
    hipEvent_t ev0, ev1;
    uint32_t n_levels;
    uint64_t n_sec, n_blocks, n_sum[kMaxLevels], slot_first[kMaxLevels + 1], sum_base[kMaxLevels + 1];
    void *d_plan;                        // the per-chromosome arrays
    itx_bw_summary *d_sum;
    uint8_t *d_out, *d_packed;
    uint64_t *d_out_off, *d_poff;
    uint32_t *d_csize;
    std::vector<uint64_t> poff;
    std::vector<uint8_t> packed;
    std::vector<itx_bw_summary> sums;
};

static void bw_free(itx_bigwig *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->st) (void)hipStreamSynchronize(b->st);
    void *bufs[] = {b->d_plan, b->d_sum, b->d_out, b->d_packed, b->d_out_off, b->d_poff, b->d_csize};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->st) (void)hipStreamDestroy(b->st);
    delete b;
}

static int bw_start(itx_bigwig *b, itx_engine *e, int uniq, const uint64_t *cov_off, const uint32_t *len, uint32_t n_chrom,
                    const uint32_t *reduction, uint32_t n_levels)
{
    const uint32_t *cov;
    uint64_t cov_len;
    int rc = itxe_cov_device(e, uniq, &cov, &cov_len, &b->device);
    if (rc) return rc;
    ITX_HIP(hipSetDevice(b->device));
    for (uint32_t c = 0; c < n_chrom; c++)
        if (!len[c] || cov_off[c] > cov_len || len[c] > cov_len - cov_off[c]) {     // (no sum of the two: it could wrap)
            itx_set_error("itx_bigwig_start: chromosome %u (offset %llu, length %u) is empty or outside the coverage", c,
                          (unsigned long long)cov_off[c], len[c]);
            return ITX_E_ARG;
        }
    if (n_levels && (!reduction[0] || reduction[0] >= 1u << 31)) {
        itx_set_error("itx_bigwig_start: reduction %u is outside 1 .. 2^31 - 1", reduction[0]);
        return ITX_E_ARG;
    }
    for (uint32_t k = 1; k < n_levels; k++) {
        const uint32_t q = reduction[k] / reduction[k - 1];                // 4, 16, 64, ...: one bit, at an even place
        if (reduction[k] % reduction[k - 1] || q < 4 || (q & (q - 1)) || (__builtin_ctz(q) & 1) || reduction[k] >= 1u << 31) {
            itx_set_error("itx_bigwig_start: reduction %u is no power-of-4 multiple of %u below 2^31", reduction[k], reduction[k - 1]);
            return ITX_E_ARG;
        }
    }
    // per-chromosome tables: sections, then the summaries of each level
    const size_t nc1 = (size_t)n_chrom + 1;
    std::vector<uint64_t> h(n_chrom + nc1 * (1 + n_levels));
    std::vector<uint32_t> hsize(len, len + n_chrom);
    memcpy(h.data(), cov_off, sizeof(uint64_t) * n_chrom);
    uint64_t *sec_first = h.data() + n_chrom;
    sec_first[0] = 0;
    for (uint32_t c = 0; c < n_chrom; c++) sec_first[c + 1] = sec_first[c] + (len[c] + kItems - 1) / kItems;
    b->n_sec = sec_first[n_chrom];
    b->n_levels = n_levels;
    b->sum_base[0] = 0;
    b->slot_first[0] = b->n_sec;
    for (uint32_t k = 0; k < n_levels; k++) {
        uint64_t *f = sec_first + nc1 * (1 + k);
        f[0] = 0;
        for (uint32_t c = 0; c < n_chrom; c++) f[c + 1] = f[c] + (len[c] + (uint64_t)reduction[k] - 1) / reduction[k];
        b->n_sum[k] = f[n_chrom];
        b->sum_base[k + 1] = b->sum_base[k] + b->n_sum[k];
        b->slot_first[k + 1] = b->slot_first[k] + (b->n_sum[k] + kItems - 1) / kItems;
    }
    b->n_blocks = b->slot_first[n_levels];
    // where each block's zlib stream is made (room for a stored block), then packed
    std::vector<uint64_t> out_off(b->n_blocks + 1);
    uint64_t at = 0;
    for (uint32_t c = 0; c < n_chrom; c++)
        for (uint32_t s = 0; s < len[c]; s += kItems) {
            out_off[sec_first[c] + s / kItems] = at;
            at += ITXD_OUT_CAP(24 + 4 * (len[c] - s < kItems ? len[c] - s : kItems));
        }
    for (uint32_t k = 0; k < n_levels; k++)
        for (uint64_t j = 0; j < b->n_sum[k]; j += kItems) {
            out_off[b->slot_first[k] + j / kItems] = at;
            at += ITXD_OUT_CAP(32 * (b->n_sum[k] - j < kItems ? b->n_sum[k] - j : kItems));
        }
    out_off[b->n_blocks] = at;

    ITX_HIP(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
    ITX_HIP(hipEventCreate(&b->ev0));
    ITX_HIP(hipEventCreate(&b->ev1));
    const size_t plan_bytes = sizeof(uint64_t) * h.size() + sizeof(uint32_t) * (n_chrom + 2);
    ITX_HIP(hipMalloc(&b->d_plan, plan_bytes));
    ITX_HIP(hipMalloc((void **)&b->d_sum, sizeof(itx_bw_summary) * (b->sum_base[n_levels] + 1)));
    ITX_HIP(hipMalloc((void **)&b->d_out, at + 16));
    ITX_HIP(hipMalloc((void **)&b->d_packed, at + 16));
    ITX_HIP(hipMalloc((void **)&b->d_out_off, sizeof(uint64_t) * (b->n_blocks + 1)));
    ITX_HIP(hipMalloc((void **)&b->d_poff, sizeof(uint64_t) * (b->n_blocks + 1)));
    ITX_HIP(hipMalloc((void **)&b->d_csize, sizeof(uint32_t) * (b->n_blocks + 1)));
    uint64_t *d_h = (uint64_t *)b->d_plan;
    uint32_t *d_size = (uint32_t *)(d_h + h.size());
    ITX_HIP(hipMemcpyAsync(d_h, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(d_size, hsize.data(), sizeof(uint32_t) * n_chrom, hipMemcpyHostToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(b->d_out_off, out_off.data(), sizeof(uint64_t) * (b->n_blocks + 1), hipMemcpyHostToDevice, b->st));

    BwDev d;
    memset(&d, 0, sizeof d);
    d.n_chrom = n_chrom;
    d.n_levels = n_levels;
    d.n_sec = b->n_sec;
    d.n_blocks = b->n_blocks;
    d.cov = cov;
    d.cov_off = d_h;
    d.size = d_size;
    d.sec_first = d_h + n_chrom;
    for (uint32_t k = 0; k < n_levels; k++) {
        d.sum_first[k] = d_h + n_chrom + nc1 * (1 + k);
        d.sum[k] = b->d_sum + b->sum_base[k];
        d.reduction[k] = reduction[k];
    }
    memcpy(d.slot_first, b->slot_first, sizeof d.slot_first);
    d.out_off = b->d_out_off;
    d.out = b->d_out;
    d.csize = b->d_csize;
    ITX_HIP(hipEventRecord(b->ev0, b->st));
    if (b->n_sec) k_bw_sections<<<dim3((uint32_t)b->n_sec), dim3(64), 0, b->st>>>(d);
    for (uint32_t k = 0; k < n_levels; k++) {
        const uint32_t grid = (uint32_t)((b->n_sum[k] + 255) / 256);
        if (!grid) continue;
        if (k == 0) k_bw_level0<<<dim3(grid), dim3(256), 0, b->st>>>(d);
        else k_bw_levelk<<<dim3(grid), dim3(256), 0, b->st>>>(d, k);
    }
    if (b->n_blocks > b->n_sec) k_bw_zoom<<<dim3((uint32_t)(b->n_blocks - b->n_sec)), dim3(64), 0, b->st>>>(d);
    if (b->n_blocks) {
        k_size_scan<<<dim3(1), dim3(ITX_SCAN_WG), 0, b->st>>>(b->d_csize, b->n_blocks, b->d_poff);
        k_pack_blocks<<<dim3((uint32_t)b->n_blocks), dim3(256), 0, b->st>>>(b->d_out, b->d_out_off, 0u, b->d_csize, b->d_poff, b->d_packed);
    }
    ITX_HIP(hipGetLastError());
    ITX_HIP(hipEventRecord(b->ev1, b->st));
    return ITX_OK;
}

extern "C" int itx_bigwig_start(itx_engine *e, int uniq, const uint64_t *cov_off, const uint32_t *len, uint32_t n_chrom,
                                const uint32_t *reduction, uint32_t n_levels, itx_bigwig **out)
{
    if (!e || !out || (n_chrom && (!cov_off || !len)) || n_levels > kMaxLevels || (n_levels && !reduction)) {
        itx_set_error("itx_bigwig_start: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    itx_bigwig *b = new (std::nothrow) itx_bigwig();
    if (!b) return ITX_E_NOMEM;
    const int rc = bw_start(b, e, uniq, cov_off, len, n_chrom, reduction, n_levels);
    if (rc) {
        bw_free(b);
        return rc;
    }
    *out = b;
    return ITX_OK;
}

extern "C" int itx_bigwig_collect(itx_bigwig *b, itx_bw_result *out)
{
    if (!b || !out) {
        itx_set_error("itx_bigwig_collect: bad argument");
        return ITX_E_ARG;
    }
    ITX_HIP(hipSetDevice(b->device));
    ITX_HIP(hipStreamSynchronize(b->st));
    float ms = 0;
    ITX_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    b->poff.assign(b->n_blocks + 1, 0);
    if (b->n_blocks) ITX_HIP(hipMemcpy(b->poff.data(), b->d_poff, sizeof(uint64_t) * (b->n_blocks + 1), hipMemcpyDeviceToHost));
    b->packed.resize(b->poff[b->n_blocks] + 1);
    if (b->poff[b->n_blocks]) ITX_HIP(hipMemcpy(b->packed.data(), b->d_packed, b->poff[b->n_blocks], hipMemcpyDeviceToHost));
    b->sums.resize(b->sum_base[b->n_levels] + 1);
    if (b->sum_base[b->n_levels])
        ITX_HIP(hipMemcpy(b->sums.data(), b->d_sum, sizeof(itx_bw_summary) * b->sum_base[b->n_levels], hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->n_sec = b->n_sec;
    out->n_blocks = b->n_blocks;
    out->n_levels = b->n_levels;
    for (uint32_t k = 0; k < b->n_levels; k++) {
        out->n_sum[k] = b->n_sum[k];
        out->slot_first[k] = b->slot_first[k];
        out->sum[k] = b->sums.data() + b->sum_base[k];
    }
    out->block_off = b->poff.data();
    out->blocks = b->packed.data();
    out->device_ms = ms;
    return ITX_OK;
}

extern "C" void itx_bigwig_destroy(itx_bigwig *b) { bw_free(b); }
