// itx_bigwig.hip — the blocks of the two bigWig files of `iteres stat`, built in HBM from the engine's coverage.
//
// host/bigwig.c lays a file down around three kinds of content (bw_dense.c says which); this builds all of it on the device:
//   sections     a 24-byte header and (float)(double)cov[i] for up to 1024 bases (cmd_stat.c's conversion, bw_dense.c's
//                section writer), one wave per section, assembled straight into LDS and deflated there (itx_deflate_core.h)
//   summaries    every zoom level with the arithmetic of bw_sum.c reduce_sections / reduce_summaries (itx_bwfold.h is the step): one
//                lane per output summary, the same sequential fold (double operations, a float store after each step).
//                Every chromosome is covered base by base from 0, so the summaries of a level tile it in steps of the
//                reduction, and each one of level k takes whole summaries of level k - 1 (the reductions are power-of-4
//                multiples of each other): f = overlap / item size is exactly 1.0 everywhere.
//   zoom blocks  1024 summaries of 32 bytes, one wave per block, deflated like the sections
// Then the compressed blocks are packed one after the other, and the host copies back only them and the summaries.
#include "itx_bwblock.h"
#include "itx_bwfold.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

struct BwDev {
    uint32_t n_chrom;
    const uint32_t *cov;
    const uint64_t *cov_off;             // [n_chrom]
    const uint32_t *size;                // [n_chrom]
    const uint64_t *sec_first;           // [n_chrom + 1]
    const uint64_t *sum_first[kBwMaxLevels];   // [n_chrom + 1] per level, index into that level's summaries
    itx_bw_summary *sum[kBwMaxLevels];
    uint32_t reduction[kBwMaxLevels];
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

// zoom level 0 from the bases (bw_sum.c reduce_sections): every base is an item of its own, f = 1.0
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
    itx_bw_summary a = {c, start, end, 0, 0, 0, 0, 0};
    itx_bwfold_open(&a, v0, v0);
    for (uint32_t p = start; p < end; p++) {
        const double val = (double)(float)(double)cov[p];
        itx_bwfold_add(&a, 1.0, 1.0, val, val, val, val * val);
    }
    d.sum[0][i] = a;
}

// zoom level k from level k - 1 (bw_sum.c reduce_summaries): a summary takes whole summaries of the level below, f = 1.0
__global__ void k_bw_levelk(BwDev d, uint32_t k)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t *first = d.sum_first[k], *pfirst = d.sum_first[k - 1];
    if (i >= first[d.n_chrom]) return;
    const uint32_t c = find_chrom(first, d.n_chrom, i), r = d.reduction[k], size = d.size[c];
    const uint32_t q = r / d.reduction[k - 1];
    const uint32_t start = (uint32_t)(i - first[c]) * r;
    const uint32_t end = size - start < r ? size : start + r;
    const uint64_t lo = pfirst[c] + (i - first[c]) * q, e0 = lo + q;
    const uint64_t e = e0 < pfirst[c + 1] ? e0 : pfirst[c + 1];
    const itx_bw_summary *in = d.sum[k - 1];
    itx_bw_summary a = {c, start, end, 0, 0, 0, 0, 0};
    itx_bwfold_open(&a, (double)in[lo].min_val, (double)in[lo].max_val);
    for (uint64_t j = lo; j < e; j++) {
        const itx_bw_summary t = in[j];
        itx_bwfold_add(&a, 1.0, (double)t.valid_count, (double)t.min_val, (double)t.max_val, (double)t.sum_data, (double)t.sum_squares);
    }
    d.sum[k][i] = a;
}

}  // namespace

struct itx_bigwig {
    int device;
    hipStream_t st;
    hipEvent_t ev0, ev1;
    ItxBuf d_plan, d_sum;                // the per-chromosome arrays; every level's summaries
    BwPack pack;
};

static void bw_free(itx_bigwig *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->st) (void)hipStreamSynchronize(b->st);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->st) (void)hipStreamDestroy(b->st);
    delete b;                            // (frees the device buffers)
}

static int bw_start(itx_bigwig *b, itx_engine *e, int uniq, const uint64_t *cov_off, const uint32_t *len, uint32_t n_chrom,
                    const uint32_t *reduction, uint32_t n_levels)
{
    static const char who[] = "itx_bigwig_start";
    int rc;
    const uint32_t *cov;
    uint64_t cov_len;
    if ((rc = itxe_cov_device(e, uniq, &cov, &cov_len, &b->device)) != ITX_OK) return rc;
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
    // per-chromosome tables: sections, then the summaries of each level; and every section's payload
    const size_t nc1 = (size_t)n_chrom + 1;
    std::vector<uint64_t> h(n_chrom + nc1 * (1 + n_levels));
    std::vector<uint32_t> hsize(len, len + n_chrom), payload;
    memcpy(h.data(), cov_off, sizeof(uint64_t) * n_chrom);
    uint64_t *sec_first = h.data() + n_chrom, n_sum[kBwMaxLevels];
    sec_first[0] = 0;
    for (uint32_t c = 0; c < n_chrom; c++) {
        sec_first[c + 1] = sec_first[c] + (len[c] + kItems - 1) / kItems;
        for (uint32_t s = 0; s < len[c]; s += kItems) payload.push_back(24 + 4 * (len[c] - s < kItems ? len[c] - s : kItems));
    }
    for (uint32_t k = 0; k < n_levels; k++) {
        uint64_t *f = sec_first + nc1 * (1 + k);
        f[0] = 0;
        for (uint32_t c = 0; c < n_chrom; c++) f[c + 1] = f[c] + (len[c] + (uint64_t)reduction[k] - 1) / reduction[k];
        n_sum[k] = f[n_chrom];
    }
    ITX_HIP(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
    ITX_HIP(hipEventCreate(&b->ev0));
    ITX_HIP(hipEventCreate(&b->ev1));
    BwPack &P = b->pack;
    if ((rc = bw_pack_layout(P, who, b->st, payload.data(), sec_first[n_chrom], n_levels, n_sum)) != ITX_OK) return rc;
    if ((rc = itx_buf_need(who, b->d_plan, sizeof(uint64_t) * h.size() + sizeof(uint32_t) * (n_chrom + 2))) != ITX_OK) return rc;
    if ((rc = itx_buf_need(who, b->d_sum, sizeof(itx_bw_summary) * (P.sum_base[n_levels] + 1))) != ITX_OK) return rc;
    uint64_t *d_h = b->d_plan.as<uint64_t>();
    uint32_t *d_size = (uint32_t *)(d_h + h.size());
    ITX_HIP(hipMemcpyAsync(d_h, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(d_size, hsize.data(), sizeof(uint32_t) * n_chrom, hipMemcpyHostToDevice, b->st));
    BwDev d;
    memset(&d, 0, sizeof d);
    d.n_chrom = n_chrom;
    d.cov = cov;
    d.cov_off = d_h;
    d.size = d_size;
    d.sec_first = d_h + n_chrom;
    for (uint32_t k = 0; k < n_levels; k++) {
        d.sum_first[k] = d_h + n_chrom + nc1 * (1 + k);
        P.L.sum[k] = d.sum[k] = b->d_sum.as<itx_bw_summary>() + P.sum_base[k];
        d.reduction[k] = reduction[k];
    }
    d.out_off = P.out_off.as<uint64_t>();
    d.out = P.out.as<uint8_t>();
    d.csize = P.csize.as<uint32_t>();
    ITX_HIP(hipEventRecord(b->ev0, b->st));
    if (sec_first[n_chrom]) k_bw_sections<<<dim3((uint32_t)sec_first[n_chrom]), dim3(64), 0, b->st>>>(d);
    for (uint32_t k = 0; k < n_levels; k++) {
        const uint32_t grid = (uint32_t)((n_sum[k] + 255) / 256);
        if (!grid) continue;
        if (k == 0) k_bw_level0<<<dim3(grid), dim3(256), 0, b->st>>>(d);
        else k_bw_levelk<<<dim3(grid), dim3(256), 0, b->st>>>(d, k);
    }
    if ((rc = bw_pack_run(P, b->st)) != ITX_OK) return rc;
    ITX_HIP(hipEventRecord(b->ev1, b->st));
    return ITX_OK;
}

extern "C" int itx_bigwig_start(itx_engine *e, int uniq, const uint64_t *cov_off, const uint32_t *len, uint32_t n_chrom,
                                const uint32_t *reduction, uint32_t n_levels, itx_bigwig **out)
{
    if (!e || !out || (n_chrom && (!cov_off || !len)) || n_levels > kBwMaxLevels || (n_levels && !reduction)) {
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
    int rc = bw_pack_collect(b->pack, "itx_bigwig_collect", b->st);     // (waits for the stream)
    if (rc != ITX_OK) return rc;
    float ms = 0;
    ITX_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    memset(out, 0, sizeof *out);
    bw_pack_result(b->pack, out);
    out->device_ms = ms;
    return ITX_OK;
}

extern "C" void itx_bigwig_destroy(itx_bigwig *b) { bw_free(b); }
