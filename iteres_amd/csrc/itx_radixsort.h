// itx_radixsort.h — the stable LSD radix sort of (key, payload) pairs, 8 bits a pass between two buffers of 8 bytes per
// entry (the read lists of itx_names.hip sort (row, entry) by row; the .loci order of itx_loci.hip sorts (chrom rank | bin, row)).
// One pass over n pairs, nwg = ceil(n / SORT_CHUNK) workgroups, hist: 256 * nwg words:
//   k_sort_hist     per-workgroup digit counts, stored digit-major
//   k_sort_scan     one workgroup, exclusive scan in place: digit-major so that the scan IS the global order
//   k_sort_scatter  ranks inside a wave by ballot match: equal digits keep their order, so the sort is stable
// The key is .x, the payload .y; n < 2^32. The host runs the passes with itx_sort_run (below), the one place that launches the three.
#pragma once
#include "itx_device.h"

#define SORT_CHUNK 8192u             // keys per workgroup and pass

static __global__ __launch_bounds__(256) void k_sort_hist(const uint2 *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t *__restrict__ hist, uint32_t nwg)
{
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * SORT_CHUNK;
    for (uint32_t k = threadIdx.x; k < SORT_CHUNK && base + k < n; k += 256u) atomicAdd(&s_h[(keys[base + k].x >> shift) & 255u], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * nwg + blockIdx.x] = s_h[threadIdx.x];
}

// exclusive scan in place, one workgroup; digit-major counts: the scanned value is where (digit, workgroup) starts
static __global__ __launch_bounds__(ITX_SCAN_WG) void k_sort_scan(uint32_t *__restrict__ v, uint32_t n)
{
    __shared__ uint32_t s[ITX_SCAN_WG];
    uint64_t lo, hi;
    itx_scan_chunk(n, &lo, &hi);
    uint32_t a = 0, total;
    for (uint64_t k = lo; k < hi; k++) a += v[k];
    uint32_t e = itx_scan_wg(a, s, &total);
    for (uint64_t k = lo; k < hi; k++) {
        const uint32_t c = v[k];
        v[k] = e;
        e += c;
    }
}

static __global__ __launch_bounds__(256) void k_sort_scatter(const uint2 *__restrict__ in, uint2 *__restrict__ out, uint32_t n, uint32_t shift, const uint32_t *__restrict__ hist,
                                                       uint32_t nwg)
{
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wc[4][256];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    s_base[t] = hist[(size_t)t * nwg + blockIdx.x];
    for (uint32_t k = 0; k < 4u; k++) s_wc[k][t] = 0;
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * SORT_CHUNK;
    for (uint32_t r = 0; r < SORT_CHUNK && base + r < n; r += 256u) {
        const unsigned long long j = base + r + t;
        const bool valid = j < n;
        const uint2 key = valid ? in[j] : make_uint2(0u, 0u);
        const uint32_t d = (key.x >> shift) & 255u;
        unsigned long long m = __ballot(valid);                                        // the lanes of this wave with the same digit
        for (uint32_t bit = 0; bit < 8u; bit++) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bm = __ballot(one);
            m &= one ? bm : ~bm;
        }
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_wc[w][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (valid) {
            uint32_t off = s_base[d] + rank;
            for (uint32_t k = 0; k < w; k++) off += s_wc[k][d];
            out[off] = key;
        }
        __syncthreads();
        uint32_t sum = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            sum += s_wc[k][t];
            s_wc[k][t] = 0;
        }
        s_base[t] += sum;
        __syncthreads();
    }
}

// ---- host: the three kernels run as one
// bytes of the digit counts (hist) of a sort of n pairs
static inline size_t itx_sort_hist_bytes(uint64_t n) { return 4 * 256 * (size_t)((n + SORT_CHUNK - 1) / SORT_CHUNK); }

// `passes` passes over the n pairs of `from`, by the digits at first_shift, first_shift + 8, ..., enqueued on st; the pairs go to and
// fro between `from` and `other`, *sorted is the one that holds them in the end.
static inline int itx_sort_run(hipStream_t st, uint2 *from, uint2 *other, uint32_t n, uint32_t first_shift, uint32_t passes, uint32_t *hist, uint2 **sorted)
{
    int rc = ITX_OK;
    const uint32_t nwg = (uint32_t)(((uint64_t)n + SORT_CHUNK - 1) / SORT_CHUNK);
    *sorted = from;
    for (uint32_t p = 0; p < passes; p++) {
        uint2 *to = *sorted == from ? other : from;
        hipLaunchKernelGGL(k_sort_hist, dim3(nwg), dim3(256), 0, st, *sorted, n, first_shift + 8u * p, hist, nwg);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(ITX_SCAN_WG), 0, st, hist, 256u * nwg);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sort_scatter, dim3(nwg), dim3(256), 0, st, *sorted, to, n, first_shift + 8u * p, hist, nwg);
        ITX_TRY(hipGetLastError());
        *sorted = to;
    }
out:
    return rc;
}
