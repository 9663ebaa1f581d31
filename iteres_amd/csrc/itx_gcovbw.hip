// itx_gcovbw.hip — the bigWig content of `iteres filter -W` (an extension): one file of the genome coverage (itx_gcov.hip) as the
// reference's converter would write it from the bedGraph text, built from the change points where they lie.
//
// Sparse data is what itx_bigwig.hip never met: `stat` covers every chromosome base by base from 0, so its summaries tile in fixed
// steps. Here the summaries follow the data (host/bw_sum.c add_to_summary is the rule): the first one of a chromosome starts at
// the first item's start; the open summary [S, E) takes what reaches into it; an item base at or behind E opens the next one,
// at E when that base lies before E + R (R: the reduction), at the base itself otherwise (a new ANCHOR); and an item that a
// boundary cuts gives the fraction overlap / (what is LEFT of the item) to each summary, not overlap / its length.
//
//   items        k_gbw_item_measure / k_tile_scan2 / k_gbw_item_write: point k is an item when its depth is > 0 and point k + 1
//                lies on the same chromosome; compacted as (chromosome, start, end, depth). k_gbw_lower finds every chromosome's
//                first item; the host numbers the chromosomes that have one (the bigWig ids) and k_gbw_remap writes the ids in.
//   sections     1024 items of one chromosome. k_gbw_secstat (a wave per section): key, count, smallest item length (their mean
//                is the resolution the first reduction starts from). k_gbw_sections (a wave per section): header and 12-byte
//                items into LDS, deflated (itx_bwblock.h).
//   the chain    for a reduction R over items that are level-0 items or the summaries of the level below (both start with
//                chromosome, start, end). Between anchors the boundaries are anchor + k R and every cell has data, so all that
//                is sequential is which items anchor. With g the gap to the item before: g >= 2R - 1 always anchors (E is at most
//                R - 1 behind that item's end), g < R never does, and g in [R, 2R - 2] depends on the anchor before it.
//                k_ch_flag_* flag the definite anchors and the ambiguous items and compact both (two columns of one scan);
//                k_ch_walk: one lane per definite anchor walks the ambiguous items up to the next definite anchor, and nothing
//                else; k_ch_anc_*: the anchors numbered (a run = an anchor and the items up to the next one) and every item given
//                its run; k_ch_cell_measure: the cells an item opens, summed: the number of summaries. That is the counting form
//                the first-reduction loop runs (the host drives it: two 8-byte totals cross the bus a try); k_ch_runbase then
//                gives every run its first summary.
//                Worst case: a chromosome without a gap >= 2R - 1 whose gaps are all ambiguous is walked by ONE lane, an item a
//                step (two 16-byte loads each).
//   the fold     k_ch_fold: one lane per output summary finds its run and its first item by search and folds in the
//                reference's order with its widths: double operations, a float (or u32) store after each, no contraction.
//   zoom blocks  itx_bwblock.h (layout, k_bw_zoom, packing, copies back); which levels there are is itx_bwzoomrule.h.
// Only the packed blocks, the section keys and the summaries go back to the host. The chain and fold kernels use no scratch; the two
// deflating kernels have the 144 bytes a lane that itx_deflate_core.h costs the dense builder's kernels too.
#include "itx_bwblock.h"
#include "itx_bwfold.h"
#include "itx_bwzoomrule.h"
#include "itx_gcovbw.h"

#include <string.h>

#include <vector>

#pragma clang fp contract(off)

typedef unsigned long long ull;

namespace {

constexpr uint32_t kWg = 256;
constexpr uint32_t kBgSecMax = 24 + 12 * kItems;      // 12 312 bytes: a bedGraph section's payload

// ---- items
__device__ __forceinline__ bool gbw_is_item(const uint4 *pts, ull n, ull j, uint4 *P, uint32_t *end)
{
    if (j + 1 >= n) return false;
    *P = pts[j];
    if (P->y == 0u) return false;
    const uint4 N = pts[j + 1];
    if (N.z != P->z) return false;
    *end = N.x;
    return true;
}

__global__ __launch_bounds__(kWg) void k_gbw_item_measure(const uint4 *__restrict__ pts, ull n, ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_w[kWg / 64u];
    const ull j = (ull)blockIdx.x * kWg + threadIdx.x;
    uint4 P;
    uint32_t end, tot = 0;
    (void)itx_tile_offsets<kWg>(gbw_is_item(pts, n, j, &P, &end) ? 1u : 0u, s_w, &tot);
    if (threadIdx.x == 0) {
        tile_sum[2ull * blockIdx.x] = tot;
        tile_sum[2ull * blockIdx.x + 1] = 0;
    }
}

__global__ __launch_bounds__(kWg) void k_gbw_item_write(const uint4 *__restrict__ pts, ull n, const ull *__restrict__ tile_base, uint4 *__restrict__ items)
{
    __shared__ uint32_t s_w[kWg / 64u];
    const ull j = (ull)blockIdx.x * kWg + threadIdx.x;
    uint4 P;
    uint32_t end = 0, tot = 0;
    const bool is = gbw_is_item(pts, n, j, &P, &end);
    const uint32_t off = itx_tile_offsets<kWg>(is ? 1u : 0u, s_w, &tot);
    if (is) items[tile_base[2ull * blockIdx.x] + off] = make_uint4(P.z, P.x, end, P.y);
}

// first[v], v in 0 .. nv: the first item whose chromosome is >= v
__global__ void k_gbw_lower(const uint4 *__restrict__ items, uint32_t n, uint32_t nv, uint32_t *__restrict__ first)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > nv) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (items[mid].x >= v) hi = mid;
        else lo = mid + 1u;
    }
    first[v] = lo;
}

__global__ void k_gbw_remap(uint4 *__restrict__ items, uint32_t n, const uint32_t *__restrict__ id_of, uint32_t nv)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = items[i].x;
    items[i].x = v < nv ? id_of[v] : 0u;
}

// ---- sections
struct GbwSec {
    const uint4 *items;
    const uint64_t *sec_first;        // [n_chrom + 1]
    const uint32_t *item_first;       // [n_chrom + 1]
    uint32_t n_chrom;
};

__device__ __forceinline__ void gbw_section_of(const GbwSec &S, ull b, uint32_t *c, uint32_t *first, uint32_t *cnt)
{
    *c = find_chrom(S.sec_first, S.n_chrom, b);
    *first = S.item_first[*c] + (uint32_t)(b - S.sec_first[*c]) * kItems;
    const uint32_t left = S.item_first[*c + 1] - *first;
    *cnt = left < kItems ? left : kItems;
}

// stat[5 b ..]: chromosome id, first start, last end, item count, smallest item length
__global__ __launch_bounds__(64) void k_gbw_secstat(GbwSec S, uint32_t *__restrict__ stat)
{
    uint32_t c, first, cnt;
    gbw_section_of(S, blockIdx.x, &c, &first, &cnt);
    uint32_t mn = 0xffffffffu;
    for (uint32_t q = threadIdx.x; q < cnt; q += 64u) {
        const uint4 it = S.items[first + q];
        const uint32_t len = it.z - it.y;
        mn = len < mn ? len : mn;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_down((int32_t)mn, o, 64);
        mn = t < mn ? t : mn;
    }
    if (threadIdx.x == 0) {
        uint32_t *o = stat + 5ull * blockIdx.x;
        o[0] = c;
        o[1] = S.items[first].y;
        o[2] = S.items[first + cnt - 1u].z;
        o[3] = cnt;
        o[4] = mn;
    }
}

// one wave per section: bwgCreate.c:45-135 for bwgTypeBedGraph
__global__ __launch_bounds__(64) void k_gbw_sections(GbwSec S, const ull *__restrict__ out_off, uint8_t *__restrict__ out, uint32_t *__restrict__ csize)
{
    __shared__ BwLds<kBgSecMax> s;
    const uint32_t lane = threadIdx.x;
    uint32_t c, first, cnt;
    gbw_section_of(S, blockIdx.x, &c, &first, &cnt);
    const uint32_t n = 24u + 12u * cnt, words = n / 4u;
    for (uint32_t i = words + lane; i < kBgSecMax / 4u + 4u; i += 64u) s.in[i] = 0u;
    for (uint32_t q = lane; q < cnt; q += 64u) {
        const uint4 it = S.items[first + q];
        s.in[6u + 3u * q] = it.y;
        s.in[7u + 3u * q] = it.z;
        s.in[8u + 3u * q] = __float_as_uint((float)(double)it.w);
    }
    if (lane == 0) {
        s.in[0] = c;
        s.in[1] = S.items[first].y;
        s.in[2] = S.items[first + cnt - 1u].z;
        s.in[3] = 0u;                                                     // step, span: not used by this type
        s.in[4] = 0u;
        s.in[5] = 1u | cnt << 16;                                         // bwgTypeBedGraph, reserved, item count
    }
    __syncthreads();
    const uint32_t z = itxd_deflate(ws_of(s), n, out + out_off[blockIdx.x], lane, 64);
    if (lane == 0) csize[blockIdx.x] = z;
}

// ---- the chain
struct ChIn {
    const uint32_t *it;               // n items of w words each: chromosome id, start, end, ...
    uint32_t w, n, red;
    const uint32_t *size;             // [n_chrom]
};

__device__ __forceinline__ uint4 ch_head(const ChIn &I, uint32_t i) { return *reinterpret_cast<const uint4 *>(I.it + (size_t)i * I.w); }

// 1: a definite anchor, 2: ambiguous, 0: never an anchor
__device__ __forceinline__ uint32_t ch_flag(const ChIn &I, uint32_t i)
{
    if (i >= I.n) return 0u;
    if (i == 0u) return 1u;
    const uint4 p = ch_head(I, i - 1u), c = ch_head(I, i);
    if (p.x != c.x) return 1u;
    const ull gap = (ull)c.y - (ull)p.z, R = I.red;                        // (an overlap would wrap: an anchor, and harmless)
    if (gap >= 2ull * R - 1ull) return 1u;
    return gap >= R ? 2u : 0u;
}

__global__ __launch_bounds__(kWg) void k_ch_flag_measure(ChIn I, ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_a[kWg / 64u], s_b[kWg / 64u];
    const uint32_t f = ch_flag(I, blockIdx.x * kWg + threadIdx.x);
    uint32_t td = 0, ta = 0;
    (void)itx_tile_offsets<kWg>(f == 1u ? 1u : 0u, s_a, &td);
    (void)itx_tile_offsets<kWg>(f == 2u ? 1u : 0u, s_b, &ta);
    if (threadIdx.x == 0) {
        tile_sum[2ull * blockIdx.x] = td;
        tile_sum[2ull * blockIdx.x + 1] = ta;
    }
}

// anc[i]: is a definite anchor; def_list / def_amb: the definite anchors and how many ambiguous items lie before each; amb_list
__global__ __launch_bounds__(kWg) void k_ch_flag_write(ChIn I, const ull *__restrict__ tile_base, uint8_t *__restrict__ anc, uint32_t *__restrict__ def_list,
                                                       uint32_t *__restrict__ def_amb, uint32_t *__restrict__ amb_list)
{
    __shared__ uint32_t s_a[kWg / 64u], s_b[kWg / 64u];
    const uint32_t i = blockIdx.x * kWg + threadIdx.x, f = ch_flag(I, i);
    uint32_t td = 0, ta = 0;
    const uint32_t od = itx_tile_offsets<kWg>(f == 1u ? 1u : 0u, s_a, &td), oa = itx_tile_offsets<kWg>(f == 2u ? 1u : 0u, s_b, &ta);
    if (i >= I.n) return;
    const uint32_t dpos = (uint32_t)tile_base[2ull * blockIdx.x] + od, apos = (uint32_t)tile_base[2ull * blockIdx.x + 1] + oa;
    anc[i] = f == 1u;
    if (f == 1u) {
        def_list[dpos] = i;
        def_amb[dpos] = apos;
    } else if (f == 2u) {
        amb_list[apos] = i;
    }
}

// tot[0], tot[1]: the numbers of definite anchors and of ambiguous items
__global__ __launch_bounds__(kWg) void k_ch_walk(ChIn I, const uint32_t *__restrict__ def_list, const uint32_t *__restrict__ def_amb,
                                                 const uint32_t *__restrict__ amb_list, const ull *__restrict__ tot, uint8_t *__restrict__ anc)
{
    const ull d = (ull)blockIdx.x * kWg + threadIdx.x, nd = tot[0], na = tot[1];
    if (d >= nd) return;
    const uint32_t lo = def_amb[d], hi = d + 1 < nd ? def_amb[d + 1] : (uint32_t)na;
    const ull R = I.red;
    ull a = ch_head(I, def_list[d]).y;
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t m = amb_list[j];                                    // (m >= 1: item 0 is a definite anchor)
        const uint4 c = ch_head(I, m), p = ch_head(I, m - 1u);
        const ull size = I.size[c.x], pe = p.z < size ? p.z : size;
        ull E = a + ((pe - 1ull - a) / R + 1ull) * R;                     // the end of the summary that holds the base before the gap
        if (E > size) E = size;
        if ((ull)c.y >= E + R) {
            anc[m] = 1;
            a = c.y;
        }
    }
}

__global__ __launch_bounds__(kWg) void k_ch_anc_measure(const uint8_t *__restrict__ anc, uint32_t n, ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_w[kWg / 64u];
    const uint32_t i = blockIdx.x * kWg + threadIdx.x;
    uint32_t tot = 0;
    (void)itx_tile_offsets<kWg>(i < n && anc[i] ? 1u : 0u, s_w, &tot);
    if (threadIdx.x == 0) {
        tile_sum[2ull * blockIdx.x] = tot;
        tile_sum[2ull * blockIdx.x + 1] = 0;
    }
}

// anc_list[r]: the anchor of run r; run_of[i]: the run of item i (item 0 is an anchor, so every item has one)
__global__ __launch_bounds__(kWg) void k_ch_anc_write(const uint8_t *__restrict__ anc, uint32_t n, const ull *__restrict__ tile_base, uint32_t *__restrict__ anc_list,
                                                      uint32_t *__restrict__ run_of)
{
    __shared__ uint32_t s_w[kWg / 64u];
    const uint32_t i = blockIdx.x * kWg + threadIdx.x;
    const uint32_t is = i < n && anc[i] ? 1u : 0u;
    uint32_t tot = 0;
    const uint32_t at = (uint32_t)tile_base[2ull * blockIdx.x] + itx_tile_offsets<kWg>(is, s_w, &tot);
    if (i >= n) return;
    if (is) anc_list[at] = i;
    run_of[i] = at + is - 1u;
}

// the summaries item i opens: those from the one after the item before it (of the same run) up to the one its last base lies in
__device__ __forceinline__ uint32_t ch_cells(const ChIn &I, const uint32_t *anc_list, const uint32_t *run_of, uint32_t i, bool *is_anchor)
{
    const uint32_t ia = anc_list[run_of[i]];
    const uint4 h = ch_head(I, i);
    const ull R = I.red, a = ch_head(I, ia).y, size = I.size[h.x];
    const ull e = h.z < size ? h.z : size, last = (e - 1ull - a) / R;
    *is_anchor = i == ia;
    if (i == ia) return (uint32_t)(last + 1ull);
    const uint4 p = ch_head(I, i - 1u);
    const ull pe = p.z < size ? p.z : size;
    return (uint32_t)(last - (pe - 1ull - a) / R);
}

__global__ __launch_bounds__(kWg) void k_ch_cell_measure(ChIn I, const uint32_t *__restrict__ anc_list, const uint32_t *__restrict__ run_of, ull *__restrict__ tile_sum)
{
    __shared__ ull s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kWg + threadIdx.x;
    bool an = false;
    const uint32_t c = i < I.n ? ch_cells(I, anc_list, run_of, i, &an) : 0u;
    if (c) atomicAdd(&s_sum, (ull)c);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_sum[2ull * blockIdx.x] = s_sum;
        tile_sum[2ull * blockIdx.x + 1] = 0;
    }
}

// run_base[r]: the first summary of run r; run_base[n_runs] = n_cells (the host checked n_cells < 2^31: the lanes' sums fit u32)
__global__ __launch_bounds__(kWg) void k_ch_runbase(ChIn I, const uint32_t *__restrict__ anc_list, const uint32_t *__restrict__ run_of, const ull *__restrict__ tile_base,
                                                    uint32_t n_runs, uint32_t n_cells, uint32_t *__restrict__ run_base)
{
    __shared__ uint32_t s_w[kWg / 64u];
    const uint32_t i = blockIdx.x * kWg + threadIdx.x;
    bool an = false;
    const uint32_t c = i < I.n ? ch_cells(I, anc_list, run_of, i, &an) : 0u;
    uint32_t tot = 0;
    const uint32_t off = itx_tile_offsets<kWg>(c, s_w, &tot);
    if (an) run_base[run_of[i]] = (uint32_t)tile_base[2ull * blockIdx.x] + off;
    if (i == 0u) run_base[n_runs] = n_cells;
}

// ---- the fold: host/bw_sum.c add_to_summary with itx_bwfold.h's step, one lane per summary. L0: the items are level-0 items (bbiAddRangeToSummary's
// numbers: valid count = size, sum = size * val, sum of squares = sum * val), otherwise the summaries of the level below
template <bool L0>
__global__ __launch_bounds__(kWg) void k_ch_fold(ChIn I, const uint32_t *__restrict__ anc_list, const uint32_t *__restrict__ run_base, uint32_t n_runs, uint32_t n_out,
                                                 itx_bw_summary *__restrict__ out)
{
    const uint32_t j = blockIdx.x * kWg + threadIdx.x;
    if (j >= n_out) return;
    uint32_t lo = 0, hi = n_runs;                                          // run_base[lo] <= j < run_base[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (run_base[mid] <= j) lo = mid;
        else hi = mid;
    }
    const uint32_t ia = anc_list[lo], ie = lo + 1u < n_runs ? anc_list[lo + 1u] : I.n;
    const uint4 h0 = ch_head(I, ia);
    const uint32_t c = h0.x, size = I.size[c];
    const ull cs64 = (ull)h0.y + (ull)(j - run_base[lo]) * I.red, ce64 = cs64 + I.red;
    const uint32_t cs = (uint32_t)cs64, ce = ce64 < size ? (uint32_t)ce64 : size;
    uint32_t a = ia, b = ie;                                               // the first item that ends behind cs
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2u;
        const uint32_t e = ch_head(I, mid).z;
        if ((e < size ? e : size) > cs) b = mid;
        else a = mid + 1u;
    }
    itx_bw_summary acc = {c, cs, ce, 0, 0, 0, 0, 0};
    bool fresh = true;
    for (uint32_t i = a; i < ie; i++) {
        uint32_t s, e, ivc;
        double imn, imx, isd, isq;
        if (L0) {
            const uint4 t = ch_head(I, i);
            s = t.y;
            e = t.z;
            const double val = (double)(float)(double)t.w;
            const int isz = (int)(e - s);
            ivc = (uint32_t)isz;
            imn = imx = val;
            isd = isz * val;
            isq = isd * val;
        } else {
            const itx_bw_summary t = reinterpret_cast<const itx_bw_summary *>(I.it)[i];
            s = t.start;
            e = t.end;
            ivc = t.valid_count;
            imn = (double)t.min_val;
            imx = (double)t.max_val;
            isd = (double)t.sum_data;
            isq = (double)t.sum_squares;
        }
        if (s >= ce) break;
        const uint32_t ec = e < size ? e : size, st = s > cs ? s : cs;    // st: where the item stands when this summary is open
        const int overlap = (int)((ec < ce ? ec : ce) - st), left = (int)(ec - st);
        const double f = (double)overlap / left;
        if (fresh) {
            itx_bwfold_open(&acc, imn, imx);
            fresh = false;
        }
        itx_bwfold_add(&acc, f, (double)ivc, imn, imx, isd, isq);
    }
    out[j] = acc;
}

// ---- host side
struct Chain {                        // what a chain over n items works in
    ItxBuf anc, def_list, def_amb, amb_list, anc_list, run_of, run_base, tsum, tbase, tot;
    ull *h_tot = nullptr;             // page-locked, 4 words
    ~Chain()
    {
        if (h_tot) (void)hipHostFree(h_tot);
    }
};

#define GBW_NEED(buf, bytes)                                                                  \
    do {                                                                                      \
        if ((rc = itx_buf_need("itx_gcov_bigwig_build", (buf), (bytes))) != ITX_OK) goto out; \
    } while (0)

struct Timer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Timer()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// the counting form: the runs and the number of summaries of reduction I.red over I's items
int chain_count(hipStream_t st, Chain &C, const ChIn &I, uint32_t *n_runs, ull *n_cells)
{
    int rc = ITX_OK;
    const uint32_t n = I.n, nt = (n + kWg - 1u) / kWg;
    const size_t words = 4 * ((size_t)n + 1);
    GBW_NEED(C.anc, (size_t)n + 1);
    GBW_NEED(C.def_list, words);
    GBW_NEED(C.def_amb, words);
    GBW_NEED(C.amb_list, words);
    GBW_NEED(C.anc_list, words);
    GBW_NEED(C.run_of, words);
    GBW_NEED(C.run_base, words + 4);
    GBW_NEED(C.tsum, 16 * ((size_t)nt + 1));
    GBW_NEED(C.tbase, 16 * ((size_t)nt + 1));
    GBW_NEED(C.tot, 64);
    if (!C.h_tot) ITX_TRY(hipHostMalloc((void **)&C.h_tot, 64, hipHostMallocDefault));
    {
        ull *tsum = C.tsum.as<ull>(), *tbase = C.tbase.as<ull>(), *tot = C.tot.as<ull>();
        hipLaunchKernelGGL(k_ch_flag_measure, dim3(nt), dim3(kWg), 0, st, I, tsum);
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, tsum, nt, tbase, tot);
        hipLaunchKernelGGL(k_ch_flag_write, dim3(nt), dim3(kWg), 0, st, I, tbase, C.anc.as<uint8_t>(), C.def_list.as<uint32_t>(), C.def_amb.as<uint32_t>(),
                           C.amb_list.as<uint32_t>());
        // (at most n definite anchors: the grid covers them all, lanes past tot[0] leave)
        hipLaunchKernelGGL(k_ch_walk, dim3(nt), dim3(kWg), 0, st, I, C.def_list.as<uint32_t>(), C.def_amb.as<uint32_t>(), C.amb_list.as<uint32_t>(), tot,
                           C.anc.as<uint8_t>());
        hipLaunchKernelGGL(k_ch_anc_measure, dim3(nt), dim3(kWg), 0, st, C.anc.as<uint8_t>(), n, tsum);
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, tsum, nt, tbase, tot + 2);
        hipLaunchKernelGGL(k_ch_anc_write, dim3(nt), dim3(kWg), 0, st, C.anc.as<uint8_t>(), n, tbase, C.anc_list.as<uint32_t>(), C.run_of.as<uint32_t>());
        hipLaunchKernelGGL(k_ch_cell_measure, dim3(nt), dim3(kWg), 0, st, I, C.anc_list.as<uint32_t>(), C.run_of.as<uint32_t>(), tsum);
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, tsum, nt, tbase, tot + 4);
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(C.h_tot, tot, 48, hipMemcpyDeviceToHost, st));
        ITX_TRY(hipStreamSynchronize(st));
        *n_runs = (uint32_t)C.h_tot[2];
        *n_cells = C.h_tot[4];
        if (*n_cells >= 0x80000000ull) {
            itx_set_error("itx_gcov_bigwig_build: %llu summaries at reduction %u, 2^31 and more", *n_cells, I.red);
            rc = ITX_E_LIMIT;
        }
    }
out:
    return rc;
}

// after chain_count for the same I (its tile bases still hold the cells' scan): the summaries themselves
int chain_fold(hipStream_t st, Chain &C, const ChIn &I, bool level0, uint32_t n_runs, uint32_t n_cells, itx_bw_summary *out)
{
    int rc = ITX_OK;
    const uint32_t nt = (I.n + kWg - 1u) / kWg, no = (n_cells + kWg - 1u) / kWg;
    hipLaunchKernelGGL(k_ch_runbase, dim3(nt), dim3(kWg), 0, st, I, C.anc_list.as<uint32_t>(), C.run_of.as<uint32_t>(), C.tbase.as<ull>(), n_runs, n_cells,
                       C.run_base.as<uint32_t>());
    if (level0) hipLaunchKernelGGL(k_ch_fold<true>, dim3(no), dim3(kWg), 0, st, I, C.anc_list.as<uint32_t>(), C.run_base.as<uint32_t>(), n_runs, n_cells, out);
    else hipLaunchKernelGGL(k_ch_fold<false>, dim3(no), dim3(kWg), 0, st, I, C.anc_list.as<uint32_t>(), C.run_base.as<uint32_t>(), n_runs, n_cells, out);
    ITX_TRY(hipGetLastError());
out:
    return rc;
}

}  // namespace

struct GcBw {                         // what a build leaves: host memory only
    ull n_items = 0;
    uint32_t rounds = 0;
    std::vector<uint32_t> chrom, sec_key, sec_count;
    uint32_t reduction[kBwMaxLevels] = {0};
    BwPack pack;                      // (its device buffers go when the blocks are back)
    double ms[4] = {0, 0, 0, 0};      // items and sections' numbers, chains, folds, deflate and packing
};

void gcbw_free(GcBw *b) { delete b; }

double gcbw_device_ms(const GcBw *b) { return b->ms[0] + b->ms[1] + b->ms[2] + b->ms[3]; }

void gcbw_result(const GcBw *b, itx_gcov_bw_result *out)
{
    memset(out, 0, sizeof *out);
    out->n_items = b->n_items;
    if (!b->n_items) return;
    bw_pack_result(b->pack, out);
    out->n_chrom = (uint32_t)b->chrom.size();
    out->chrom = b->chrom.data();
    out->sec_key = b->sec_key.data();
    out->sec_count = b->sec_count.data();
    for (uint32_t k = 0; k < b->pack.L.n; k++) out->reduction[k] = b->reduction[k];
    out->reduce_rounds = b->rounds;
    out->items_ms = b->ms[0];
    out->chain_ms = b->ms[1];
    out->fold_ms = b->ms[2];
    out->deflate_ms = b->ms[3];
}

// the device time from T.e0 (recorded by the caller) to here is added to *acc; the stream is idle afterwards
static int gbw_lap(hipStream_t st, Timer &T, double *acc)
{
    int rc = ITX_OK;
    float ms = 0;
    ITX_TRY(hipEventRecord(T.e1, st));
    ITX_TRY(hipEventSynchronize(T.e1));
    ITX_TRY(hipEventElapsedTime(&ms, T.e0, T.e1));
    *acc += (double)ms;
    ITX_TRY(hipEventRecord(T.e0, st));
out:
    return rc;
}

int gcbw_build(int device, hipStream_t st, const uint4 *pts, ull n_pts, const uint32_t *vsize, const uint32_t *vchrom, uint32_t nv, GcBw **out)
{
    int rc = ITX_OK;
    *out = nullptr;
    GcBw *B = new GcBw();
    Chain C;
    Timer T;
    ItxBuf items, first, idmap, sizes, sec_first, item_first, secstat, tsum, tbase, tot, level[kBwMaxLevels];
    std::vector<uint32_t> h_first((size_t)nv + 1, 0u), id_of(nv ? nv : 1, 0u), id_size, id_item_first, h_stat, payload;
    std::vector<ull> id_sec_first;
    uint32_t n_items = 0, n_chrom = 0, n_sec = 0;
    ull h_tot[2] = {0, 0};
    ITX_TRY(hipSetDevice(device));
    ITX_TRY(hipEventCreate(&T.e0));
    ITX_TRY(hipEventCreate(&T.e1));
    ITX_TRY(hipEventRecord(T.e0, st));
    // ---- the items
    if (n_pts >= 2) {
        if ((n_pts + kWg - 1) / kWg > 0x7fffffffull) {
            itx_set_error("itx_gcov_bigwig_build: %llu change points", n_pts);
            rc = ITX_E_LIMIT;
            goto out;
        }
        const uint32_t nt = (uint32_t)((n_pts + kWg - 1) / kWg);
        GBW_NEED(tsum, 16 * ((size_t)nt + 1));
        GBW_NEED(tbase, 16 * ((size_t)nt + 1));
        GBW_NEED(tot, 64);
        hipLaunchKernelGGL(k_gbw_item_measure, dim3(nt), dim3(kWg), 0, st, pts, n_pts, tsum.as<ull>());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, tsum.as<ull>(), nt, tbase.as<ull>(), tot.as<ull>());
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(h_tot, tot.as<ull>(), 16, hipMemcpyDeviceToHost, st));
        ITX_TRY(hipStreamSynchronize(st));
        if (h_tot[0] >= 0x80000000ull) {
            itx_set_error("itx_gcov_bigwig_build: %llu items, 2^31 and more", h_tot[0]);
            rc = ITX_E_LIMIT;
            goto out;
        }
        n_items = (uint32_t)h_tot[0];
        if (n_items) {
            GBW_NEED(items, 16 * (size_t)n_items);
            GBW_NEED(first, 4 * ((size_t)nv + 1));
            hipLaunchKernelGGL(k_gbw_item_write, dim3(nt), dim3(kWg), 0, st, pts, n_pts, tbase.as<ull>(), items.as<uint4>());
            hipLaunchKernelGGL(k_gbw_lower, dim3((nv + 1 + kWg - 1) / kWg), dim3(kWg), 0, st, items.as<uint4>(), n_items, nv, first.as<uint32_t>());
            ITX_TRY(hipGetLastError());
            ITX_TRY(hipMemcpyAsync(h_first.data(), first.p, 4 * ((size_t)nv + 1), hipMemcpyDeviceToHost, st));
            ITX_TRY(hipStreamSynchronize(st));
        }
    }
    B->n_items = n_items;
    if (!n_items) {                                                        // no data: no file (the converter refuses such an input)
        *out = B;
        return ITX_OK;
    }
    // ---- ids for the chromosomes with an item, and their sections
    id_sec_first.push_back(0);
    for (uint32_t v = 0; v < nv; v++) {
        const uint32_t cnt = h_first[v + 1] - h_first[v];
        if (!cnt) continue;
        id_of[v] = n_chrom++;
        B->chrom.push_back(vchrom[v]);
        id_size.push_back(vsize[v]);
        id_item_first.push_back(h_first[v]);
        id_sec_first.push_back(id_sec_first.back() + (cnt + kItems - 1) / kItems);
    }
    id_item_first.push_back(n_items);
    n_sec = (uint32_t)id_sec_first.back();
    GBW_NEED(idmap, 4 * (size_t)(nv ? nv : 1));
    GBW_NEED(sizes, 4 * (size_t)n_chrom);
    GBW_NEED(sec_first, 8 * ((size_t)n_chrom + 1));
    GBW_NEED(item_first, 4 * ((size_t)n_chrom + 1));
    GBW_NEED(secstat, 20 * (size_t)n_sec);
    h_stat.resize(5 * (size_t)n_sec);
    ITX_TRY(hipMemcpyAsync(idmap.p, id_of.data(), 4 * (size_t)nv, hipMemcpyHostToDevice, st));
    ITX_TRY(hipMemcpyAsync(sizes.p, id_size.data(), 4 * (size_t)n_chrom, hipMemcpyHostToDevice, st));
    ITX_TRY(hipMemcpyAsync(sec_first.p, id_sec_first.data(), 8 * ((size_t)n_chrom + 1), hipMemcpyHostToDevice, st));
    ITX_TRY(hipMemcpyAsync(item_first.p, id_item_first.data(), 4 * ((size_t)n_chrom + 1), hipMemcpyHostToDevice, st));
    {
        const GbwSec S = {items.as<uint4>(), sec_first.as<uint64_t>(), item_first.as<uint32_t>(), n_chrom};
        hipLaunchKernelGGL(k_gbw_remap, dim3((n_items + kWg - 1) / kWg), dim3(kWg), 0, st, items.as<uint4>(), n_items, idmap.as<uint32_t>(), nv);
        hipLaunchKernelGGL(k_gbw_secstat, dim3(n_sec), dim3(64), 0, st, S, secstat.as<uint32_t>());
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(h_stat.data(), secstat.p, 20 * (size_t)n_sec, hipMemcpyDeviceToHost, st));
        if ((rc = gbw_lap(st, T, &B->ms[0])) != ITX_OK) goto out;         // (waits: the host vectors above are this function's)
        ull total_res = 0, full_size = 0;
        B->sec_key.resize(3 * (size_t)n_sec);
        B->sec_count.resize(n_sec);
        for (uint32_t s = 0; s < n_sec; s++) {
            const uint32_t *q = &h_stat[5 * (size_t)s];
            B->sec_key[3 * (size_t)s] = q[0];
            B->sec_key[3 * (size_t)s + 1] = q[1];
            B->sec_key[3 * (size_t)s + 2] = q[2];
            B->sec_count[s] = q[3];
            total_res += (ull)(int)q[4];
            full_size += 24 + 12 * (ull)q[3];
        }
        // ---- the levels (itx_bwzoomrule.h): the first reduction is counted until it fits, every further one from the last level kept
        itx_bwzoom Z;
        uint64_t n_sum[kBwMaxLevels] = {0};
        ull n_cells = 0;
        uint32_t n_runs = 0;
        ChIn I = {items.as<uint32_t>(), 4u, n_items, (uint32_t)0, sizes.as<uint32_t>()};
        int w = itx_bwzoom_init(&Z, full_size, (int)((total_res + n_sec / 2u) / n_sec), n_chrom);
        while (w == ITX_BWZ_COUNT) {
            I.red = (uint32_t)Z.red;
            if ((rc = chain_count(st, C, I, &n_runs, &n_cells)) != ITX_OK) goto out;
            w = itx_bwzoom_first(&Z, n_cells);
        }
        if (w == ITX_BWZ_RANGE) {
            itx_set_error("itx_gcov_bigwig_build: a first reduction of %lld", Z.red);
            rc = ITX_E_LIMIT;
            goto out;
        }
        if ((rc = gbw_lap(st, T, &B->ms[1])) != ITX_OK) goto out;
        GBW_NEED(level[0], 32 * ((size_t)n_cells + 1));
        if ((rc = chain_fold(st, C, I, true, n_runs, (uint32_t)n_cells, level[0].as<itx_bw_summary>())) != ITX_OK) goto out;
        if ((rc = gbw_lap(st, T, &B->ms[2])) != ITX_OK) goto out;
        n_sum[0] = n_cells;
        while (itx_bwzoom_next(&Z)) {
            const int k = Z.n_levels;
            const ChIn J = {level[k - 1].as<uint32_t>(), 8u, (uint32_t)n_sum[k - 1], (uint32_t)Z.red, sizes.as<uint32_t>()};
            if ((rc = chain_count(st, C, J, &n_runs, &n_cells)) != ITX_OK) goto out;
            if ((rc = gbw_lap(st, T, &B->ms[1])) != ITX_OK) goto out;
            if (!itx_bwzoom_keep(&Z, n_cells)) continue;
            GBW_NEED(level[k], 32 * ((size_t)n_cells + 1));
            if ((rc = chain_fold(st, C, J, false, n_runs, (uint32_t)n_cells, level[k].as<itx_bw_summary>())) != ITX_OK) goto out;
            if ((rc = gbw_lap(st, T, &B->ms[2])) != ITX_OK) goto out;
            n_sum[k] = n_cells;
        }
        B->rounds = Z.reduce_rounds;
        memcpy(B->reduction, Z.reduction, sizeof B->reduction);
        // ---- the blocks (itx_bwblock.h): sections, then each level's zoom blocks; deflated, packed, copied back with the summaries
        BwPack &P = B->pack;
        payload.resize(n_sec);
        for (uint32_t s = 0; s < n_sec; s++) payload[s] = 24u + 12u * B->sec_count[s];
        if ((rc = bw_pack_layout(P, "itx_gcov_bigwig_build", st, payload.data(), n_sec, (uint32_t)Z.n_levels, n_sum)) != ITX_OK) goto out;
        for (int k = 0; k < Z.n_levels; k++) P.L.sum[k] = level[k].as<itx_bw_summary>();
        hipLaunchKernelGGL(k_gbw_sections, dim3(n_sec), dim3(64), 0, st, S, P.out_off.as<ull>(), P.out.as<uint8_t>(), P.csize.as<uint32_t>());
        if ((rc = bw_pack_run(P, st)) != ITX_OK) goto out;
        if ((rc = gbw_lap(st, T, &B->ms[3])) != ITX_OK) goto out;
        if ((rc = bw_pack_collect(P, "itx_gcov_bigwig_build", st)) != ITX_OK) goto out;
        for (ItxBuf *d : {&P.out, &P.packed, &P.out_off, &P.poff, &P.csize}) d->drop();   // (what is kept is host memory)
    }
out:
    if (rc != ITX_OK) {
        (void)hipStreamSynchronize(st);                                    // before the buffers above are freed
        delete B;
        return rc;
    }
    *out = B;
    return ITX_OK;
}
