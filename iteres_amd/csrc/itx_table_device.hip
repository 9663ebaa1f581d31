// itx_table_device.hip — the repeat table built on the device (the default build).
// The same table, built where it will live: the rows cross the link once, both orders come from itx_sort_run, pbelow is a
// segmented running maximum across workgroups, the binned index one lane per bin. The calling thread validates the rows and
// finds the units in ONE pass (no host thread is started: the reader's copy threads and the decoder's producer need the cores
// at that moment), everything else runs on a stream of the build's own, which is waited for at the end — not the device.
#include "itx_radixsort.h"
#include "itx_table_priv.h"

#include <algorithm>
#include <utility>
#include <vector>

static_assert(sizeof(uint2) == sizeof(TbPair) && sizeof(uint4) == sizeof(TbQuad), "the rules' plain structs are cast to the device's vector types");

#define TB_RUN_WG 256u
#define TB_RUN_ROWS 32u                                  // rows per thread of k_tb_runs
#define TB_RUN_BLOCK (TB_RUN_WG * TB_RUN_ROWS)

// file order, keyed for binKeeperFind's return order inside a chromosome
static __global__ __launch_bounds__(256) void k_tb_rank_keys(const itx_row *__restrict__ rows, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    int level = 0, bin = 0;
    (void)tb_bin_of_range((int)rows[i].start, (int)rows[i].end, &level, &bin);        // (the host's pass has vouched for the row)
    keys[i] = make_uint2(tb_rank_key(level, bin), i);
}
// file order, keyed by start
static __global__ __launch_bounds__(256) void k_tb_start_keys(const itx_row *__restrict__ rows, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = make_uint2(rows[i].start, i);
}
// the order so far, keyed by chromosome for the last passes
static __global__ __launch_bounds__(256) void k_tb_chrom_keys(const itx_row *__restrict__ rows, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) keys[k].x = (uint32_t)rows[keys[k].y].chrom;
}
// rank = place inside the chromosome in the order by (chromosome, level desc, bin desc, file order)
static __global__ __launch_bounds__(256) void k_tb_ranks(const uint2 *__restrict__ keys, uint32_t n, const itx_row *__restrict__ rows,
                                                         const uint32_t *__restrict__ chrom_off, uint32_t *__restrict__ rank)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = keys[k].y;
    rank[i] = k - chrom_off[rows[i].chrom];
}
// the records in (chromosome, start, file order) order, all but pbelow
static __global__ __launch_bounds__(256) void k_tb_rows(const uint2 *__restrict__ order, uint32_t n, const itx_row *__restrict__ rows, const uint32_t *__restrict__ rep_len,
                                                        const uint32_t *__restrict__ first_unit, const uint4 *__restrict__ unit_ids, const uint32_t *__restrict__ unit_slot,
                                                        uint32_t n_units, const uint32_t *__restrict__ rank, ItxIv *__restrict__ iv, int32_t *__restrict__ orig,
                                                        uint32_t *__restrict__ row_unit, int32_t *__restrict__ schrom)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = order[k].y;
    const itx_row r = rows[i];
    const uint32_t u = tb_row_unit(r, first_unit, (const TbQuad *)unit_ids, n_units);
    iv[k] = tb_row_record(r, rep_len[r.rep], unit_slot[u], rank[i]);
    orig[k] = (int32_t)i;
    row_unit[k] = u;
    schrom[k] = r.chrom;
}
// pbelow. A workgroup takes TB_RUN_BLOCK sorted rows, a thread TB_RUN_ROWS of them in a row; the stretches' summaries (TbRun)
// are joined across the workgroup. WRITE false: the workgroup's own summary goes to totals; true: with what precedes the
// workgroup (carry, from k_tb_carry) every row gets the maximum end of its chromosome's rows below it.
template <bool WRITE>
static __global__ __launch_bounds__(TB_RUN_WG) void k_tb_runs(ItxIv *__restrict__ iv, const int32_t *__restrict__ schrom, uint32_t n, const TbRun *__restrict__ carry,
                                                              TbRun *__restrict__ totals)
{
    __shared__ TbRun s[TB_RUN_WG];
    const uint32_t t = threadIdx.x;
    const uint64_t lo0 = (uint64_t)blockIdx.x * TB_RUN_BLOCK + (uint64_t)t * TB_RUN_ROWS;
    const uint64_t lo = lo0 < n ? lo0 : n, hi = lo + TB_RUN_ROWS < n ? lo + TB_RUN_ROWS : n;
    TbRun mine = tb_run_empty();
    for (uint64_t k = lo; k < hi; k++) mine = tb_run_push(mine, schrom[k], iv[k].e);
    s[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < TB_RUN_WG; d <<= 1) {
        TbRun v = tb_run_empty();
        if (t >= d) v = s[t - d];
        __syncthreads();
        if (t >= d) s[t] = tb_run_join(v, s[t]);
        __syncthreads();
    }
    if (!WRITE) {
        if (t == TB_RUN_WG - 1) totals[blockIdx.x] = s[t];
        return;
    }
    TbRun before = carry[blockIdx.x];
    if (t > 0) before = tb_run_join(before, s[t - 1]);
    for (uint64_t k = lo; k < hi; k++) {
        const int32_t c = schrom[k], e = iv[k].e;
        iv[k].pbelow = tb_run_below(before, c);
        before = tb_run_push(before, c, e);
    }
}
// what precedes every workgroup of k_tb_runs: a few hundred summaries, one thread
static __global__ void k_tb_carry(const TbRun *__restrict__ totals, uint32_t n_blocks, TbRun *__restrict__ carry)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    TbRun acc = tb_run_empty();
    for (uint32_t b = 0; b < n_blocks; b++) {
        carry[b] = acc;
        acc = tb_run_join(acc, totals[b]);
    }
}
// the binned index, one lane per bin: both bounds are bisections (starts and prefix-max ends both rise along a chromosome)
static __global__ __launch_bounds__(256) void k_tb_bins(const ItxIv *__restrict__ iv, const uint32_t *__restrict__ chrom_off, const uint32_t *__restrict__ bin_off, uint32_t n_chrom,
                                                        uint32_t n_bins, int shift, uint2 *__restrict__ bl)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_bins) return;
    const uint32_t c = tb_chrom_of_bin(bin_off, n_chrom, g);
    const uint32_t lo = chrom_off[c], hi = chrom_off[c + 1];
    const int64_t bound = tb_bin_bound(g, bin_off[c], shift);
    bl[g] = make_uint2(tb_first_start(iv, lo, hi, bound), tb_first_reach(iv, lo, hi, bound));
}
// first unit reaching into every window of 2^ITX_LOGW slots
static __global__ __launch_bounds__(256) void k_tb_part_unit(const uint32_t *__restrict__ unit_slot, uint32_t n_units, uint32_t n_win, uint32_t *__restrict__ part_unit)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < n_win) part_unit[w] = tb_window_unit(unit_slot, n_units, w);
}

// the build's stream, its stage events and (until the table owns it) its device memory
struct TbDevice {
    hipStream_t st = nullptr;
    char *base = nullptr;
    std::vector<std::pair<const char *, hipEvent_t>> marks;
    bool timing = tb_timing();
    ~TbDevice()
    {
        if (st) (void)hipStreamSynchronize(st);
        for (auto &m : marks) (void)hipEventDestroy(m.second);
        if (st) (void)hipStreamDestroy(st);
        if (base) (void)hipFree(base);
    }
    int mark(const char *what)
    {
        if (!timing) return ITX_OK;
        hipEvent_t e;
        ITX_HIP(hipEventCreate(&e));
        ITX_HIP(hipEventRecord(e, st));
        marks.emplace_back(what, e);
        return ITX_OK;
    }
    void report()
    {
        for (size_t k = 1; k < marks.size(); k++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, marks[k - 1].second, marks[k].second) == hipSuccess)
                fprintf(stderr, "[itx timing] table: device %s %.3f ms\n", marks[k].first, (double)ms);
        }
    }
};
#define TB_GRID(n) dim3((unsigned)(((uint64_t)(n) + 255u) / 256u)), dim3(256)

// (chromosome, key) order of the n pairs of `from`, stable: the key's passes, then the chromosome's
static int tb_sort(hipStream_t st, const itx_row *d_rows, uint2 *from, uint2 *other, uint32_t n, uint32_t key_passes, uint32_t chrom_passes, uint32_t *hist,
                   uint2 **sorted)
{
    int rc = itx_sort_run(st, from, other, n, 0, key_passes, hist, sorted);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tb_chrom_keys, TB_GRID(n), 0, st, d_rows, n, *sorted);
    ITX_HIP(hipGetLastError());
    return itx_sort_run(st, *sorted, *sorted == from ? other : from, n, 0, chrom_passes, hist, sorted);
}

int table_create_device(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla,
                        int device, itx_table **out, size_t *bad_row)
{
    int rc;
    int64_t max_size = 0;
    for (int c = 0; c < n_chrom; c++) max_size = std::max(max_size, chrom_size[c]);
    tb_tick("start");
    // ONE pass of the calling thread: every row validated as binKeeperAdd would (the first bad row is reported), counted into
    // its chromosome, and its (name, family, class) collected
    std::vector<uint32_t> chrom_off(n_chrom + 1, 0);
    std::vector<Triple> triples;
    {
        TbTriples T(n_rep);
        for (size_t i = 0; i < n_rows; i++) {
            int level, bin;
            if (!tb_row_ok(rows[i], chrom_size, n_chrom, n_rep, n_fam, n_cla, &level, &bin)) return tb_bad_row(rows, i, bad_row);
            chrom_off[(size_t)rows[i].chrom + 1]++;
            T.add(rows[i]);
        }
        T.append_to(triples);
    }
    for (int c = 0; c < n_chrom; c++) chrom_off[c + 1] += chrom_off[c];
    tb_tick("validate + count + units' triples (one host pass)");
    TbUnits U;
    if ((rc = tb_units(triples, rep_len, n_rep, U))) return rc;
    const uint32_t n_units = U.n;
    std::vector<uint32_t> bin_off;
    const int shift = tb_bin_shift(n_rows, chrom_size, n_chrom, bin_off);
    const size_t n_bins = bin_off[n_chrom];
    tb_tick("units");

    if ((rc = tb_device_ready(device))) return rc;
    const uint32_t n = (uint32_t)n_rows;
    const uint32_t n_runs = (uint32_t)(((uint64_t)n + TB_RUN_BLOCK - 1) / TB_RUN_BLOCK);
    // the table's arrays where they will live (as the host build lays them out), the build's working memory behind them
    Carver cv;
    const TbLayout L = tb_layout(cv, n_rows, n_bins, U.slots, n_units);
    const size_t n_win = L.n_win;
    cv.take(256);
    const size_t w_rows = cv.take((n_rows + 1) * sizeof(itx_row));
    const size_t w_ka = cv.take((n_rows + 1) * sizeof(uint2)), w_kb = cv.take((n_rows + 1) * sizeof(uint2));
    const size_t w_rank = cv.take((n_rows + 1) * 4), w_schrom = cv.take((n_rows + 1) * 4);
    const size_t w_hist = cv.take(itx_sort_hist_bytes(n_rows) + 1024);
    const size_t w_tot = cv.take(((size_t)n_runs + 1) * sizeof(TbRun)), w_carry = cv.take(((size_t)n_runs + 1) * sizeof(TbRun));
    const size_t w_coff = cv.take(((size_t)n_chrom + 1) * 4), w_boff = cv.take(((size_t)n_chrom + 1) * 4);
    const size_t w_rlen = cv.take(((size_t)n_rep + 1) * 4), w_funit = cv.take(((size_t)n_rep + 1) * 4);
    const size_t total = cv.take(0) + 256;
    TbDevice D;
    ITX_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    if ((rc = tb_device_alloc(&D.base, total))) return rc;
    char *base = D.base;
    hipStream_t st = D.st;
    itx_row *d_rows = (itx_row *)(base + w_rows);
    uint2 *ka = (uint2 *)(base + w_ka), *kb = (uint2 *)(base + w_kb), *sorted = nullptr;
    uint32_t *d_rank = (uint32_t *)(base + w_rank), *d_hist = (uint32_t *)(base + w_hist);
    int32_t *d_schrom = (int32_t *)(base + w_schrom);
    uint32_t *d_coff = (uint32_t *)(base + w_coff), *d_boff = (uint32_t *)(base + w_boff), *d_rlen = (uint32_t *)(base + w_rlen),
             *d_funit = (uint32_t *)(base + w_funit);
    ItxIv *d_iv = (ItxIv *)(base + L.iv);
    uint32_t *d_uslot = (uint32_t *)(base + L.uslot);
    if ((rc = D.mark("start"))) return rc;
    // the one upload: the rows, and the few per-chromosome, per-name and per-unit numbers the host has just derived
    auto up = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    ITX_HIP(up(d_rows, rows, n_rows * sizeof(itx_row)));
    ITX_HIP(up(d_coff, chrom_off.data(), chrom_off.size() * 4));
    ITX_HIP(up(d_boff, bin_off.data(), bin_off.size() * 4));
    ITX_HIP(up(d_rlen, rep_len, (size_t)n_rep * 4));
    ITX_HIP(up(d_funit, U.first.data(), U.first.size() * 4));
    ITX_HIP(up(d_uslot, U.slot.data(), U.slot.size() * 4));
    ITX_HIP(up(base + L.uids, U.ids.data(), U.ids.size() * sizeof(uint4)));
    ITX_HIP(up(base + L.ucov, U.covoff.data(), U.covoff.size() * 8));
    if ((rc = D.mark("upload"))) return rc;
    const uint32_t chrom_passes = tb_key_passes(n_chrom > 0 ? (uint64_t)n_chrom - 1 : 0);
    if (n) {
        // ranks first: their order is only needed to number the rows, the buffers then serve the order by start
        hipLaunchKernelGGL(k_tb_rank_keys, TB_GRID(n), 0, st, d_rows, n, ka);
        ITX_HIP(hipGetLastError());
        if ((rc = tb_sort(st, d_rows, ka, kb, n, tb_key_passes((1ull << TB_RANK_KEY_BITS) - 1), chrom_passes, d_hist, &sorted))) return rc;
        hipLaunchKernelGGL(k_tb_ranks, TB_GRID(n), 0, st, sorted, n, d_rows, d_coff, d_rank);
        ITX_HIP(hipGetLastError());
        if ((rc = D.mark("ranks (sort by chromosome, level, bin)"))) return rc;
        hipLaunchKernelGGL(k_tb_start_keys, TB_GRID(n), 0, st, d_rows, n, ka);
        ITX_HIP(hipGetLastError());
        if ((rc = tb_sort(st, d_rows, ka, kb, n, tb_key_passes((uint64_t)max_size), chrom_passes, d_hist, &sorted))) return rc;
        if ((rc = D.mark("sort by chromosome, start"))) return rc;
        hipLaunchKernelGGL(k_tb_rows, TB_GRID(n), 0, st, sorted, n, d_rows, d_rlen, d_funit, (const uint4 *)(base + L.uids), d_uslot, n_units, d_rank, d_iv,
                           (int32_t *)(base + L.orig), (uint32_t *)(base + L.runit), d_schrom);
        ITX_HIP(hipGetLastError());
        TbRun *d_tot = (TbRun *)(base + w_tot), *d_carry = (TbRun *)(base + w_carry);
        hipLaunchKernelGGL(k_tb_runs<false>, dim3(n_runs), dim3(TB_RUN_WG), 0, st, d_iv, d_schrom, n, d_carry, d_tot);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tb_carry, dim3(1), dim3(64), 0, st, d_tot, n_runs, d_carry);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tb_runs<true>, dim3(n_runs), dim3(TB_RUN_WG), 0, st, d_iv, d_schrom, n, d_carry, d_tot);
        ITX_HIP(hipGetLastError());
        if ((rc = D.mark("rows + pbelow"))) return rc;
    }
    if (n_bins) {
        hipLaunchKernelGGL(k_tb_bins, TB_GRID(n_bins), 0, st, d_iv, d_coff, d_boff, (uint32_t)n_chrom, (uint32_t)n_bins, shift, (uint2 *)(base + L.bl));
        ITX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tb_part_unit, TB_GRID(n_win), 0, st, d_uslot, n_units, (uint32_t)n_win, (uint32_t *)(base + L.punit));
    ITX_HIP(hipGetLastError());
    if ((rc = D.mark("binned index + windows' units"))) return rc;
    ITX_HIP(hipStreamSynchronize(st));                                 // the build's own stream: the host arrays above may go, the table may be used
    tb_tick("device build (upload, sorts, rows, index)");
    if (D.timing) D.report();

    // (the working memory stays behind the arrays until the table goes: freeing it now would wait for everything else on the device)
    itx_table *t = tb_object(base, L, device, shift, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, U, chrom_off, bin_off);
    D.base = nullptr;
    *out = t;
    return ITX_OK;
}
