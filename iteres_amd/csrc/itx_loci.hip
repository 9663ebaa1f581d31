// itx_loci.hip — the per-locus table of `iteres filter` (writeFilterOut, generic.c:1709-1746) and `iteres cpgfilter`
// (writeFilterOutMRE, generic.c:1748-1772) built on the device. The host used to qsort every chromosome's (bin, row) pairs after
// the stream and fprintf one line per row on one thread; but the ORDER of the lines is a function of the table alone, so the sort
// runs as soon as the table is parsed, beside the scan of the alignments, and the end of the command is two kernels and a copy.
//
// create (the table):
//   k_loci_keys     (key, row) pairs in DESCENDING row order, key = chromosome rank << 13 | bin (itx_lociline.h)
//   k_sort_hist / k_sort_scan / k_sort_scatter (itx_radixsort.h)  ceil((13 + bits(n_chrom)) / 8) stable passes by key: the rows of
//                   a bin keep their descending order, which is binKeeper's "newest insertion first" (cuskent/binRange.c:185)
// text (the counts):
//   k_loci_measure  one lane per sorted place: is the line printed (count >= -t / total > -t), is it one the host has to look at
//                   (itx_loci_hard), its length; a tile of LO_TILE places adds up its bytes and its lines (64 bit)
//   k_tile_scan2    (itx_textpack.h) exclusive sums over the tiles; the totals and the hard count are all the host waits for
//   k_loci_write    one workgroup per tile: the tile's lines are ONE contiguous range of the text, staged in LDS a window at a
//                   time and stored with 16-byte vectors (itx_textpack.h says why and how); the bytes come from itx_loci_write
//   hard > 0: nothing is handed out, the caller writes the file on the host (the bed route's contract).
// The passes are enqueued by itx_sort_run (itx_radixsort.h); the text leaves through itx_copy_out (itx_devbuf.h).
//
// Integer and byte work, two double divisions per line; no kernel uses scratch (DESIGN.md has the figures).
#include "itx_devbuf.h"
#include "itx_textpack.h"
#include "itx_radixsort.h"
#include "itx_lociline.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

typedef unsigned long long ull;

#define LO_TILE 256u                 // sorted places per workgroup
#define LO_LDS 32768u                // bytes staged at a time: a tile of ordinary lines (256 x 60-90 bytes) in one window
#define LO_MAX_CHROM (1u << 19)      // rank << 13 stays inside 32 bits
#define LO_MAX_ROWS 0xfffffffeull
#define LO_CANARY 0xA5

// the table as the kernels read it: a row is two vectors {start, end, rep, cla} {fam, chromosome, 0, 0}; names: 0 chromosome, 1 repName,
// 2 repClass, 3 repFamily, name i = nb[t][no[t][i] .. no[t][i + 1])
struct LociTab {
    const uint4 *rows;
    const uint8_t *nb[4];
    const uint32_t *no[4];
};

__global__ __launch_bounds__(256) void k_loci_keys(const uint4 *__restrict__ rows, const uint32_t *__restrict__ rank, uint32_t n, uint2 *__restrict__ keys)
{
    const ull j = (ull)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t row = n - 1u - (uint32_t)j;
    const uint4 a = rows[2u * (size_t)row], b = rows[2u * (size_t)row + 1u];
    keys[j] = make_uint2(itx_loci_key(rank[b.y], itx_loci_bin((int)a.x, (int)a.y)), row);
}

// the numbers of the line of `row`; false: the line is not printed (then nothing else of L is set). The names follow in loci_names.
template <int KIND>
__device__ __forceinline__ bool loci_numbers(const uint4 a, uint32_t row, const void *__restrict__ cnt, const double *__restrict__ tot, ull reads_num, int thr_i,
                                             double thr_d, ItxLociLine *L)
{
    if (KIND == ITX_LOCI_FILTER) {
        const uint32_t c = static_cast<const uint32_t *>(cnt)[row];
        if ((int)c < thr_i) return false;                               // generic.c:1725
        itx_loci_filter_numbers(L, a.x, a.y, c, reads_num);
    } else {
        const double t = tot[row];
        if (!(t > thr_d)) return false;                                 // generic.c:1763
        itx_loci_cpg_numbers(L, a.x, a.y, static_cast<const int *>(cnt)[row], t);
    }
    return true;
}

__device__ __forceinline__ void loci_names(const LociTab &T, const uint4 a, const uint4 b, ItxLociLine *L)
{
    const uint32_t c0 = T.no[0][b.y], r0 = T.no[1][a.z], k0 = T.no[2][a.w], f0 = T.no[3][b.x];
    L->chr = T.nb[0] + c0;
    L->chr_len = T.no[0][b.y + 1u] - c0;
    L->rep = T.nb[1] + r0;
    L->rep_len = T.no[1][a.z + 1u] - r0;
    L->cla = T.nb[2] + k0;
    L->cla_len = T.no[2][a.w + 1u] - k0;
    L->fam = T.nb[3] + f0;
    L->fam_len = T.no[3][b.x + 1u] - f0;
}

template <int KIND>
__global__ __launch_bounds__(LO_TILE) void k_loci_measure(const LociTab T, const uint2 *__restrict__ order, uint32_t n, const void *__restrict__ cnt,
                                                           const double *__restrict__ tot_in, ull reads_num, int thr_i, double thr_d, uint32_t *__restrict__ len_out,
                                                           ull *__restrict__ tile_sum, ull *__restrict__ tot)
{
    __shared__ ull s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const ull j = (ull)blockIdx.x * LO_TILE + threadIdx.x;
    bool hard = false;
    if (j < n) {
        const uint32_t row = order[j].y;
        const uint4 a = T.rows[2u * (size_t)row], b = T.rows[2u * (size_t)row + 1u];
        ItxLociLine L;
        uint32_t len = 0;
        if (loci_numbers<KIND>(a, row, cnt, tot_in, reads_num, thr_i, thr_d, &L)) {
            hard = itx_loci_hard(&L);
            if (!hard) {
                loci_names(T, a, b, &L);
                len = itx_loci_len(&L);
            }
            atomicAdd(&s_sum[0], (ull)len);
            atomicAdd(&s_sum[1], 1ull);
        }
        len_out[j] = len;
    }
    const ull hardm = __ballot(hard);
    if ((threadIdx.x & 63u) == 0 && hardm) atomicAdd(&tot[2], (ull)__popcll(hardm));
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

template <int KIND>
__global__ __launch_bounds__(LO_TILE) void k_loci_write(const LociTab T, const uint2 *__restrict__ order, uint32_t n, const void *__restrict__ cnt,
                                                         const double *__restrict__ tot_in, ull reads_num, int thr_i, double thr_d, const uint32_t *__restrict__ len_in,
                                                         const ull *__restrict__ tile_base, uint8_t *__restrict__ text)
{
    __shared__ uint4 s_buf[LO_LDS / 16u];
    __shared__ uint32_t s_w[LO_TILE / 64u];
    const ull j = (ull)blockIdx.x * LO_TILE + threadIdx.x;
    const uint32_t len = j < n ? len_in[j] : 0u;                        // 0: not printed (a line has 18 bytes and more)
    ItxLociLine L;
    L.kind = KIND;
    L.chr = L.rep = L.cla = L.fam = T.nb[0];
    L.chr_len = L.rep_len = L.cla_len = L.fam_len = 0;
    L.start = L.end = L.length = L.count = 0;
    L.a = L.b = 0.0;
    if (len) {
        const uint32_t row = order[j].y;
        const uint4 a = T.rows[2u * (size_t)row], b = T.rows[2u * (size_t)row + 1u];
        (void)loci_numbers<KIND>(a, row, cnt, tot_in, reads_num, thr_i, thr_d, &L);
        loci_names(T, a, b, &L);
    }
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<LO_TILE>(len, s_w, &total);
    const ull tb = tile_base[2u * blockIdx.x], te = tb + total;
    const ull mb = tb + moff, me = mb + len;
    itx_pack_tile<LO_TILE, LO_LDS>(s_buf, text, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) { itx_loci_write(&L, dst, from, to); });
}

// ---- host side
struct itx_loci {
    int device, kind;
    size_t n;                        // rows
    uint32_t n_chrom, passes;
    hipStream_t st;
    hipEvent_t ev[6];                // sort: 0 .. 1; measure + scan: 2 .. 3; write: 4 .. 5
    uint4 *d_rows;
    uint32_t *d_rank;
    uint8_t *d_nb[4];
    uint32_t *d_no[4];
    uint2 *d_key[2];
    int cur;                         // d_key[cur] is the sorted order
    uint32_t *d_hist, *d_len;
    void *d_cnt;
    double *d_total;
    ull *d_tsum, *d_tbase, *d_tot, *h_tot;
    uint8_t *d_text;
    size_t d_text_cap;
    uint8_t *h_pin[2];               // the page-locked pair the text leaves through
    char *text;
    double sort_ms;
    int sort_read;
};

// a device allocation that may not fit: ITX_E_NOMEM, the caller keeps the host route
#define LO_ALLOC(ptr, bytes)                                                                           \
    do {                                                                                               \
        if (hipMalloc((void **)&(ptr), (bytes)) != hipSuccess) {                                       \
            (void)hipGetLastError();                                                                   \
            (ptr) = nullptr;                                                                           \
            itx_set_error("itx_loci: no device memory for %zu bytes; ITX_HOST_LOCI=1 writes the file on the host", (size_t)(bytes)); \
            rc = ITX_E_NOMEM;                                                                          \
            goto out;                                                                                  \
        }                                                                                              \
    } while (0)

extern "C" void itx_loci_destroy(itx_loci *lo)
{
    if (!lo) return;
    (void)hipSetDevice(lo->device);
    if (lo->st) (void)hipStreamSynchronize(lo->st);
    for (auto &e : lo->ev)
        if (e) (void)hipEventDestroy(e);
    if (lo->st) (void)hipStreamDestroy(lo->st);
    (void)hipFree(lo->d_rows);
    (void)hipFree(lo->d_rank);
    for (int t = 0; t < 4; t++) {
        (void)hipFree(lo->d_nb[t]);
        (void)hipFree(lo->d_no[t]);
    }
    (void)hipFree(lo->d_key[0]);
    (void)hipFree(lo->d_key[1]);
    (void)hipFree(lo->d_hist);
    (void)hipFree(lo->d_len);
    (void)hipFree(lo->d_cnt);
    (void)hipFree(lo->d_total);
    (void)hipFree(lo->d_tsum);
    (void)hipFree(lo->d_tbase);
    (void)hipFree(lo->d_tot);
    (void)hipFree(lo->d_text);
    if (lo->h_tot) (void)hipHostFree(lo->h_tot);
    for (auto &p : lo->h_pin)
        if (p) (void)hipHostFree(p);
    free(lo->text);
    delete lo;
}

// name i = bytes[off[i] .. off[i + 1]): ascending offsets, a table of less than 2^31 bytes; the offsets as the device reads them
static bool lo_names_ok(const char *bytes, const uint64_t *off, uint32_t n, std::vector<uint32_t> *o32)
{
    o32->assign((size_t)n + 1, 0u);
    if (!n) return true;
    if (!off) return false;
    for (uint32_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    if (off[n] - off[0] >= 0x80000000ull || (off[n] != off[0] && !bytes)) return false;
    for (uint32_t i = 0; i <= n; i++) (*o32)[i] = (uint32_t)(off[i] - off[0]);
    return true;
}

extern "C" int itx_loci_create(int device, int kind, const itx_row *rows, const uint32_t *row_chrom, size_t n_rows, const uint32_t *chrom_rank, uint32_t n_chrom,
                               const char *chrom_bytes, const uint64_t *chrom_off, const char *rep_bytes, const uint64_t *rep_off, uint32_t n_rep,
                               const char *cla_bytes, const uint64_t *cla_off, uint32_t n_cla, const char *fam_bytes, const uint64_t *fam_off, uint32_t n_fam,
                               itx_loci **out)
{
    if (out) *out = nullptr;
    if (!out || (kind != ITX_LOCI_FILTER && kind != ITX_LOCI_CPG) || (n_rows && (!rows || !row_chrom)) || (n_chrom && (!chrom_rank || !chrom_off)) ||
        (n_rep && !rep_off) || (n_cla && !cla_off) || (n_fam && !fam_off)) {
        itx_set_error("itx_loci_create: bad argument");
        return ITX_E_ARG;
    }
    if (n_chrom >= LO_MAX_CHROM || (ull)n_rows > LO_MAX_ROWS) {
        itx_set_error("itx_loci_create: %u chromosomes, %zu rows: the sort key holds 2^19 - 1 chromosomes and the order 2^32 - 2 rows", n_chrom, n_rows);
        return ITX_E_RANGE;
    }
    const char *nbytes[4] = {chrom_bytes, rep_bytes, cla_bytes, fam_bytes};
    const uint64_t *noff[4] = {chrom_off, rep_off, cla_off, fam_off};
    const uint32_t nn[4] = {n_chrom, n_rep, n_cla, n_fam};
    std::vector<uint32_t> o32[4];
    for (int t = 0; t < 4; t++)
        if (!lo_names_ok(nbytes[t], noff[t], nn[t], &o32[t])) {
            itx_set_error("itx_loci_create: name table %d: the offsets do not ascend, or it has 2^31 bytes and more", t);
            return ITX_E_ARG;
        }
    for (uint32_t c = 0; c < n_chrom; c++)
        if (chrom_rank[c] >= n_chrom) {
            itx_set_error("itx_loci_create: chrom_rank[%u] = %u with %u chromosomes", c, chrom_rank[c], n_chrom);
            return ITX_E_ARG;
        }
    std::vector<uint4> packed(2 * n_rows);
    for (size_t r = 0; r < n_rows; r++) {
        const itx_row *w = &rows[r];
        if (row_chrom[r] >= n_chrom || w->rep >= n_rep || w->cla >= n_cla || w->fam >= n_fam) {
            itx_set_error("itx_loci_create: row %zu names a chromosome, repName, repClass or repFamily the tables do not have", r);
            return ITX_E_ARG;
        }
        if (!itx_loci_bin_fits(itx_loci_bin((int)w->start, (int)w->end))) {
            itx_set_error("itx_loci_create: row %zu (%u %u) lies in a bin the sort key does not hold; ITX_HOST_LOCI=1 writes the file on the host", r, w->start, w->end);
            return ITX_E_RANGE;
        }
        packed[2 * r] = make_uint4(w->start, w->end, w->rep, w->cla);
        packed[2 * r + 1] = make_uint4(w->fam, row_chrom[r], 0u, 0u);
    }

    int rc = ITX_OK;
    itx_loci *lo = new itx_loci();
    lo->device = device;
    lo->kind = kind;
    lo->n = n_rows;
    lo->n_chrom = n_chrom;
    const uint32_t n = (uint32_t)n_rows, nt = (uint32_t)((n_rows + LO_TILE - 1) / LO_TILE);
    uint32_t bits = 0;
    while ((1u << bits) < n_chrom) bits++;
    lo->passes = (ITX_LOCI_BIN_BITS + bits + 7u) / 8u;
    ITX_TRY(hipSetDevice(device));
    LO_ALLOC(lo->d_rows, 32 * (n_rows + 1));
    LO_ALLOC(lo->d_rank, 4 * ((size_t)n_chrom + 1));
    for (int t = 0; t < 4; t++) {
        LO_ALLOC(lo->d_nb[t], (size_t)o32[t][nn[t]] + 16);
        LO_ALLOC(lo->d_no[t], 4 * ((size_t)nn[t] + 1));
    }
    LO_ALLOC(lo->d_key[0], 8 * (n_rows + 1));
    LO_ALLOC(lo->d_key[1], 8 * (n_rows + 1));
    LO_ALLOC(lo->d_hist, itx_sort_hist_bytes(n_rows) + 1024);
    LO_ALLOC(lo->d_len, 4 * (n_rows + 1));
    LO_ALLOC(lo->d_cnt, 4 * (n_rows + 1));
    if (kind == ITX_LOCI_CPG) LO_ALLOC(lo->d_total, 8 * (n_rows + 1));
    LO_ALLOC(lo->d_tsum, 16 * ((size_t)nt + 1));
    LO_ALLOC(lo->d_tbase, 16 * ((size_t)nt + 1));
    LO_ALLOC(lo->d_tot, 32);
    ITX_TRY(hipHostMalloc((void **)&lo->h_tot, 32, hipHostMallocDefault));
    ITX_TRY(hipStreamCreateWithFlags(&lo->st, hipStreamNonBlocking));
    for (auto &e : lo->ev) ITX_TRY(hipEventCreate(&e));
    if (n_rows) ITX_TRY(hipMemcpyAsync(lo->d_rows, packed.data(), 32 * n_rows, hipMemcpyHostToDevice, lo->st));
    if (n_chrom) ITX_TRY(hipMemcpyAsync(lo->d_rank, chrom_rank, 4 * (size_t)n_chrom, hipMemcpyHostToDevice, lo->st));
    for (int t = 0; t < 4; t++) {
        if (o32[t][nn[t]]) ITX_TRY(hipMemcpyAsync(lo->d_nb[t], nbytes[t] + noff[t][0], o32[t][nn[t]], hipMemcpyHostToDevice, lo->st));
        ITX_TRY(hipMemcpyAsync(lo->d_no[t], o32[t].data(), 4 * ((size_t)nn[t] + 1), hipMemcpyHostToDevice, lo->st));
    }
    ITX_TRY(hipStreamSynchronize(lo->st));                                 // the caller's arrays (and packed, o32) are free again
    ITX_TRY(hipEventRecord(lo->ev[0], lo->st));
    if (n) {
        hipLaunchKernelGGL(k_loci_keys, dim3(nt), dim3(256), 0, lo->st, lo->d_rows, lo->d_rank, n, lo->d_key[0]);
        ITX_TRY(hipGetLastError());
        uint2 *sorted = nullptr;
        if ((rc = itx_sort_run(lo->st, lo->d_key[0], lo->d_key[1], n, 0u, lo->passes, lo->d_hist, &sorted)) != ITX_OK) goto out;
        lo->cur = sorted == lo->d_key[1];
    }
    ITX_TRY(hipEventRecord(lo->ev[1], lo->st));                            // not waited for: the sort runs beside the caller's stream
out:
    if (rc != ITX_OK) {
        itx_loci_destroy(lo);
        return rc;
    }
    *out = lo;
    return ITX_OK;
}

// after the stream has been waited for
static void lo_read_sort_time(itx_loci *lo)
{
    float ms = 0;
    if (!lo->sort_read && hipEventElapsedTime(&ms, lo->ev[0], lo->ev[1]) == hipSuccess) lo->sort_ms = (double)ms;
    lo->sort_read = 1;
}

extern "C" int itx_loci_order(itx_loci *lo, uint32_t *order, double *sort_ms)
{
    if (!lo || (lo->n && !order)) {
        itx_set_error("itx_loci_order: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    std::vector<uint2> k(lo->n);
    ITX_TRY(hipSetDevice(lo->device));
    ITX_TRY(hipStreamSynchronize(lo->st));
    lo_read_sort_time(lo);
    if (lo->n) ITX_TRY(hipMemcpy(k.data(), lo->d_key[lo->cur], 8 * lo->n, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < lo->n; j++) order[j] = k[j].y;
    if (sort_ms) *sort_ms = lo->sort_ms;
out:
    return rc;
}

template <int KIND>
static int lo_text(itx_loci *lo, const void *cnt, const double *total, int thr_i, double thr_d, ull reads_num, itx_loci_text *res)
{
    int rc = ITX_OK;
    const uint32_t n = (uint32_t)lo->n, nt = (uint32_t)((lo->n + LO_TILE - 1) / LO_TILE);
    LociTab T;
    ull bytes = 0;
    size_t cap = 0;
    float ms = 0, ms2 = 0;
    char *text = nullptr;
    T.rows = lo->d_rows;
    for (int t = 0; t < 4; t++) {
        T.nb[t] = lo->d_nb[t];
        T.no[t] = lo->d_no[t];
    }
    memset(res, 0, sizeof *res);
    ITX_TRY(hipSetDevice(lo->device));
    if (n) {
        ITX_TRY(hipMemcpyAsync(lo->d_cnt, cnt, 4 * lo->n, hipMemcpyHostToDevice, lo->st));
        if (KIND == ITX_LOCI_CPG) ITX_TRY(hipMemcpyAsync(lo->d_total, total, 8 * lo->n, hipMemcpyHostToDevice, lo->st));
    }
    ITX_TRY(hipMemsetAsync(lo->d_tot, 0, 32, lo->st));
    ITX_TRY(hipEventRecord(lo->ev[2], lo->st));
    if (n) {
        hipLaunchKernelGGL(k_loci_measure<KIND>, dim3(nt), dim3(LO_TILE), 0, lo->st, T, lo->d_key[lo->cur], n, lo->d_cnt, lo->d_total, reads_num, thr_i, thr_d,
                           lo->d_len, lo->d_tsum, lo->d_tot);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, lo->st, lo->d_tsum, nt, lo->d_tbase, lo->d_tot);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipEventRecord(lo->ev[3], lo->st));
    ITX_TRY(hipMemcpyAsync(lo->h_tot, lo->d_tot, 32, hipMemcpyDeviceToHost, lo->st));
    ITX_TRY(hipStreamSynchronize(lo->st));                                 // (the sort of create is through as well)
    lo_read_sort_time(lo);
    ITX_TRY(hipEventElapsedTime(&ms, lo->ev[2], lo->ev[3]));
    res->sort_ms = lo->sort_ms;
    res->text_ms = (double)ms;
    res->lines = lo->h_tot[1];
    res->hard = lo->h_tot[2];
    if (res->hard) goto out;                                              // the host has to look: nothing is handed out
    bytes = lo->h_tot[0];
    cap = (size_t)((bytes + 15ull) & ~15ull) + 64;
    if (cap > lo->d_text_cap) {
        (void)hipFree(lo->d_text);
        lo->d_text = nullptr;
        lo->d_text_cap = 0;
        LO_ALLOC(lo->d_text, cap);
        lo->d_text_cap = cap;
    }
    text = (char *)malloc(cap);
    if (!text) {
        itx_set_error("itx_loci: no host memory for %zu bytes of text", cap);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipMemsetAsync(lo->d_text + bytes, LO_CANARY, cap - (size_t)bytes, lo->st));
    ITX_TRY(hipEventRecord(lo->ev[4], lo->st));
    if (bytes) {
        hipLaunchKernelGGL(k_loci_write<KIND>, dim3(nt), dim3(LO_TILE), 0, lo->st, T, lo->d_key[lo->cur], n, lo->d_cnt, lo->d_total, reads_num, thr_i, thr_d,
                           lo->d_len, lo->d_tbase, lo->d_text);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipEventRecord(lo->ev[5], lo->st));
    if ((rc = itx_copy_out(lo->st, lo->h_pin, text, lo->d_text, cap)) != ITX_OK) goto out;
    ITX_TRY(hipEventElapsedTime(&ms2, lo->ev[4], lo->ev[5]));
    res->text_ms += (double)ms2;
    free(lo->text);
    lo->text = text;
    text = nullptr;
    res->text = lo->text;
    res->bytes = bytes;
    res->capacity = cap;
out:
    if (rc != ITX_OK && lo->st) (void)hipStreamSynchronize(lo->st);
    free(text);
    return rc;
}

extern "C" int itx_loci_filter_text(itx_loci *lo, const uint32_t *locus_cnt, int threshold, unsigned long long reads_num, itx_loci_text *out)
{
    if (!lo || !out || lo->kind != ITX_LOCI_FILTER || (lo->n && !locus_cnt)) {
        itx_set_error("itx_loci_filter_text: bad argument%s", lo && lo->kind != ITX_LOCI_FILTER ? " (the object was created for cpgfilter)" : "");
        return ITX_E_ARG;
    }
    return lo_text<ITX_LOCI_FILTER>(lo, locus_cnt, nullptr, threshold, 0.0, reads_num, out);
}

extern "C" int itx_loci_cpg_text(itx_loci *lo, const int *cpg_count, const double *cpg_total, double threshold, itx_loci_text *out)
{
    if (!lo || !out || lo->kind != ITX_LOCI_CPG || (lo->n && (!cpg_count || !cpg_total))) {
        itx_set_error("itx_loci_cpg_text: bad argument%s", lo && lo->kind != ITX_LOCI_CPG ? " (the object was created for filter)" : "");
        return ITX_E_ARG;
    }
    return lo_text<ITX_LOCI_CPG>(lo, cpg_count, cpg_total, 0, threshold, 0ull, out);
}
