// itx_names.hip — the read lists of `iteres filter -r` (generic.c:662-666, written by writeFilterOut generic.c:1729-1731) built
// where the records lie: per table row the names of the records that chose it, in file order, joined with ','. The host used to
// fetch the inflated bytes of every batch, parse each record a second time for its name (one strdup each) and concatenate the
// lists on one thread at the end; here a batch leaves (row, name) entries in a pool in HBM and the end of the stream is a sort.
//
// per batch (records in device memory, the chosen rows in d_hit_row):
//   k_names_measure  one lane per record: a record with hit_row >= 0 gets itx_bed_scan (itx_bedline.h: the name is the bytes up to
//                    the first NUL; no NUL inside the record is `hard`). A tile of NM_TILE records adds up its entries and its
//                    name bytes (64 bit).
//   k_tile_scan2     (itx_textpack.h) exclusive sums over the tiles, one workgroup; the two totals are all the host waits for.
//   k_names_gather   one workgroup per tile: every hit appends {row, len, pool offset}; the tile's names are ONE contiguous range
//                    of the pool, staged in LDS a window at a time and stored with 16-byte vectors (itx_textpack.h says why and how).
//   n_hard > 0: nothing of the batch is appended, the caller takes the host route (the bed route's contract). The host route
//   hands its hits to the same pool (itx_names_append_host), so the stream is one ordered list whatever route a window took.
//
// end of stream (itx_names_finish):
//   (row, entry index) pairs, LSD radix sort by row in ceil(log2(n_rows) / 8) passes of 8 bits between two buffers of 8 bytes
//   per entry: k_sort_hist (per-workgroup digit counts), k_sort_scan (one workgroup, digit-major so that the scan IS the global
//   order), k_sort_scatter (ranks inside a wave by ballot match: equal digits keep their order, so entries of a row stay in
//   append order). Then len + 1 per sorted entry, scanned in 64 bits: each name's place in the text, every name followed by ','
//   and the last of its row by NUL; the first of a row writes row_off[row]. k_names_write copies pool -> text like the gather.
//
// The host half enqueues with the shared plumbing: the passes are itx_sort_run's (itx_radixsort.h), the pool's growth and the way
// the results leave are itx_devbuf.h's.
//
// Byte and integer work; the sort's scatter moves the most bytes. No kernel uses scratch (DESIGN.md has the figures).
#include "itx_devbuf.h"
#include "itx_textpack.h"
#include "itx_radixsort.h"
#include "itx_bedline.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

typedef unsigned long long ull;

#define NM_TILE 256u                 // records (gather) / sorted entries (write) per workgroup
#define NM_LDS 16384u                // bytes staged at a time: a tile of ordinary names (256 x 20-40 bytes) in one window
#define NM_NOHIT 0xffffffffu
#define NM_MAX_ENTRIES 0xfffffffeull

struct NameEnt {                     // 16 bytes, stored as one vector
    uint32_t row, len;
    ull off;
};

__global__ __launch_bounds__(NM_TILE) void k_names_measure(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, const int32_t *__restrict__ hit_row,
                                                            uint32_t n, uint32_t *__restrict__ len_out, ull *__restrict__ tile_sum, ull *__restrict__ tot)
{
    __shared__ ull s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * NM_TILE + threadIdx.x;
    bool hard = false;
    if (i < n) {
        uint32_t len = NM_NOHIT;
        if (hit_row[i] >= 0) {
            const ItxBedScan sc = itx_bed_scan(u + rec_off[i], false);
            hard = sc.hard;
            len = sc.qname_len;
            atomicAdd(&s_sum[0], 1ull);
            atomicAdd(&s_sum[1], (ull)len);
        }
        len_out[i] = len;
    }
    const ull hardm = __ballot(hard);
    if ((threadIdx.x & 63u) == 0 && hardm) atomicAdd(&tot[2], (ull)__popcll(hardm));
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

__global__ __launch_bounds__(NM_TILE) void k_names_gather(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, const int32_t *__restrict__ hit_row, uint32_t n,
                                                           const uint32_t *__restrict__ len_in, const ull *__restrict__ tile_base, ull ent_base, ull pool_base,
                                                           NameEnt *__restrict__ ent, uint8_t *__restrict__ pool)
{
    __shared__ uint4 s_buf[NM_LDS / 16u];
    __shared__ uint32_t s_w[NM_TILE / 64u], s_c[NM_TILE / 64u];
    const uint32_t i = blockIdx.x * NM_TILE + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t l0 = i < n ? len_in[i] : NM_NOHIT;
    const bool hit = l0 != NM_NOHIT;
    const uint32_t len = hit ? l0 : 0u;
    const ull hm = __ballot(hit);
    if (lane == 0) s_c[w] = (uint32_t)__popcll(hm);
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<NM_TILE>(len, s_w, &total);  // (its barrier covers s_c)
    uint32_t rank = (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < w; k++) rank += s_c[k];
    const ull tb = pool_base + tile_base[2u * blockIdx.x + 1u], te = tb + total;
    const ull mb = tb + moff, me = mb + len;
    const uint8_t *src = hit ? u + rec_off[i] + 36 : u;
    if (hit) {
        const ull k = ent_base + tile_base[2u * blockIdx.x] + rank;
        *reinterpret_cast<uint4 *>(&ent[k]) = make_uint4((uint32_t)hit_row[i], len, (uint32_t)mb, (uint32_t)(mb >> 32));
    }
    itx_pack_tile<NM_TILE, NM_LDS>(s_buf, pool, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) {
        // 20-40 bytes at any alignment: kept a byte loop (the vectoriser would make unaligned 8-byte loads and 16-byte LDS stores of it)
#pragma clang loop vectorize(disable)
        for (uint32_t k = from; k < to; k++) dst[k - from] = src[k];
    });
}

// ---- the sort
__global__ __launch_bounds__(256) void k_sort_init(const NameEnt *__restrict__ ent, uint32_t n, uint32_t n_rows, uint2 *__restrict__ keys, ull *__restrict__ bad)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t row = ent[j].row;
    if (row >= n_rows) atomicAdd(bad, 1ull);
    keys[j] = make_uint2(row, j);
}

// (k_sort_hist, k_sort_scan, k_sort_scatter: itx_radixsort.h)

// ---- the text
__global__ __launch_bounds__(NM_TILE) void k_text_measure(const uint2 *__restrict__ keys, const NameEnt *__restrict__ ent, uint32_t n, ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_w[NM_TILE / 64u];
    const ull j = (ull)blockIdx.x * NM_TILE + threadIdx.x;
    uint32_t total = 0;
    (void)itx_tile_offsets<NM_TILE>(j < n ? ent[keys[j].y].len + 1u : 0u, s_w, &total);
    if (threadIdx.x == 0) {
        tile_sum[2u * blockIdx.x] = total;
        tile_sum[2u * blockIdx.x + 1u] = 0;
    }
}

__global__ __launch_bounds__(NM_TILE) void k_names_write(const uint2 *__restrict__ keys, const NameEnt *__restrict__ ent, uint32_t n, const ull *__restrict__ tile_base,
                                                          const uint8_t *__restrict__ pool, uint8_t *__restrict__ text, ull *__restrict__ row_off, uint32_t *__restrict__ row_cnt,
                                                          uint32_t n_rows)
{
    __shared__ uint4 s_buf[NM_LDS / 16u];
    __shared__ uint32_t s_w[NM_TILE / 64u];
    const ull j = (ull)blockIdx.x * NM_TILE + threadIdx.x;
    const bool valid = j < n;
    uint2 key = make_uint2(0u, 0u);
    NameEnt e = {0u, 0u, 0ull};
    if (valid) {
        key = keys[j];
        const uint4 q = *reinterpret_cast<const uint4 *>(&ent[key.y]);
        e.row = q.x;
        e.len = q.y;
        e.off = (ull)q.z | (ull)q.w << 32;
    }
    const uint32_t l1 = valid ? e.len + 1u : 0u;
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<NM_TILE>(l1, s_w, &total);
    const ull tb = tile_base[2u * blockIdx.x], te = tb + total;
    const ull mb = tb + moff, me = mb + l1;
    uint8_t term = 0;
    if (valid) {
        if (j + 1 < n && keys[j + 1].x == key.x) term = ',';
        if (key.x < n_rows) {
            if (j == 0 || keys[j - 1].x != key.x) row_off[key.x] = mb;
            atomicAdd(&row_cnt[key.x], 1u);
        }
    }
    const uint8_t *src = pool + e.off;
    const uint32_t len = e.len;
    itx_pack_tile<NM_TILE, NM_LDS>(s_buf, text, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) {
        for (uint32_t k = from; k < to; k++) dst[k - from] = k < len ? src[k] : term;
    });
}

// ---- host side
struct itx_names {
    int device;
    size_t cap;                      // records per batch
    hipStream_t st;
    hipEvent_t ev[5];                // measure: 0 .. 1, gather: 2 .. 3; 4: the caller's stream
    int gather_timed;                // ev[2], ev[3] are recorded and not yet read
    int32_t *d_hits;
    uint32_t *d_len;
    ull *d_tile_sum, *d_tile_base, *d_tot, *h_tot;
    uint8_t *d_pool;
    NameEnt *d_ent;
    size_t pool_cap, pool_used, ent_cap, n_ent;
    int finished;
    uint8_t *h_pin[2];               // the page-locked pair the results leave through
    char *text;
    uint64_t *row_off;
    uint32_t *row_cnt;
    itx_names_stats stats;
};

extern "C" void itx_names_destroy(itx_names *nm)
{
    if (!nm) return;
    (void)hipSetDevice(nm->device);
    if (nm->st) (void)hipStreamSynchronize(nm->st);
    for (auto &e : nm->ev)
        if (e) (void)hipEventDestroy(e);
    if (nm->st) (void)hipStreamDestroy(nm->st);
    (void)hipFree(nm->d_hits);
    (void)hipFree(nm->d_len);
    (void)hipFree(nm->d_tile_sum);
    (void)hipFree(nm->d_tile_base);
    (void)hipFree(nm->d_tot);
    (void)hipFree(nm->d_pool);
    (void)hipFree(nm->d_ent);
    if (nm->h_tot) (void)hipHostFree(nm->h_tot);
    for (auto &p : nm->h_pin)
        if (p) (void)hipHostFree(p);
    free(nm->text);
    free(nm->row_off);
    free(nm->row_cnt);
    delete nm;
}

extern "C" int itx_names_create(int device, size_t batch_capacity, size_t pool_bytes, itx_names **out)
{
    if (!out || batch_capacity == 0 || batch_capacity > 0xffffff00u) {
        itx_set_error("itx_names_create: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    int rc = ITX_OK;
    itx_names *nm = new itx_names();
    nm->device = device;
    nm->cap = batch_capacity;
    const size_t n = batch_capacity + 64, nt = (batch_capacity + NM_TILE - 1) / NM_TILE + 1;
    if (!pool_bytes) {
        const char *e = getenv("ITX_NAMES_POOL_BYTES");
        pool_bytes = e && atoll(e) > 0 ? (size_t)atoll(e) : (size_t)64 << 20;
    }
    if (pool_bytes < 256) pool_bytes = 256;
    ITX_TRY(hipSetDevice(device));
    ITX_TRY(hipMalloc((void **)&nm->d_hits, 4 * n));
    ITX_TRY(hipMalloc((void **)&nm->d_len, 4 * n));
    ITX_TRY(hipMalloc((void **)&nm->d_tile_sum, 16 * nt));
    ITX_TRY(hipMalloc((void **)&nm->d_tile_base, 16 * nt));
    ITX_TRY(hipMalloc((void **)&nm->d_tot, 32));
    ITX_TRY(hipHostMalloc((void **)&nm->h_tot, 32, hipHostMallocDefault));
    nm->pool_cap = pool_bytes;
    nm->ent_cap = pool_bytes / 32 + 16;
    ITX_TRY(hipMalloc((void **)&nm->d_pool, nm->pool_cap + 16));
    ITX_TRY(hipMalloc((void **)&nm->d_ent, sizeof(NameEnt) * nm->ent_cap));
    ITX_TRY(hipStreamCreateWithFlags(&nm->st, hipStreamNonBlocking));
    for (auto &e : nm->ev) ITX_TRY(hipEventCreate(&e));
out:
    if (rc != ITX_OK) {
        itx_names_destroy(nm);
        return rc;
    }
    *out = nm;
    return ITX_OK;
}

extern "C" int32_t *itx_names_hits(itx_names *nm) { return nm ? nm->d_hits : nullptr; }
extern "C" void *itx_names_stream(itx_names *nm) { return nm ? (void *)nm->st : nullptr; }

// room for add_ent more entries and add_bytes more name bytes; nm->st is idle when this is called. The limits are checked here,
// before anything is written: what does not fit leaves the object as it was.
static int names_grow(itx_names *nm, ull add_ent, ull add_bytes)
{
    size_t want_pool = 0, want_ent = 0;
    if ((ull)nm->n_ent + add_ent > NM_MAX_ENTRIES) {
        itx_set_error("itx_names: more than 2^32 - 2 names in one run; ITX_HOST_NAMES=1 builds the lists on the host");
        return ITX_E_NOMEM;
    }
    if (nm->pool_used + add_bytes > nm->pool_cap) {
        want_pool = (size_t)(nm->pool_used + add_bytes);
        want_pool = want_pool + (want_pool > 2 * nm->pool_cap ? want_pool / 4 : want_pool);       // at least twice what there was
    }
    if (nm->n_ent + add_ent > nm->ent_cap) {
        want_ent = (size_t)(nm->n_ent + add_ent);
        want_ent = want_ent + (want_ent > 2 * nm->ent_cap ? want_ent / 4 : want_ent);
        if (want_ent > NM_MAX_ENTRIES) want_ent = (size_t)NM_MAX_ENTRIES;
    }
    // the pool and the entries are taken together (itx_devbuf.h); what they hold is kept
    ItxGrow g[2] = {{(void **)&nm->d_pool, nm->pool_used, want_pool ? want_pool + 16 : 0}, {(void **)&nm->d_ent, sizeof(NameEnt) * nm->n_ent, sizeof(NameEnt) * want_ent}};
    const int bad = itx_grow_alloc(g, 2);
    if (bad == 0) itx_set_error("itx_names: no device memory for a pool of %zu bytes; ITX_HOST_NAMES=1 builds the lists on the host", want_pool);
    if (bad == 1) itx_set_error("itx_names: no device memory for %zu entries; ITX_HOST_NAMES=1 builds the lists on the host", want_ent);
    if (bad >= 0) return ITX_E_NOMEM;
    const int rc = itx_grow_commit(nm->st, g, 2);
    if (rc != ITX_OK) return rc;
    if (want_pool) {
        nm->pool_cap = want_pool;
        nm->stats.grows++;
    }
    if (want_ent) nm->ent_cap = want_ent;
    return ITX_OK;
}

static void names_read_gather_time(itx_names *nm)
{
    if (!nm->gather_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, nm->ev[2], nm->ev[3]) == hipSuccess) nm->stats.gather_ms += (double)ms;
    nm->gather_timed = 0;
}

// measure + scan (waited for: the two totals decide whether the pool has to grow), then the gather is enqueued
int itx_names_start(itx_names *nm, const uint8_t *u, const uint32_t *rec_off, const int32_t *d_hit_row, size_t n, void *stream, uint64_t *n_hard)
{
    if (!nm || !n_hard || (n && (!u || !rec_off || !d_hit_row))) {
        itx_set_error("itx_names: bad argument");
        return ITX_E_ARG;
    }
    if (n > nm->cap) {
        itx_set_error("itx_names: batch exceeds the capacity");
        return ITX_E_ARG;
    }
    if (nm->finished) {
        itx_set_error("itx_names: the lists are finished");
        return ITX_E_STATE;
    }
    *n_hard = 0;
    if (!n) return ITX_OK;
    int rc = ITX_OK;
    float ms = 0;
    const uint32_t nt = (uint32_t)((n + NM_TILE - 1) / NM_TILE);
    ITX_TRY(hipSetDevice(nm->device));
    if ((hipStream_t)stream != nm->st) {                                   // the chosen rows were left on another stream
        ITX_TRY(hipEventRecord(nm->ev[4], (hipStream_t)stream));
        ITX_TRY(hipStreamWaitEvent(nm->st, nm->ev[4], 0));
    }
    ITX_TRY(hipEventRecord(nm->ev[0], nm->st));
    ITX_TRY(hipMemsetAsync(nm->d_tot, 0, 32, nm->st));
    hipLaunchKernelGGL(k_names_measure, dim3(nt), dim3(NM_TILE), 0, nm->st, u, rec_off, d_hit_row, (uint32_t)n, nm->d_len, nm->d_tile_sum, nm->d_tot);
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, nm->st, nm->d_tile_sum, nt, nm->d_tile_base, nm->d_tot);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(nm->ev[1], nm->st));
    ITX_TRY(hipMemcpyAsync(nm->h_tot, nm->d_tot, 32, hipMemcpyDeviceToHost, nm->st));
    ITX_TRY(hipStreamSynchronize(nm->st));
    names_read_gather_time(nm);                                            // (the batch before this one)
    ITX_TRY(hipEventElapsedTime(&ms, nm->ev[0], nm->ev[1]));
    nm->stats.gather_ms += (double)ms;
    if (nm->h_tot[2]) {                                                    // the host has to look: nothing of this batch is appended
        *n_hard = nm->h_tot[2];
        nm->stats.hard_batches++;
        goto out;
    }
    if ((rc = names_grow(nm, nm->h_tot[0], nm->h_tot[1])) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(nm->ev[2], nm->st));
    if (nm->h_tot[0]) {
        hipLaunchKernelGGL(k_names_gather, dim3(nt), dim3(NM_TILE), 0, nm->st, u, rec_off, d_hit_row, (uint32_t)n, nm->d_len, nm->d_tile_base, (ull)nm->n_ent,
                           (ull)nm->pool_used, nm->d_ent, nm->d_pool);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipEventRecord(nm->ev[3], nm->st));
    nm->gather_timed = 1;
    nm->n_ent += (size_t)nm->h_tot[0];
    nm->pool_used += (size_t)nm->h_tot[1];
    nm->stats.batches++;
    nm->stats.entries += nm->h_tot[0];
    nm->stats.bytes += nm->h_tot[1];
out:
    return rc;
}

extern "C" int itx_names_run(itx_names *nm, const void *d_bytes, const uint32_t *d_rec_off, const int32_t *d_hit_row, size_t n, void *stream, uint64_t *n_hard)
{
    return itx_names_start(nm, (const uint8_t *)d_bytes, d_rec_off, d_hit_row, n, stream, n_hard);
}

extern "C" int itx_names_wait_kernels(itx_names *nm)
{
    if (!nm) {
        itx_set_error("itx_names_wait_kernels: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(nm->device));
    ITX_TRY(hipStreamSynchronize(nm->st));
    names_read_gather_time(nm);
out:
    return rc;
}

extern "C" int itx_names_append_host(itx_names *nm, const uint32_t *rows, const char *name_bytes, const uint64_t *name_off, size_t n)
{
    if (!nm || (n && (!rows || !name_off))) {
        itx_set_error("itx_names_append_host: bad argument");
        return ITX_E_ARG;
    }
    if (nm->finished) {
        itx_set_error("itx_names_append_host: the lists are finished");
        return ITX_E_STATE;
    }
    if (!n) return ITX_OK;
    for (size_t i = 0; i < n; i++)
        if (name_off[i + 1] < name_off[i] || name_off[i + 1] - name_off[i] > 0xffffffffull) {
            itx_set_error("itx_names_append_host: the offsets do not ascend");
            return ITX_E_ARG;
        }
    const uint64_t bytes = name_off[n] - name_off[0];
    if (bytes && !name_bytes) {
        itx_set_error("itx_names_append_host: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    std::vector<NameEnt> v(n);
    ITX_TRY(hipSetDevice(nm->device));
    ITX_TRY(hipStreamSynchronize(nm->st));                                  // device batches before this one have their place
    names_read_gather_time(nm);
    if ((rc = names_grow(nm, n, bytes)) != ITX_OK) goto out;
    for (size_t i = 0; i < n; i++) {
        v[i].row = rows[i];
        v[i].len = (uint32_t)(name_off[i + 1] - name_off[i]);
        v[i].off = (ull)nm->pool_used + (name_off[i] - name_off[0]);
    }
    ITX_TRY(hipMemcpyAsync(nm->d_ent + nm->n_ent, v.data(), sizeof(NameEnt) * n, hipMemcpyHostToDevice, nm->st));
    if (bytes) ITX_TRY(hipMemcpyAsync(nm->d_pool + nm->pool_used, name_bytes + name_off[0], bytes, hipMemcpyHostToDevice, nm->st));
    ITX_TRY(hipStreamSynchronize(nm->st));                                  // the caller's arrays are its own again
    nm->n_ent += n;
    nm->pool_used += (size_t)bytes;
    nm->stats.host_batches++;
    nm->stats.entries += n;
    nm->stats.bytes += bytes;
out:
    return rc;
}

extern "C" int itx_names_finish(itx_names *nm, size_t n_rows, itx_names_result *res)
{
    if (!nm || !res || n_rows == 0 || n_rows > 0xffffffffull) {
        itx_set_error("itx_names_finish: bad argument");
        return ITX_E_ARG;
    }
    if (nm->finished) {
        itx_set_error("itx_names_finish: called twice");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    const uint32_t n = (uint32_t)nm->n_ent, nt = (uint32_t)(((ull)n + NM_TILE - 1) / NM_TILE);
    uint32_t bits = 0;
    while (((ull)1 << bits) < (ull)n_rows) bits++;
    const uint32_t passes = (bits + 7u) / 8u;
    uint2 *d_key[2] = {nullptr, nullptr}, *sorted = nullptr;
    uint32_t *d_hist = nullptr, *d_cnt = nullptr;
    ull *d_tsum = nullptr, *d_tbase = nullptr, *d_off = nullptr;
    uint8_t *d_text = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ull total = 0;
    float ms = 0;
    char *text = nullptr;
    uint64_t *row_off = nullptr;
    uint32_t *row_cnt = nullptr;
    ITX_TRY(hipSetDevice(nm->device));
    ITX_TRY(hipStreamSynchronize(nm->st));
    names_read_gather_time(nm);
    ITX_TRY(hipEventCreate(&e0));
    ITX_TRY(hipEventCreate(&e1));
    row_off = (uint64_t *)malloc(sizeof(uint64_t) * n_rows);
    row_cnt = (uint32_t *)malloc(sizeof(uint32_t) * n_rows);
    if (!row_off || !row_cnt || hipMalloc((void **)&d_off, 8 * n_rows) != hipSuccess || hipMalloc((void **)&d_cnt, 4 * n_rows) != hipSuccess ||
        (n && (hipMalloc((void **)&d_key[0], 8 * (size_t)n) != hipSuccess || hipMalloc((void **)&d_key[1], 8 * (size_t)n) != hipSuccess ||
               hipMalloc((void **)&d_hist, itx_sort_hist_bytes(n)) != hipSuccess || hipMalloc((void **)&d_tsum, 16 * (size_t)nt) != hipSuccess ||
               hipMalloc((void **)&d_tbase, 16 * (size_t)nt) != hipSuccess))) {
        (void)hipGetLastError();
        itx_set_error("itx_names_finish: no memory to sort %u names over %zu rows; ITX_HOST_NAMES=1 builds the lists on the host", n, n_rows);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipEventRecord(e0, nm->st));
    ITX_TRY(hipMemsetAsync(d_off, 0xff, 8 * n_rows, nm->st));
    ITX_TRY(hipMemsetAsync(d_cnt, 0, 4 * n_rows, nm->st));
    if (n) {
        ITX_TRY(hipMemsetAsync(nm->d_tot, 0, 32, nm->st));
        hipLaunchKernelGGL(k_sort_init, dim3(nt), dim3(256), 0, nm->st, nm->d_ent, n, (uint32_t)n_rows, d_key[0], nm->d_tot + 2);
        ITX_TRY(hipGetLastError());
        if ((rc = itx_sort_run(nm->st, d_key[0], d_key[1], n, 0u, passes, d_hist, &sorted)) != ITX_OK) goto out;
        hipLaunchKernelGGL(k_text_measure, dim3(nt), dim3(NM_TILE), 0, nm->st, sorted, nm->d_ent, n, d_tsum);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, nm->st, d_tsum, nt, d_tbase, nm->d_tot);
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(nm->h_tot, nm->d_tot, 32, hipMemcpyDeviceToHost, nm->st));
        ITX_TRY(hipStreamSynchronize(nm->st));
        if (nm->h_tot[2]) {
            itx_set_error("itx_names_finish: %llu names sit on rows >= n_rows (%zu)", (unsigned long long)nm->h_tot[2], n_rows);
            rc = ITX_E_ARG;
            goto out;
        }
        total = nm->h_tot[0];
        if (hipMalloc((void **)&d_text, (size_t)total + 16) != hipSuccess) {
            (void)hipGetLastError();
            d_text = nullptr;
            itx_set_error("itx_names_finish: no device memory for %llu bytes of text; ITX_HOST_NAMES=1 builds the lists on the host", total);
            rc = ITX_E_NOMEM;
            goto out;
        }
        hipLaunchKernelGGL(k_names_write, dim3(nt), dim3(NM_TILE), 0, nm->st, sorted, nm->d_ent, n, d_tbase, nm->d_pool, d_text, d_off, d_cnt, (uint32_t)n_rows);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipEventRecord(e1, nm->st));
    text = (char *)malloc((size_t)total + 1);
    if (!text) {
        itx_set_error("itx_names_finish: no host memory for %llu bytes of text", total);
        rc = ITX_E_NOMEM;
        goto out;
    }
    text[total] = 0;
    if (total && (rc = itx_copy_out(nm->st, nm->h_pin, text, d_text, (size_t)total)) != ITX_OK) goto out;
    if ((rc = itx_copy_out(nm->st, nm->h_pin, row_off, d_off, 8 * n_rows)) != ITX_OK) goto out;
    if ((rc = itx_copy_out(nm->st, nm->h_pin, row_cnt, d_cnt, 4 * n_rows)) != ITX_OK) goto out;
    ITX_TRY(hipStreamSynchronize(nm->st));
    ITX_TRY(hipEventElapsedTime(&ms, e0, e1));
    nm->stats.finish_ms = (double)ms;
    nm->text = text;
    nm->row_off = row_off;
    nm->row_cnt = row_cnt;
    text = nullptr;
    row_off = nullptr;
    row_cnt = nullptr;
    nm->finished = 1;
    res->text = nm->text;
    res->text_bytes = total;
    res->row_off = nm->row_off;
    res->row_cnt = nm->row_cnt;
    res->n_entries = n;
out:
    if (rc != ITX_OK && nm->st) (void)hipStreamSynchronize(nm->st);       // nothing of this call still reads what is freed below
    (void)hipFree(d_key[0]);
    (void)hipFree(d_key[1]);
    (void)hipFree(d_hist);
    (void)hipFree(d_cnt);
    (void)hipFree(d_tsum);
    (void)hipFree(d_tbase);
    (void)hipFree(d_off);
    (void)hipFree(d_text);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    free(text);
    free(row_off);
    free(row_cnt);
    return rc;
}

extern "C" int itx_names_get_stats(const itx_names *nm, itx_names_stats *out)
{
    if (!nm || !out) {
        itx_set_error("itx_names_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *out = nm->stats;
    return ITX_OK;
}
