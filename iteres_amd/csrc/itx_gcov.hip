// itx_gcov.hip — the genome coverage of `iteres filter -G` (an extension: the reference writes no such file): the depth of the
// counted reads over the chromosomes of the size file, as bedGraph text, built where the records lie.
//
// Which records, which interval: a record that chose a row (hit_row >= 0, not ITX_F5_NOLOOKUP) adds 1 to every base of the
// [start, end) that itx_derive (itx_derive.h) gives for it — the interval the lookup ran on. For a counted record
// 0 <= start < end <= size - 1 holds; the kernels check it all the same, a record outside adds nothing and is counted.
//
// per batch:
//   k_gc_add       one lane per record: +1 at off[chrom] + start, -1 at off[chrom] + end of a u32 difference array over all
//                  chromosomes (64-bit offsets), the same on the array of the MAPQ >= -Q reads. Atomic adds whose result is not
//                  used (no return value: the L2 does the add). Sums commute, so the batches of the two routes add in any order.
//   k_gc_add_iv    the same for intervals the host derived (the host route's records): chrom, start, end, uniq as arrays.
//
// end of stream, per array (itx_gcov_finish): a position is a change point when its difference is not 0.
//   k_gc_measure   a tile of GC_TILE slots of ONE chromosome (tiles do not span chromosomes), 16-byte loads: its number of
//                  non-zero slots and the sum of its differences.
//   k_tile_scan2   (itx_textpack.h) both columns scanned over the tiles: where a tile's points go, and the sum before it. The depth
//                  a tile starts from is that sum MINUS the sum before its chromosome's first tile: a chromosome's first slot
//                  starts from depth 0 by construction, whatever the chromosomes before it left behind.
//   k_gc_points    tiles without a point leave at once; the others emit (position, depth from here on, chromosome) compacted, in
//                  order: GC_VEC sweeps of the workgroup over the tile, each a scan of the lanes' counts and sums.
// text in rounds (itx_gcov_next): point k gives a line when its depth is > 0 and point k + 1 lies on the same chromosome:
// [pos_k, pos_{k+1}) with that depth. Neighbouring lines cannot have equal depth (a change point is a non-zero difference).
//   k_gc_text_measure / k_tile_scan2 / k_gc_text_write   line lengths, their places, and the lines formatted a tile at a time in
//                  LDS and stored with full vectors (itx_textpack.h; the digits as itx_bedline.h prints them). A round is a fixed
//                  number of points, so it ends at a line's end; its text comes back into one of two page-locked buffers while the
//                  caller writes the round before.
//
// Integer and byte work. k_gc_add is bound by atomics to L2, the dense pass by HBM bandwidth (the arrays are almost all zeros).
// No kernel uses scratch (DESIGN.md has the figures).
#include "itx_textpack.h"
#include "itx_derive.h"
#include "itx_bedline.h"
#include "itx_gcovbw.h"
#include "itx_devbuf.h"

#include <string.h>

#include <string>
#include <vector>

typedef unsigned long long ull;

#define GC_WG 256u                    // lanes per workgroup of every kernel here
#define GC_SUB (GC_WG * 4u)           // slots one sweep of the workgroup covers: one 16-byte vector per lane
#define GC_VEC 8u                     // sweeps per tile
#define GC_TILE (GC_SUB * GC_VEC)     // 8192 slots, 32 KiB of the array
#define GC_TXT_TILE 256u              // points per workgroup of the text kernels
#define GC_LDS 16384u                 // bytes of text staged at a time: a tile of ordinary lines (256 x 20-40 bytes) in one window
#define GC_LINE_EXTRA 34u             // a line is its name and at most '\t' 10 digits '\t' 10 digits '\t' 10 digits '\n'
#define GC_HOST_CHUNK ((size_t)1 << 20)
#define GC_ROUND_DEFAULT ((size_t)32 << 20)
#define GC_MEMSET_CHUNK ((size_t)1 << 30)

struct GcDev {
    const int2 *tid;                  // [n_tid] (chromosome index or < 0, chromosome size)
    int32_t n_tid, n_chrom;
    const ull *off;                   // [n_chrom] first slot of the chromosome
    const uint32_t *size;             // [n_chrom] its size; 0: it has no slots
    uint32_t *arr[2];                 // the difference arrays: all reads, MAPQ >= -Q
    ull *cnt;                         // [0] records added, [1] records outside their chromosome, [2] added to the unique array; [3], [4]: a scan's totals
    ItxDeriveOpts o;
};

struct GcRecs {
    const int32_t *tid, *pos, *end;
    const uint8_t *mapq, *f5;
    const int32_t *mpos, *isize;
};

// 0 <= start < end <= size - 1, or nothing is written
__device__ __forceinline__ bool gc_add_one(const GcDev &D, int32_t chrom, uint32_t st, uint32_t en, bool uq)
{
    if (chrom < 0 || chrom >= D.n_chrom) return false;
    const uint32_t size = D.size[chrom];
    if (size <= 2u || st >= en || en > size - 1u) return false;
    const ull b = D.off[chrom];
    atomicAdd(&D.arr[0][b + st], 1u);
    atomicAdd(&D.arr[0][b + en], 0xffffffffu);
    if (uq) {
        atomicAdd(&D.arr[1][b + st], 1u);
        atomicAdd(&D.arr[1][b + en], 0xffffffffu);
    }
    return true;
}

__device__ __forceinline__ void gc_count(const GcDev &D, bool cand, bool ok, bool uq)
{
    const ull ma = __ballot(ok), mo = __ballot(cand && !ok), mu = __ballot(ok && uq);
    if ((threadIdx.x & 63u) == 0) {
        if (ma) atomicAdd(&D.cnt[0], (ull)__popcll(ma));
        if (mo) atomicAdd(&D.cnt[1], (ull)__popcll(mo));
        if (mu) atomicAdd(&D.cnt[2], (ull)__popcll(mu));
    }
}

__global__ __launch_bounds__(GC_WG) void k_gc_add(GcDev D, GcRecs R, const int32_t *__restrict__ hit_row, uint32_t n)
{
    const uint32_t i = blockIdx.x * GC_WG + threadIdx.x;
    bool cand = false, ok = false, uq = false;
    if (i < n && hit_row[i] >= 0) {
        const uint32_t f5 = R.f5[i];
        if (!(f5 & F5_NOLOOKUP)) {
            cand = true;
            const int32_t t = R.tid[i];
            const int2 tr = (t >= 0 && t < D.n_tid) ? D.tid[t] : make_int2(-1, 0);
            uint32_t st = 0, en = 0, sd = 0;
            uq = R.mapq[i] >= D.o.mapq_min;
            if (itx_derive(&D.o, tr.x, tr.y, f5, R.pos[i], R.end[i], R.mpos ? R.mpos[i] : 0, R.isize ? R.isize[i] : 0, &st, &en, &sd))
                ok = gc_add_one(D, tr.x, st, en, uq);
        }
    }
    gc_count(D, cand, ok, uq);
}

__global__ __launch_bounds__(GC_WG) void k_gc_add_iv(GcDev D, const int32_t *__restrict__ chrom, const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                     const uint8_t *__restrict__ uniq, uint32_t n)
{
    const uint32_t i = blockIdx.x * GC_WG + threadIdx.x;
    bool cand = false, ok = false, uq = false;
    if (i < n) {
        cand = true;
        uq = uniq[i] != 0;
        ok = gc_add_one(D, chrom[i], start[i], end[i], uq);
    }
    gc_count(D, cand, ok, uq);
}

// ---- the dense pass
struct GcVisit {                      // the chromosomes with slots in the order they are written, and their tiles
    const uint32_t *first;            // [nv + 1] first tile of visited chromosome k
    const ull *off;                   // [nv]
    const uint32_t *size;             // [nv]
    uint32_t nv;
};

// the visited chromosome tile `t` belongs to: the last k with first[k] <= t
__device__ __forceinline__ uint32_t gc_visit_of(const GcVisit &V, uint32_t t)
{
    uint32_t lo = 0, hi = V.nv;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (V.first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the 4 differences at slots [p, p + 4) of a chromosome of `size` slots starting at a; slots >= size read as 0
__device__ __forceinline__ uint4 gc_load(const uint32_t *__restrict__ a, uint32_t p, uint32_t size)
{
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    if (p < size) {
        d = *reinterpret_cast<const uint4 *>(a + p);                  // (a and p are multiples of 4 slots; the array is padded)
        if (p + 1u >= size) d.y = 0u;
        if (p + 2u >= size) d.z = 0u;
        if (p + 3u >= size) d.w = 0u;
    }
    return d;
}

__global__ __launch_bounds__(GC_WG) void k_gc_measure(const uint32_t *__restrict__ arr, GcVisit V, ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_acc[2];
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t k = gc_visit_of(V, blockIdx.x);
    const uint32_t size = V.size[k], p0 = (blockIdx.x - V.first[k]) * GC_TILE;
    const uint32_t *a = arr + V.off[k];
    uint32_t c = 0, s = 0;
#pragma unroll
    for (uint32_t v = 0; v < GC_VEC; v++) {
        const uint4 d = gc_load(a, p0 + v * GC_SUB + 4u * threadIdx.x, size);
        c += (d.x != 0u) + (d.y != 0u) + (d.z != 0u) + (d.w != 0u);
        s += d.x + d.y + d.z + d.w;
    }
    for (int o = 32; o > 0; o >>= 1) {
        c += (uint32_t)__shfl_down((int32_t)c, o, 64);
        s += (uint32_t)__shfl_down((int32_t)s, o, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (c) atomicAdd(&s_acc[0], c);
        if (s) atomicAdd(&s_acc[1], s);
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2ull * blockIdx.x + threadIdx.x] = s_acc[threadIdx.x];     // (sums are taken mod 2^32 in the end)
}

__global__ __launch_bounds__(GC_WG) void k_gc_points(const uint32_t *__restrict__ arr, GcVisit V, const ull *__restrict__ tile_sum, const ull *__restrict__ tile_base,
                                                     uint4 *__restrict__ pts)
{
    __shared__ uint32_t s_wc[GC_WG / 64u], s_wd[GC_WG / 64u];
    if (tile_sum[2ull * blockIdx.x] == 0) return;                        // no point in this tile (the whole workgroup leaves)
    const uint32_t k = gc_visit_of(V, blockIdx.x);
    const uint32_t size = V.size[k], p0 = (blockIdx.x - V.first[k]) * GC_TILE;
    const uint32_t *a = arr + V.off[k];
    ull at = tile_base[2ull * blockIdx.x];
    // depth 0 at the chromosome's first slot: the sum before this tile less the sum before the chromosome's first tile
    uint32_t depth0 = (uint32_t)(tile_base[2ull * blockIdx.x + 1u] - tile_base[2ull * V.first[k] + 1u]);
    for (uint32_t v = 0; v < GC_VEC; v++) {
        const uint32_t p = p0 + v * GC_SUB + 4u * threadIdx.x;
        const uint4 d = gc_load(a, p, size);
        const uint32_t c = (d.x != 0u) + (d.y != 0u) + (d.z != 0u) + (d.w != 0u), s = d.x + d.y + d.z + d.w;
        uint32_t tc = 0, td = 0;
        const uint32_t oc = itx_tile_offsets<GC_WG>(c, s_wc, &tc), od = itx_tile_offsets<GC_WG>(s, s_wd, &td);
        if (c) {
            ull j = at + oc;
            uint32_t depth = depth0 + od;
            const uint32_t dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                depth += dd[q];
                if (dd[q]) pts[j++] = make_uint4(p + q, depth, k, 0u);
            }
        }
        at += tc;
        depth0 += td;
        __syncthreads();                                                  // s_wc, s_wd are written again by the next sweep
    }
}

// ---- the text
struct GcText {
    const uint4 *pts;                 // (position, depth from here on, visited chromosome, 0)
    ull n_pts;
    const uint2 *name;                // [nv] (offset into pool, length)
    const uint8_t *pool;
};

// the line of point j: false when it has none. [P.x, *end) at depth P.y on chromosome P.z
__device__ __forceinline__ bool gc_line_of(const GcText &T, ull j, uint4 *P, uint32_t *end)
{
    if (j >= T.n_pts) return false;
    *P = T.pts[j];
    if (P->y == 0u || j + 1 >= T.n_pts) return false;
    const uint4 N = T.pts[j + 1];
    if (N.z != P->z) return false;                                       // (a chromosome's depth is 0 behind its last point)
    *end = N.x;
    return true;
}

__global__ __launch_bounds__(GC_TXT_TILE) void k_gc_text_measure(GcText T, ull first, uint32_t n, ull *__restrict__ tile_sum)
{
    __shared__ ull s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * GC_TXT_TILE + threadIdx.x;
    uint4 P;
    uint32_t end = 0;
    if (i < n && gc_line_of(T, first + i, &P, &end)) {
        const uint32_t len = T.name[P.z].y + 4u + itx_bed_declen(P.x) + itx_bed_declen(end) + itx_bed_declen(P.y);
        atomicAdd(&s_sum[0], (ull)len);
        atomicAdd(&s_sum[1], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

// the bytes [lo, hi) of "name \t start \t end \t depth \n"
__device__ __forceinline__ void gc_line_write(const uint8_t *name, uint32_t name_len, uint32_t start, uint32_t end, uint32_t depth, uint8_t *dst, uint32_t lo, uint32_t hi)
{
    uint32_t pos = 0;
    pos = itx_bed_put_str(dst, lo, hi, pos, name, name_len);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_u32(dst, lo, hi, pos, start);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_u32(dst, lo, hi, pos, end);
    ITX_BED_PUT('\t');
    pos = itx_bed_put_u32(dst, lo, hi, pos, depth);
    ITX_BED_PUT('\n');
}

__global__ __launch_bounds__(GC_TXT_TILE) void k_gc_text_write(GcText T, ull first, uint32_t n, const ull *__restrict__ tile_base, uint8_t *__restrict__ out)
{
    __shared__ uint4 s_buf[GC_LDS / 16u];
    __shared__ uint32_t s_w[GC_TXT_TILE / 64u];
    const uint32_t i = blockIdx.x * GC_TXT_TILE + threadIdx.x;
    uint4 P = make_uint4(0u, 0u, 0u, 0u);
    uint32_t end = 0, len = 0;
    uint2 nm = make_uint2(0u, 0u);
    if (i < n && gc_line_of(T, first + i, &P, &end)) {
        nm = T.name[P.z];
        len = nm.y + 4u + itx_bed_declen(P.x) + itx_bed_declen(end) + itx_bed_declen(P.y);
    }
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<GC_TXT_TILE>(len, s_w, &total);
    const ull tb = tile_base[2u * blockIdx.x], te = tb + total;
    const ull mb = tb + moff, me = mb + len;
    const uint8_t *name = T.pool + nm.x;
    itx_pack_tile<GC_TXT_TILE, GC_LDS>(s_buf, out, tb, te, mb, me,
                                       [=](uint8_t *dst, uint32_t from, uint32_t to) { gc_line_write(name, nm.y, P.x, end, P.y, dst, from, to); });
}

// ---- host side
struct GcFile {                       // one of the two files, from finish on
    ItxBuf d_pts;                     // uint4[n_pts]
    ull n_pts, cursor;
    int started, done, flying;        // flying: a round is in slot `slot`
    int slot;
    uint64_t len[2];
    GcBw *bw;                         // its bigWig content, once built (itx_gcovbw.hip)
};

struct itx_gcov {
    int device;
    GcDev d;                          // (its two arrays are allocated and given back by hand: timed, and free before the text)
    std::vector<int64_t> chrom_size;
    ItxBuf d_tid, d_off, d_size, d_cnt, d_hits;
    ItxPin h_tot;
    ull slots;
    hipStream_t st, last;             // last: where the newest add kernel was enqueued
    ItxEvent ev_add[2], ev_rnd[2][3];
    int add_timed;
    ItxBuf d_hc, d_hs, d_he, d_hu;    // the host route's intervals on their way up
    // from finish on
    int finished, cur_file;
    GcFile file[2];
    ItxBuf d_vfirst, d_voff, d_vsize, d_vname, d_pool;
    GcVisit V;
    uint32_t max_name;
    ull per_round;
    ItxBuf d_text[2];                 // a round's text: both of one size, as are the page-locked two
    ItxPin h_text[2];
    ItxBuf d_tsum, d_tbase, d_ttot;
    std::vector<uint32_t> h_vsize, h_vchrom;                               // the visited chromosomes: size, index into chrom_size
    itx_gcov_stats stats;
};

#define GC_RC(call)                               \
    do {                                          \
        if ((rc = (call)) != ITX_OK) goto out;    \
    } while (0)

static void gc_free_arrays(itx_gcov *g)
{
    for (auto &a : g->d.arr) {
        (void)hipFree(a);
        a = nullptr;
    }
}

extern "C" void itx_gcov_destroy(itx_gcov *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->last) (void)hipStreamSynchronize(g->last);
    if (g->st) (void)hipStreamSynchronize(g->st);
    if (g->st) (void)hipStreamDestroy(g->st);
    gc_free_arrays(g);
    for (auto &f : g->file) gcbw_free(f.bw);
    delete g;
}

extern "C" int itx_gcov_create(int device, const int64_t *chrom_size, int n_chrom, const itx_params *p, size_t batch_capacity, itx_gcov **out)
{
    if (!out || n_chrom < 0 || (n_chrom && !chrom_size) || !p || batch_capacity == 0 || batch_capacity > 0xffffff00u) {
        itx_set_error("itx_gcov_create: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    for (int c = 0; c < n_chrom; c++)
        if (chrom_size[c] > 0x7fffffffll) {
            itx_set_error("itx_gcov_create: chromosome %d has %lld bases, more than 2^31 - 1", c, (long long)chrom_size[c]);
            return ITX_E_LIMIT;
        }
    int rc = ITX_OK;
    itx_gcov *g = new itx_gcov();
    g->device = device;
    g->cur_file = -1;
    g->chrom_size.assign(chrom_size, chrom_size + n_chrom);
    g->d.n_chrom = n_chrom;
    g->d.o.mapq_min = (uint32_t)p->mapq_min;
    g->d.o.extension = p->extension;
    g->d.o.isize_max = p->isize_max;
    g->d.o.treat = p->treat_pe_as_se;
    g->d.o.discard = p->discard_half_mapped;
    // a chromosome of size <= 2 is "not found" to the reference (generic.c:796-797): no slots. Every chromosome starts on a
    // 16-byte boundary, and the array ends with a vector of padding
    std::vector<ull> off((size_t)n_chrom + 1, 0ull);
    std::vector<uint32_t> size((size_t)n_chrom + 1, 0u);
    ull total = 0;
    for (int c = 0; c < n_chrom; c++) {
        off[(size_t)c] = total;
        if (chrom_size[c] > 2) {
            size[(size_t)c] = (uint32_t)chrom_size[c];
            total += ((ull)chrom_size[c] + 3ull) & ~3ull;
        }
    }
    g->slots = total;
    const size_t bytes = (size_t)(4ull * (total + 4ull));
    ITX_TRY(hipSetDevice(device));
    {
        // the two arrays first: when the device cannot hold them nothing else has been touched
        const double t0 = itx_wall_now();
        for (auto &a : g->d.arr)
            if (hipMalloc((void **)&a, bytes) != hipSuccess) {
                (void)hipGetLastError();
                a = nullptr;
                itx_set_error("itx_gcov_create: no device memory for two coverage arrays of %zu bytes each (%llu bases in the chromosome size file)", bytes, total);
                rc = ITX_E_NOMEM;
                goto out;
            }
        g->stats.alloc_s = itx_wall_now() - t0;
    }
    g->stats.slots = total;
    g->stats.device_bytes = 2ull * bytes;
    ITX_TRY(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking));
    for (auto &e : g->ev_add) GC_RC(itx_event_make(e));
    for (auto &s : g->ev_rnd)
        for (auto &e : s) GC_RC(itx_event_make(e));
    ITX_TRY(hipEventRecord(g->ev_rnd[0][0], g->st));
    for (auto &a : g->d.arr)
        for (size_t at = 0; at < bytes; at += GC_MEMSET_CHUNK)
            ITX_TRY(hipMemsetAsync((uint8_t *)a + at, 0, bytes - at < GC_MEMSET_CHUNK ? bytes - at : GC_MEMSET_CHUNK, g->st));
    ITX_TRY(hipEventRecord(g->ev_rnd[0][1], g->st));
    GC_RC(itx_buf_need("itx_gcov_create", g->d_off, 8 * off.size()));
    GC_RC(itx_buf_need("itx_gcov_create", g->d_size, 4 * size.size()));
    GC_RC(itx_buf_need("itx_gcov_create", g->d_cnt, 64));
    GC_RC(itx_buf_need("itx_gcov_create", g->d_hits, 4 * (batch_capacity + 64)));
    GC_RC(itx_pin_need("itx_gcov_create", g->h_tot, 64));
    ITX_TRY(hipMemcpyAsync(g->d_off.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, g->st));
    ITX_TRY(hipMemcpyAsync(g->d_size.p, size.data(), 4 * size.size(), hipMemcpyHostToDevice, g->st));
    ITX_TRY(hipMemsetAsync(g->d_cnt.p, 0, 64, g->st));
    ITX_TRY(hipStreamSynchronize(g->st));                                   // off, size are this function's
    {
        float ms = 0;
        ITX_TRY(hipEventElapsedTime(&ms, g->ev_rnd[0][0], g->ev_rnd[0][1]));
        g->stats.zero_ms = (double)ms;
    }
    g->d.off = g->d_off.as<ull>();
    g->d.size = g->d_size.as<uint32_t>();
    g->d.cnt = g->d_cnt.as<ull>();
out:
    if (rc != ITX_OK) {
        itx_gcov_destroy(g);
        return rc;
    }
    *out = g;
    return ITX_OK;
}

extern "C" int32_t *itx_gcov_hits(itx_gcov *g) { return g ? g->d_hits.as<int32_t>() : nullptr; }
extern "C" void *itx_gcov_stream(itx_gcov *g) { return g ? (void *)g->st : nullptr; }

// the newest add kernel is waited for and its time read
static int gc_settle(itx_gcov *g)
{
    int rc = ITX_OK;
    if (g->add_timed) {
        float ms = 0;
        ITX_TRY(hipEventSynchronize(g->ev_add[1]));
        ITX_TRY(hipEventElapsedTime(&ms, g->ev_add[0], g->ev_add[1]));
        g->stats.add_ms += (double)ms;
        g->add_timed = 0;
    }
out:
    return rc;
}

extern "C" int itx_gcov_set_tidmap(itx_gcov *g, const int32_t *tid2chrom, int n_tid)
{
    if (!g || n_tid < 0 || (n_tid && !tid2chrom)) {
        itx_set_error("itx_gcov_set_tidmap: bad argument");
        return ITX_E_ARG;
    }
    if (g->finished) {
        itx_set_error("itx_gcov_set_tidmap: the coverage is finished");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    ItxBuf nt;
    std::vector<int2> v((size_t)n_tid + 1, make_int2(-1, 0));
    for (int k = 0; k < n_tid; k++) {
        const int32_t c = tid2chrom[k];
        v[(size_t)k] = make_int2(c, (c >= 0 && (size_t)c < g->chrom_size.size()) ? (int32_t)g->chrom_size[(size_t)c] : 0);
    }
    ITX_TRY(hipSetDevice(g->device));
    if ((rc = gc_settle(g)) != ITX_OK) goto out;                           // no kernel reads the old map any more
    GC_RC(itx_buf_need("itx_gcov_set_tidmap", nt, sizeof(int2) * v.size()));
    ITX_TRY(hipMemcpy(nt.p, v.data(), sizeof(int2) * v.size(), hipMemcpyHostToDevice));
    g->d_tid.swap(nt);
    g->d.tid = g->d_tid.as<int2>();
    g->d.n_tid = n_tid;
out:
    return rc;                                                             // (nt goes: the old map, or the new one that was not taken)
}

extern "C" int itx_gcov_run(itx_gcov *g, const itx_batch *b, const int32_t *d_hit_row, size_t n, void *stream)
{
    if (!g || !b || n > 0xffffff00u || (n && (!d_hit_row || !b->tid || !b->pos || !b->tmpend || !b->mapq || !b->flag5))) {
        itx_set_error("itx_gcov_run: bad argument");
        return ITX_E_ARG;
    }
    if (g->finished || !g->d.tid) {
        itx_set_error("itx_gcov_run: %s", g->finished ? "the coverage is finished" : "no tid map");
        return ITX_E_STATE;
    }
    if (!n) return ITX_OK;
    int rc = ITX_OK;
    const GcRecs R = {b->tid, b->pos, b->tmpend, b->mapq, b->flag5, b->mpos, b->isize};
    hipStream_t st = (hipStream_t)stream;
    ITX_TRY(hipSetDevice(g->device));
    if ((rc = gc_settle(g)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(g->ev_add[0], st));
    hipLaunchKernelGGL(k_gc_add, dim3((uint32_t)((n + GC_WG - 1) / GC_WG)), dim3(GC_WG), 0, st, g->d, R, d_hit_row, (uint32_t)n);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(g->ev_add[1], st));
    g->add_timed = 1;
    g->last = st;
    g->stats.batches++;
out:
    return rc;
}

extern "C" int itx_gcov_wait_kernels(itx_gcov *g)
{
    if (!g) {
        itx_set_error("itx_gcov_wait_kernels: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(g->device));
    {
        const double t0 = itx_wall_now();
        rc = gc_settle(g);
        g->stats.wait_s += itx_wall_now() - t0;
    }
out:
    return rc;
}

extern "C" int itx_gcov_add_host(itx_gcov *g, const int32_t *chrom, const uint32_t *start, const uint32_t *end, const uint8_t *uniq, size_t n)
{
    if (!g || (n && (!chrom || !start || !end || !uniq))) {
        itx_set_error("itx_gcov_add_host: bad argument");
        return ITX_E_ARG;
    }
    if (g->finished) {
        itx_set_error("itx_gcov_add_host: the coverage is finished");
        return ITX_E_STATE;
    }
    if (!n) return ITX_OK;
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(g->device));
    GC_RC(itx_buf_need("itx_gcov_add_host", g->d_hc, 4 * GC_HOST_CHUNK));
    GC_RC(itx_buf_need("itx_gcov_add_host", g->d_hs, 4 * GC_HOST_CHUNK));
    GC_RC(itx_buf_need("itx_gcov_add_host", g->d_he, 4 * GC_HOST_CHUNK));
    GC_RC(itx_buf_need("itx_gcov_add_host", g->d_hu, GC_HOST_CHUNK));
    if ((rc = gc_settle(g)) != ITX_OK) goto out;
    for (size_t at = 0; at < n; at += GC_HOST_CHUNK) {
        const size_t m = n - at < GC_HOST_CHUNK ? n - at : GC_HOST_CHUNK;
        ITX_TRY(hipMemcpyAsync(g->d_hc.p, chrom + at, 4 * m, hipMemcpyHostToDevice, g->st));
        ITX_TRY(hipMemcpyAsync(g->d_hs.p, start + at, 4 * m, hipMemcpyHostToDevice, g->st));
        ITX_TRY(hipMemcpyAsync(g->d_he.p, end + at, 4 * m, hipMemcpyHostToDevice, g->st));
        ITX_TRY(hipMemcpyAsync(g->d_hu.p, uniq + at, m, hipMemcpyHostToDevice, g->st));
        ITX_TRY(hipEventRecord(g->ev_add[0], g->st));
        hipLaunchKernelGGL(k_gc_add_iv, dim3((uint32_t)((m + GC_WG - 1) / GC_WG)), dim3(GC_WG), 0, g->st, g->d, g->d_hc.as<int32_t>(), g->d_hs.as<uint32_t>(), g->d_he.as<uint32_t>(),
                           g->d_hu.as<uint8_t>(), (uint32_t)m);
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipEventRecord(g->ev_add[1], g->st));
        g->add_timed = 1;
        g->last = g->st;
        if ((rc = gc_settle(g)) != ITX_OK) goto out;                       // the chunk's buffers are free, the caller's arrays its own again
    }
    g->stats.host_batches++;
out:
    return rc;
}

// the change points of array w: measured, scanned, emitted. The tile arrays are the caller's (d_tsum, d_tbase: 16 bytes a tile)
static int gc_points(itx_gcov *g, int w, uint32_t n_tiles, ull *d_tsum, ull *d_tbase)
{
    int rc = ITX_OK;
    GcFile &F = g->file[w];
    if (!n_tiles) return ITX_OK;
    hipLaunchKernelGGL(k_gc_measure, dim3(n_tiles), dim3(GC_WG), 0, g->st, g->d.arr[w], g->V, d_tsum);
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, g->st, d_tsum, n_tiles, d_tbase, g->d.cnt + 3);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipMemcpyAsync(g->h_tot.p, g->d.cnt + 3, 8, hipMemcpyDeviceToHost, g->st));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(g->st));
        g->stats.wait_s += itx_wall_now() - t0;
    }
    F.n_pts = g->h_tot.as<ull>()[0];
    if (!F.n_pts) return ITX_OK;
    if ((rc = itx_buf_need("itx_gcov_finish", F.d_pts, sizeof(uint4) * (size_t)F.n_pts)) != ITX_OK) {
        itx_set_error("itx_gcov_finish: no device memory for %llu change points", F.n_pts);
        return rc;
    }
    hipLaunchKernelGGL(k_gc_points, dim3(n_tiles), dim3(GC_WG), 0, g->st, g->d.arr[w], g->V, d_tsum, d_tbase, F.d_pts.as<uint4>());
    ITX_TRY(hipGetLastError());
out:
    return rc;
}

extern "C" int itx_gcov_finish(itx_gcov *g, const uint32_t *order, int n_order, const char *name_bytes, const uint64_t *name_off, size_t round_bytes)
{
    if (!g || n_order < 0 || (n_order && (!order || !name_off))) {
        itx_set_error("itx_gcov_finish: bad argument");
        return ITX_E_ARG;
    }
    if (g->finished) {
        itx_set_error("itx_gcov_finish: called twice");
        return ITX_E_STATE;
    }
    const size_t nc = g->chrom_size.size();
    std::vector<uint8_t> seen(nc + 1, 0);
    std::vector<uint32_t> vfirst, vsize, vchrom;
    std::vector<ull> voff, off(nc + 1, 0ull);
    std::vector<uint2> vname;
    std::string pool;
    ull tiles = 0, at = 0;
    uint32_t max_name = 0;
    for (size_t c = 0; c < nc; c++) {
        off[c] = at;
        if (g->chrom_size[c] > 2) at += ((ull)g->chrom_size[c] + 3ull) & ~3ull;
    }
    for (size_t c = 0; c < nc; c++)
        if (n_order && (name_off[c + 1] < name_off[c] || name_off[c + 1] - name_off[c] > 0xffffu || (name_off[c + 1] > name_off[c] && !name_bytes))) {
            itx_set_error("itx_gcov_finish: the name offsets do not ascend, or a name has 2^16 bytes or more");
            return ITX_E_ARG;
        }
    for (int k = 0; k < n_order; k++) {
        const uint32_t c = order[k];
        if (c >= nc || seen[c]) {
            itx_set_error("itx_gcov_finish: order[%d] = %u is %s", k, c, c >= nc ? "no chromosome" : "visited twice");
            return ITX_E_ARG;
        }
        seen[c] = 1;
        if (g->chrom_size[c] <= 2) continue;                               // no slots: nothing to visit
        const uint32_t len = (uint32_t)(name_off[c + 1] - name_off[c]);
        vfirst.push_back((uint32_t)tiles);
        vsize.push_back((uint32_t)g->chrom_size[c]);
        vchrom.push_back(c);
        voff.push_back(off[c]);
        vname.push_back(make_uint2((uint32_t)pool.size(), len));
        pool.append(name_bytes + name_off[c], len);
        if (len > max_name) max_name = len;
        tiles += ((ull)g->chrom_size[c] + GC_TILE - 1) / GC_TILE;
    }
    if (tiles > 0x7fffffffull) {
        itx_set_error("itx_gcov_finish: %llu tiles of %u bases", tiles, GC_TILE);
        return ITX_E_LIMIT;
    }
    vfirst.push_back((uint32_t)tiles);
    pool.append(16, '\0');
    const uint32_t nv = (uint32_t)vsize.size(), n_tiles = (uint32_t)tiles;
    if (!round_bytes) round_bytes = GC_ROUND_DEFAULT;
    if (round_bytes > ((size_t)1 << 30)) round_bytes = (size_t)1 << 30;
    const ull line_max = (ull)max_name + GC_LINE_EXTRA;
    const ull per_round = round_bytes / line_max ? round_bytes / line_max : 1ull;     // points a round: its text fits round_bytes, or is one line
    const size_t text_cap = (size_t)(per_round * line_max) + 16;
    const size_t txt_tiles = (size_t)((per_round + GC_TXT_TILE - 1) / GC_TXT_TILE) + 1;
    int rc = ITX_OK;
    const char *const who = "itx_gcov_finish";
    ItxBuf tsum, tbase;                                                    // the dense pass's tile arrays
    ItxEvent e0, e1;
    float ms = 0;
    ITX_TRY(hipSetDevice(g->device));
    if ((rc = gc_settle(g)) != ITX_OK) goto out;
    ITX_TRY(hipStreamSynchronize(g->st));
    ITX_TRY(hipMemcpy(g->h_tot.p, g->d_cnt.p, 24, hipMemcpyDeviceToHost));
    g->stats.records = g->h_tot.as<ull>()[0];
    g->stats.out_of_range = g->h_tot.as<ull>()[1];
    g->stats.records_uniq = g->h_tot.as<ull>()[2];
    GC_RC(itx_event_make(e0));
    GC_RC(itx_event_make(e1));
    // everything the rounds will need, before the first point is made: a refusal leaves the arrays as they were
    if ((rc = itx_buf_need(who, tsum, 16 * ((size_t)n_tiles + 1))) || (rc = itx_buf_need(who, tbase, 16 * ((size_t)n_tiles + 1))) ||
        (rc = itx_buf_need(who, g->d_vfirst, 4 * vfirst.size())) || (rc = itx_buf_need(who, g->d_voff, 8 * (voff.size() + 1))) ||
        (rc = itx_buf_need(who, g->d_vsize, 4 * (vsize.size() + 1))) || (rc = itx_buf_need(who, g->d_vname, 8 * (vname.size() + 1))) ||
        (rc = itx_buf_need(who, g->d_pool, pool.size())) || (rc = itx_buf_need(who, g->d_tsum, 16 * txt_tiles)) ||
        (rc = itx_buf_need(who, g->d_tbase, 16 * txt_tiles)) || (rc = itx_buf_need(who, g->d_ttot, 32)) ||
        (rc = itx_buf_need(who, g->d_text[0], text_cap)) || (rc = itx_buf_need(who, g->d_text[1], text_cap)) ||
        (rc = itx_pin_need(who, g->h_text[0], text_cap)) || (rc = itx_pin_need(who, g->h_text[1], text_cap))) {
        itx_set_error("itx_gcov_finish: no memory for %u tiles and rounds of %zu bytes", n_tiles, text_cap);
        goto out;
    }
    ITX_TRY(hipMemcpyAsync(g->d_vfirst.p, vfirst.data(), 4 * vfirst.size(), hipMemcpyHostToDevice, g->st));
    if (nv) {
        ITX_TRY(hipMemcpyAsync(g->d_voff.p, voff.data(), 8 * voff.size(), hipMemcpyHostToDevice, g->st));
        ITX_TRY(hipMemcpyAsync(g->d_vsize.p, vsize.data(), 4 * vsize.size(), hipMemcpyHostToDevice, g->st));
        ITX_TRY(hipMemcpyAsync(g->d_vname.p, vname.data(), 8 * vname.size(), hipMemcpyHostToDevice, g->st));
    }
    ITX_TRY(hipMemcpyAsync(g->d_pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice, g->st));
    ITX_TRY(hipStreamSynchronize(g->st));                                   // the vectors are this function's
    g->V.first = g->d_vfirst.as<uint32_t>();
    g->V.off = g->d_voff.as<ull>();
    g->V.size = g->d_vsize.as<uint32_t>();
    g->V.nv = nv;
    g->max_name = max_name;
    g->h_vsize = vsize;
    g->h_vchrom = vchrom;
    g->per_round = per_round;
    ITX_TRY(hipEventRecord(e0, g->st));
    for (int w = 0; w < 2; w++)
        if ((rc = gc_points(g, w, n_tiles, tsum.as<ull>(), tbase.as<ull>())) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(e1, g->st));
    ITX_TRY(hipStreamSynchronize(g->st));
    ITX_TRY(hipEventElapsedTime(&ms, e0, e1));
    g->stats.points_ms = (double)ms;
    for (int w = 0; w < 2; w++) g->stats.points[w] = g->file[w].n_pts;
    gc_free_arrays(g);                                                     // 4 bytes a base, twice: given back before the text is made
    g->finished = 1;
out:
    if (rc != ITX_OK) {
        // a refused finish made no points: the arrays are as they were, a later finish starts again
        if (g->st) (void)hipStreamSynchronize(g->st);
        for (auto &f : g->file) {
            f.d_pts.drop();
            f.n_pts = 0;
        }
    }
    return rc;
}

// the next round of file w into slot s: lengths, scan (waited for: the size decides the copy), format, copy
static int gc_start_round(itx_gcov *g, int w, int s)
{
    int rc = ITX_OK;
    GcFile &F = g->file[w];
    const ull left = F.n_pts - F.cursor;
    const uint32_t n = (uint32_t)(left < g->per_round ? left : g->per_round), nt = (n + GC_TXT_TILE - 1) / GC_TXT_TILE;
    const GcText T = {F.d_pts.as<uint4>(), F.n_pts, g->d_vname.as<uint2>(), g->d_pool.as<uint8_t>()};
    ull *const d_tsum = g->d_tsum.as<ull>(), *const d_tbase = g->d_tbase.as<ull>(), *const h_tot = g->h_tot.as<ull>();
    ITX_TRY(hipEventRecord(g->ev_rnd[s][0], g->st));
    hipLaunchKernelGGL(k_gc_text_measure, dim3(nt), dim3(GC_TXT_TILE), 0, g->st, T, F.cursor, n, d_tsum);
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, g->st, d_tsum, nt, d_tbase, g->d_ttot.as<ull>());
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipMemcpyAsync(h_tot, g->d_ttot.p, 16, hipMemcpyDeviceToHost, g->st));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(g->st));
        g->stats.wait_s += itx_wall_now() - t0;
    }
    F.len[s] = h_tot[0];
    if (F.len[s] + 16 > g->d_text[s].cap) {                                // (a line is never longer than its bound)
        itx_set_error("itx_gcov_next: a round of %llu bytes in a buffer of %zu", (ull)F.len[s], g->d_text[s].cap);
        rc = ITX_E_LIMIT;
        goto out;
    }
    g->stats.lines[w] += h_tot[1];
    g->stats.bytes[w] += F.len[s];
    g->stats.rounds[w]++;
    if (F.len[s]) {
        hipLaunchKernelGGL(k_gc_text_write, dim3(nt), dim3(GC_TXT_TILE), 0, g->st, T, F.cursor, n, d_tbase, g->d_text[s].as<uint8_t>());
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipEventRecord(g->ev_rnd[s][1], g->st));
    if (F.len[s]) ITX_TRY(hipMemcpyAsync(g->h_text[s].p, g->d_text[s].p, (size_t)F.len[s], hipMemcpyDeviceToHost, g->st));
    ITX_TRY(hipEventRecord(g->ev_rnd[s][2], g->st));
    F.cursor += n;
    F.slot = s;
    F.flying = 1;
out:
    return rc;
}

extern "C" int itx_gcov_next(itx_gcov *g, int which, itx_gcov_text *out)
{
    if (!g || !out || which < 0 || which > 1) {
        itx_set_error("itx_gcov_next: bad argument");
        return ITX_E_ARG;
    }
    GcFile &F = g->file[which];
    if (!g->finished || F.done || (g->cur_file >= 0 && g->cur_file != which && !g->file[g->cur_file].done)) {
        itx_set_error("itx_gcov_next: %s", !g->finished ? "itx_gcov_finish comes first" : F.done ? "this file has been handed out" : "the other file's rounds come first");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    float ms = 0;
    out->bytes = nullptr;
    out->len = 0;
    out->more = 0;
    ITX_TRY(hipSetDevice(g->device));
    g->cur_file = which;
    if (!F.started) {
        F.started = 1;
        if (F.n_pts && (rc = gc_start_round(g, which, 0)) != ITX_OK) goto out;
    }
    if (!F.flying) {                                                       // no point at all: an empty file
        F.done = 1;
        goto out;
    }
    {
        const int s = F.slot;
        const double t0 = itx_wall_now();
        ITX_TRY(hipEventSynchronize(g->ev_rnd[s][2]));
        g->stats.wait_s += itx_wall_now() - t0;
        ITX_TRY(hipEventElapsedTime(&ms, g->ev_rnd[s][0], g->ev_rnd[s][1]));
        g->stats.text_ms += (double)ms;
        F.flying = 0;
        out->bytes = F.len[s] ? g->h_text[s].as<const char>() : nullptr;
        out->len = F.len[s];
        // the round after it is formatted and copied while the caller writes this one
        if (F.cursor < F.n_pts) {
            if ((rc = gc_start_round(g, which, s ^ 1)) != ITX_OK) goto out;
            out->more = 1;
        } else {
            F.done = 1;
        }
    }
out:
    return rc;
}

// ---- the bigWig content of a file (itx_gcovbw.hip builds it from the change points; the text rounds read the same points and
// neither writes them)
extern "C" int itx_gcov_bigwig_build(itx_gcov *g, int which)
{
    if (!g || which < 0 || which > 1) {
        itx_set_error("itx_gcov_bigwig_build: bad argument");
        return ITX_E_ARG;
    }
    GcFile &F = g->file[which];
    if (!g->finished || F.bw) {
        itx_set_error("itx_gcov_bigwig_build: %s", !g->finished ? "itx_gcov_finish comes first" : "this file's bigWig content has been built");
        return ITX_E_STATE;
    }
    GcBw *b = nullptr;
    const int rc = gcbw_build(g->device, g->st, F.d_pts.as<uint4>(), F.n_pts, g->h_vsize.data(), g->h_vchrom.data(), (uint32_t)g->h_vsize.size(), &b);
    if (rc != ITX_OK) return rc;
    F.bw = b;
    itx_gcov_bw_result r;
    gcbw_result(b, &r);
    g->stats.bw_items[which] = r.n_items;
    g->stats.bw_sections[which] = r.n_sec;
    g->stats.bw_levels[which] = r.n_levels;
    for (uint32_t k = 0; k < r.n_levels; k++) g->stats.bw_summaries[which] += r.n_sum[k];
    g->stats.bw_ms += gcbw_device_ms(b);
    return ITX_OK;
}

extern "C" int itx_gcov_bigwig_result(itx_gcov *g, int which, itx_gcov_bw_result *out)
{
    if (!g || !out || which < 0 || which > 1) {
        itx_set_error("itx_gcov_bigwig_result: bad argument");
        return ITX_E_ARG;
    }
    if (!g->file[which].bw) {
        itx_set_error("itx_gcov_bigwig_result: itx_gcov_bigwig_build comes first");
        return ITX_E_STATE;
    }
    gcbw_result(g->file[which].bw, out);
    return ITX_OK;
}

extern "C" int itx_gcov_copy_points(itx_gcov *g, int which, uint32_t *out)
{
    if (!g || which < 0 || which > 1 || (g->finished && g->file[which].n_pts && !out)) {
        itx_set_error("itx_gcov_copy_points: bad argument");
        return ITX_E_ARG;
    }
    if (!g->finished) {
        itx_set_error("itx_gcov_copy_points: itx_gcov_finish comes first");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    const GcFile &F = g->file[which];
    ITX_TRY(hipSetDevice(g->device));
    ITX_TRY(hipStreamSynchronize(g->st));
    if (F.n_pts) ITX_TRY(hipMemcpy(out, F.d_pts.p, sizeof(uint4) * (size_t)F.n_pts, hipMemcpyDeviceToHost));
out:
    return rc;
}

extern "C" int itx_gcov_get_stats(itx_gcov *g, itx_gcov_stats *out)
{
    if (!g || !out) {
        itx_set_error("itx_gcov_get_stats: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    if (!g->finished) {                                                    // (finish reads the counters for good)
        ITX_TRY(hipSetDevice(g->device));
        if ((rc = gc_settle(g)) != ITX_OK) goto out;
        ITX_TRY(hipStreamSynchronize(g->st));
        ITX_TRY(hipMemcpy(g->h_tot.p, g->d_cnt.p, 24, hipMemcpyDeviceToHost));
        g->stats.records = g->h_tot.as<ull>()[0];
        g->stats.out_of_range = g->h_tot.as<ull>()[1];
        g->stats.records_uniq = g->h_tot.as<ull>()[2];
    }
    *out = g->stats;
out:
    return rc;
}
