// itx_bed.hip — the bed files of `iteres stat -B / -V` (generic.c:925-936) built where the records lie: one line per record that
// reaches the bed stage, in file order, as finished text. The host used to fetch the inflated bytes of every batch back over
// PCIe, parse each record a second time for its name and fprintf the line; here only the text crosses the link.
//
//   k_bed_measure  one thread per record: itx_derive (itx_derive.h) says whether the record has a line and with which
//                  coordinates, a record the device -R pass marked ITX_F5_NOLOOKUP has none (generic.c:907-919 comes before
//                  925); itx_bed_scan (itx_bedline.h) walks the record for its name and its XA / NM tags; the byte lengths of
//                  the -B and of the -V line (-V only when MAPQ >= -Q). What the walk found is kept per record, so the tags
//                  are walked once. A tile of BED_TILE records adds up its lengths (64 bit).
//   k_tile_scan2   (itx_textpack.h) exclusive prefix sums of the tiles' lengths, 64 bit: where every tile's text starts, and the
//                  totals.
//   k_bed_write    one workgroup per tile, one lane per record. The tile's text is ONE contiguous range of the output; it is
//                  staged in LDS a window of BED_LDS bytes at a time and stored with 16-byte vectors (itx_textpack.h says why and
//                  how). itx_bed_write takes a byte range of a line, so a long XA string simply spans windows.
//
// "The host has to look" (nothing of the batch is emitted, the caller takes the host route): a read name without a NUL before
// the end of its record — the host's strdup then reads on into the next record, which is not modelled here.
//
// Byte and integer work, bound by the latency of the scattered record reads in k_bed_measure; the text leaves through pinned
// double buffers on a copy stream of its own, so that the copy of batch k and the host's fwrite overlap the kernels of batch
// k + 1 and the engine's work.
#include "itx_textpack.h"
#include "itx_derive.h"
#include "itx_bedline.h"
#include "itx_devbuf.h"

#include <string.h>

#include <string>
#include <vector>

#define BED_TILE 256u                // records per workgroup
#define BED_LDS 32768u               // bytes of text staged at a time: a tile of ordinary lines (256 x 70-120 bytes) in one window

struct BedDev {
    const int2 *tid;                 // [n_tid] (chromosome index or < 0, chromosome size)
    const uint2 *name;               // [n_tid] (offset into pool, length) of the renamed reference name
    const uint8_t *pool;
    int32_t n_tid;
    uint32_t want;                   // ITX_BED_ALL | ITX_BED_UNIQ
    ItxDeriveOpts o;
};

struct BedRecs {                     // the per-record arrays of the batch (device)
    const int32_t *tid, *pos, *end;
    const uint8_t *mapq, *f5;
    const int32_t *mpos, *isize;
};

struct BedFound {                    // what k_bed_measure keeps per record for k_bed_write
    uint32_t *len_b, *len_v, *qlen, *xa_off, *xa_len;
    int32_t *nm;
};

__global__ __launch_bounds__(BED_TILE) void k_bed_measure(BedDev D, const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, BedRecs R, uint32_t n, BedFound F,
                                                          unsigned long long *__restrict__ tile_sum, unsigned long long *__restrict__ tot)
{
    __shared__ unsigned long long s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BED_TILE + threadIdx.x;
    bool hard = false;
    if (i < n) {
        uint32_t lb = 0, lv = 0;
        ItxBedScan sc;
        sc.qname_len = 0;
        sc.xa_off = ITX_BED_NO_XA;
        sc.xa_len = 0;
        sc.nm = 0;
        const uint32_t f5 = R.f5[i];
        const int32_t t = R.tid[i];
        const int2 tr = (t >= 0 && t < D.n_tid) ? D.tid[t] : make_int2(-1, 0);
        ItxBedLine L;
        if (!(f5 & F5_NOLOOKUP) &&
            itx_derive(&D.o, tr.x, tr.y, f5, R.pos[i], R.end[i], R.mpos ? R.mpos[i] : 0, R.isize ? R.isize[i] : 0, &L.start, &L.end, &L.strand)) {
            sc = itx_bed_scan(u + rec_off[i], (D.want & 1u) != 0);
            hard = sc.hard;
            L.chr_len = D.name[t].y;
            L.qname_len = sc.qname_len;
            L.mapq = R.mapq[i];
            L.has_xa = sc.xa_off != ITX_BED_NO_XA;
            L.xa_len = sc.xa_len;
            L.nm = sc.nm;
            if (D.want & 1u) lb = itx_bed_len(&L, true);
            if ((D.want & 2u) && L.mapq >= D.o.mapq_min) lv = itx_bed_len(&L, false);
        }
        F.len_b[i] = lb;
        F.len_v[i] = lv;
        F.qlen[i] = sc.qname_len;
        F.xa_off[i] = sc.xa_off;
        F.xa_len[i] = sc.xa_len;
        F.nm[i] = sc.nm;
        if (lb) atomicAdd(&s_sum[0], (unsigned long long)lb);
        if (lv) atomicAdd(&s_sum[1], (unsigned long long)lv);
    }
    const unsigned long long hardm = __ballot(hard);
    if ((threadIdx.x & 63u) == 0 && hardm) atomicAdd(&tot[2], (unsigned long long)__popcll(hardm));
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

template <bool WITH_XA>
__global__ __launch_bounds__(BED_TILE) void k_bed_write(BedDev D, const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, BedRecs R, uint32_t n, BedFound F,
                                                        const unsigned long long *__restrict__ tile_base, uint8_t *__restrict__ out)
{
    __shared__ uint4 s_buf[BED_LDS / 16u];
    __shared__ uint32_t s_w[BED_TILE / 64u];
    const uint32_t i = blockIdx.x * BED_TILE + threadIdx.x;
    const uint32_t len = i < n ? (WITH_XA ? F.len_b[i] : F.len_v[i]) : 0u;
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<BED_TILE>(len, s_w, &total);
    const unsigned long long tb = tile_base[2u * blockIdx.x + (WITH_XA ? 0u : 1u)], te = tb + total;
    const unsigned long long mb = tb + moff, me = mb + len;
    ItxBedLine L;
    if (len) {
        const int32_t t = R.tid[i];                                   // in range: the record has a line
        const int2 tr = D.tid[t];
        (void)itx_derive(&D.o, tr.x, tr.y, R.f5[i], R.pos[i], R.end[i], R.mpos ? R.mpos[i] : 0, R.isize ? R.isize[i] : 0, &L.start, &L.end, &L.strand);
        const uint2 nm = D.name[t];
        const uint8_t *p = u + rec_off[i];
        L.chr = D.pool + nm.x;
        L.chr_len = nm.y;
        L.qname = p + 36;
        L.qname_len = F.qlen[i];
        L.mapq = R.mapq[i];
        const uint32_t xo = F.xa_off[i];
        L.has_xa = WITH_XA && xo != ITX_BED_NO_XA;
        L.xa = p + (L.has_xa ? xo : 0u);
        L.xa_len = F.xa_len[i];
        L.nm = F.nm[i];
    }
    itx_pack_tile<BED_TILE, BED_LDS>(s_buf, out, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) { itx_bed_write(&L, WITH_XA, dst, from, to); });
}

struct BedSlot {
    ItxBuf d_out[2];                   // [0] -B, [1] -V
    ItxPin h_out[2];
    uint64_t bytes[2];
    int started;
    ItxEvent ev[5];                    // measure: 0 .. 1, write: 2 .. 3, copies done: 4
};

struct itx_bed {
    int device;
    BedDev d;
    std::vector<int64_t> chrom_size;
    ItxBuf d_tid, d_name, d_pool;
    BedFound f;                        // views of f_mem
    ItxBuf f_mem[6];
    ItxBuf d_tile_sum, d_tile_base, d_tot;
    ItxPin h_tot;
    size_t cap;
    hipStream_t st, st_copy;
    BedSlot slot[2];
    int next, in_flight;
    itx_bed_stats stats;
};

#define BED_RC(call)                          \
    do {                                      \
        const int rc__ = (call);              \
        if (rc__ != ITX_OK) return rc__;      \
    } while (0)

extern "C" void itx_bed_destroy(itx_bed *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->st) (void)hipStreamSynchronize(b->st);
    if (b->st_copy) (void)hipStreamSynchronize(b->st_copy);
    if (b->st) (void)hipStreamDestroy(b->st);
    if (b->st_copy) (void)hipStreamDestroy(b->st_copy);
    delete b;
}

// fills the object; on a non-zero return the caller destroys what there is of it
static int bed_create(itx_bed *b, int device, const int64_t *chrom_size, int n_chrom, const itx_params *p, int want, size_t batch_capacity)
{
    const char *const who = "itx_bed_create";
    b->device = device;
    ITX_HIP(hipSetDevice(device));
    b->chrom_size.assign(chrom_size, chrom_size + n_chrom);
    b->cap = batch_capacity;
    b->d.want = (uint32_t)want;
    b->d.o.mapq_min = (uint32_t)p->mapq_min;
    b->d.o.extension = p->extension;
    b->d.o.isize_max = p->isize_max;
    b->d.o.treat = p->treat_pe_as_se;
    b->d.o.discard = p->discard_half_mapped;
    const size_t n = batch_capacity + 64, nt = (batch_capacity + BED_TILE - 1) / BED_TILE + 1;
    for (auto &m : b->f_mem) BED_RC(itx_buf_need(who, m, 4 * n));
    b->f = {b->f_mem[0].as<uint32_t>(), b->f_mem[1].as<uint32_t>(), b->f_mem[2].as<uint32_t>(), b->f_mem[3].as<uint32_t>(), b->f_mem[4].as<uint32_t>(),
            b->f_mem[5].as<int32_t>()};
    BED_RC(itx_buf_need(who, b->d_tile_sum, 16 * nt));
    BED_RC(itx_buf_need(who, b->d_tile_base, 16 * nt));
    BED_RC(itx_buf_need(who, b->d_tot, 32));
    BED_RC(itx_pin_need(who, b->h_tot, 32));
    ITX_HIP(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
    ITX_HIP(hipStreamCreateWithFlags(&b->st_copy, hipStreamNonBlocking));
    for (auto &s : b->slot)
        for (auto &e : s.ev) BED_RC(itx_event_make(e));
    return ITX_OK;
}

extern "C" int itx_bed_create(int device, const int64_t *chrom_size, int n_chrom, const itx_params *p, int want, size_t batch_capacity, itx_bed **out)
{
    if (!chrom_size || n_chrom < 0 || !p || !out || batch_capacity == 0 || batch_capacity > 0xffffff00u || !(want & (ITX_BED_ALL | ITX_BED_UNIQ)) ||
        (want & ~(ITX_BED_ALL | ITX_BED_UNIQ))) {
        itx_set_error("itx_bed_create: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    itx_bed *b = new itx_bed();
    const int rc = bed_create(b, device, chrom_size, n_chrom, p, want, batch_capacity);
    if (rc) {
        itx_bed_destroy(b);
        return rc;
    }
    *out = b;
    return ITX_OK;
}

/* the BAM header in use: tid2chrom as for itx_engine_set_tidmap, tid2name[t] the reference name after the -C rule (NULL: dropped) */
extern "C" int itx_bed_set_tidmap(itx_bed *b, const int32_t *tid2chrom, const char *const *tid2name, int n_tid)
{
    if (!b || n_tid < 0 || (n_tid && (!tid2chrom || !tid2name))) {
        itx_set_error("itx_bed_set_tidmap: bad argument");
        return ITX_E_ARG;
    }
    if (b->in_flight) {
        itx_set_error("itx_bed_set_tidmap: a batch has not been collected");
        return ITX_E_STATE;
    }
    ITX_HIP(hipSetDevice(b->device));
    std::vector<int2> v((size_t)n_tid + 1);
    std::vector<uint2> nm((size_t)n_tid + 1);
    std::string pool;
    for (int k = 0; k < n_tid; k++) {
        const int32_t c = tid2chrom[k];
        v[(size_t)k] = make_int2(c, (c >= 0 && (size_t)c < b->chrom_size.size()) ? (int32_t)b->chrom_size[(size_t)c] : 0);
        const char *s = tid2name[k] ? tid2name[k] : "";
        nm[(size_t)k] = make_uint2((uint32_t)pool.size(), (uint32_t)strlen(s));
        pool.append(s);
    }
    pool.append(16, '\0');
    ITX_HIP(hipStreamSynchronize(b->st));
    ITX_HIP(hipStreamSynchronize(b->st_copy));
    b->d.tid = nullptr;                                                     // (no map until the new one is whole)
    for (ItxBuf *old : {&b->d_tid, &b->d_name, &b->d_pool}) old->drop();
    BED_RC(itx_buf_need("itx_bed_set_tidmap", b->d_tid, sizeof(int2) * v.size()));
    BED_RC(itx_buf_need("itx_bed_set_tidmap", b->d_name, sizeof(uint2) * nm.size()));
    BED_RC(itx_buf_need("itx_bed_set_tidmap", b->d_pool, pool.size()));
    ITX_HIP(hipMemcpy(b->d_tid.p, v.data(), sizeof(int2) * v.size(), hipMemcpyHostToDevice));
    ITX_HIP(hipMemcpy(b->d_name.p, nm.data(), sizeof(uint2) * nm.size(), hipMemcpyHostToDevice));
    ITX_HIP(hipMemcpy(b->d_pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    b->d.tid = b->d_tid.as<int2>();
    b->d.name = b->d_name.as<uint2>();
    b->d.pool = b->d_pool.as<uint8_t>();
    b->d.n_tid = n_tid;
    return ITX_OK;
}

// measure + scan (waited for: the sizes decide the buffers), then write + copy enqueued into the next slot
int itx_bed_start(itx_bed *b, const uint8_t *u, const uint32_t *rec_off, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                  const uint8_t *f5, const int32_t *mpos, const int32_t *isize, size_t n, uint64_t *n_hard)
{
    if (!b || !n_hard || (n && (!u || !rec_off || !tid || !pos || !end || !mapq || !f5))) {
        itx_set_error("itx_bed: bad argument");
        return ITX_E_ARG;
    }
    if (n > b->cap || !b->d.tid || b->in_flight >= 2) {
        itx_set_error("itx_bed: %s", n > b->cap ? "batch exceeds the capacity" : !b->d.tid ? "no tid map" : "two batches are waiting to be collected");
        return ITX_E_STATE;
    }
    *n_hard = 0;
    ITX_HIP(hipSetDevice(b->device));
    BedSlot &s = b->slot[b->next];
    s.bytes[0] = s.bytes[1] = 0;
    const BedRecs R = {tid, pos, end, mapq, f5, mpos, isize};
    const uint32_t nt = (uint32_t)((n + BED_TILE - 1) / BED_TILE);
    unsigned long long *const d_tile_sum = b->d_tile_sum.as<unsigned long long>(), *const d_tile_base = b->d_tile_base.as<unsigned long long>(),
                             *const d_tot = b->d_tot.as<unsigned long long>(), *const h_tot = b->h_tot.as<unsigned long long>();
    ITX_HIP(hipEventRecord(s.ev[0], b->st));
    if (n) {
        ITX_HIP(hipMemsetAsync(d_tot, 0, 32, b->st));
        hipLaunchKernelGGL(k_bed_measure, dim3(nt), dim3(BED_TILE), 0, b->st, b->d, u, rec_off, R, (uint32_t)n, b->f, d_tile_sum, d_tot);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, b->st, d_tile_sum, nt, d_tile_base, d_tot);
        ITX_HIP(hipGetLastError());
    }
    ITX_HIP(hipEventRecord(s.ev[1], b->st));
    if (n) {
        const double t0 = itx_wall_now();
        ITX_HIP(hipMemcpyAsync(h_tot, d_tot, 32, hipMemcpyDeviceToHost, b->st));
        ITX_HIP(hipStreamSynchronize(b->st));
        b->stats.wait_s += itx_wall_now() - t0;
        if (h_tot[2]) {                                                 // the host has to look: nothing of this batch is emitted
            *n_hard = h_tot[2];
            b->stats.hard_batches++;
            return ITX_OK;
        }
        for (int k = 0; k < 2; k++) {
            const uint64_t need = h_tot[k];
            s.bytes[k] = need;
            const size_t want = (size_t)(need + need / 4 + 4096);
            if (need > s.d_out[k].cap && itx_buf_need("itx_bed", s.d_out[k], want) != ITX_OK) {
                itx_set_error("itx_bed: no device memory for %zu bytes of text", want);
                return ITX_E_NOMEM;
            }
            if (need > s.h_out[k].cap && itx_pin_need("itx_bed", s.h_out[k], want) != ITX_OK) {
                itx_set_error("itx_bed: no page-locked memory for %zu bytes of text", want);
                return ITX_E_NOMEM;
            }
        }
    }
    ITX_HIP(hipEventRecord(s.ev[2], b->st));
    if (s.bytes[0]) {
        hipLaunchKernelGGL(k_bed_write<true>, dim3(nt), dim3(BED_TILE), 0, b->st, b->d, u, rec_off, R, (uint32_t)n, b->f, d_tile_base, s.d_out[0].as<uint8_t>());
        ITX_HIP(hipGetLastError());
    }
    if (s.bytes[1]) {
        hipLaunchKernelGGL(k_bed_write<false>, dim3(nt), dim3(BED_TILE), 0, b->st, b->d, u, rec_off, R, (uint32_t)n, b->f, d_tile_base, s.d_out[1].as<uint8_t>());
        ITX_HIP(hipGetLastError());
    }
    ITX_HIP(hipEventRecord(s.ev[3], b->st));
    ITX_HIP(hipStreamWaitEvent(b->st_copy, s.ev[3], 0));
    for (int k = 0; k < 2; k++)
        if (s.bytes[k]) ITX_HIP(hipMemcpyAsync(s.h_out[k].p, s.d_out[k].p, s.bytes[k], hipMemcpyDeviceToHost, b->st_copy));
    ITX_HIP(hipEventRecord(s.ev[4], b->st_copy));
    s.started = 1;
    b->next ^= 1;
    b->in_flight++;
    return ITX_OK;
}

extern "C" int itx_bed_run(itx_bed *b, const void *d_bytes, const uint32_t *d_rec_off, const itx_batch *d_batch, size_t n, uint64_t *n_hard)
{
    if (!d_batch) {
        itx_set_error("itx_bed_run: bad argument");
        return ITX_E_ARG;
    }
    return itx_bed_start(b, (const uint8_t *)d_bytes, d_rec_off, d_batch->tid, d_batch->pos, d_batch->tmpend, d_batch->mapq, d_batch->flag5, d_batch->mpos, d_batch->isize, n,
                         n_hard);
}

extern "C" int itx_bed_wait_kernels(itx_bed *b)
{
    if (!b) {
        itx_set_error("itx_bed_wait_kernels: bad argument");
        return ITX_E_ARG;
    }
    ITX_HIP(hipSetDevice(b->device));
    const double t0 = itx_wall_now();
    ITX_HIP(hipStreamSynchronize(b->st));
    b->stats.wait_s += itx_wall_now() - t0;
    return ITX_OK;
}

extern "C" int itx_bed_collect(itx_bed *b, itx_bed_text *out)
{
    if (!b || !out) {
        itx_set_error("itx_bed_collect: bad argument");
        return ITX_E_ARG;
    }
    if (!b->in_flight) {
        itx_set_error("itx_bed_collect: no batch has been started");
        return ITX_E_STATE;
    }
    ITX_HIP(hipSetDevice(b->device));
    BedSlot &s = b->slot[(b->next + 2 - b->in_flight) & 1];
    const double t0 = itx_wall_now();
    ITX_HIP(hipEventSynchronize(s.ev[4]));
    b->stats.wait_s += itx_wall_now() - t0;
    float ma = 0, mw = 0;
    ITX_HIP(hipEventElapsedTime(&ma, s.ev[0], s.ev[1]));
    ITX_HIP(hipEventElapsedTime(&mw, s.ev[2], s.ev[3]));
    b->stats.kernel_ms += (double)ma + (double)mw;
    b->stats.batches++;
    b->stats.bytes += s.bytes[0] + s.bytes[1];
    out->all = s.h_out[0].as<const char>();
    out->all_bytes = s.bytes[0];
    out->uniq = s.h_out[1].as<const char>();
    out->uniq_bytes = s.bytes[1];
    s.started = 0;
    b->in_flight--;
    return ITX_OK;
}

extern "C" int itx_bed_get_stats(const itx_bed *b, itx_bed_stats *out)
{
    if (!b || !out) {
        itx_set_error("itx_bed_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *out = b->stats;
    return ITX_OK;
}
