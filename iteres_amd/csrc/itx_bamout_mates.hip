// itx_bamout_mates.hip — filter -b -s -m: the mates of the counted pairs join the sorted BAM (the rule: csrc/itx_materule.h).
// Without -T a proper pair is counted through its READ1 alone, so the held stream of -s has half of every counted fragment. With
// itx_bamout_mates_enable every batch also feeds a candidate store, and the first sort_next joins the wanted candidates to the held
// stream before the existing sort and replay run over the longer pool, untouched.
//
// per batch, behind the counted gather and k_bs_entries on bo->st (bm_batch, called by itx_bamout_start):
//   k_bm_measure   one lane per record: 4 + block_size for a candidate, else 0; the tile sums as k_bo_measure leaves them, and the
//                  highest tid among the candidates.
//   k_tile_scan2   the host waits for the totals and sizes the candidate store (two-phase growth, itx_devbuf.h) before anything is
//                  written to it.
//   k_bo_gather<uint32_t, false>  lays the candidates' bytes behind the candidate stream in HBM.
//   k_bm_entries   one lane per candidate: {tid, pos, h32(name), 64-bit offset, length} behind the candidate pool; places come
//                  from the tile bases and itx_tile_offsets, as in k_bs_entries.
// The candidate pass has lengths, tile sums, tile bases and totals of its own: the counted pass's are read by the host's totals step
// and by k_bs_entries. The candidate gather and k_bm_entries read the decoder's window, and the decoder takes the window back after
// itx_bamout_wait_kernels: that call therefore waits for mev[1], recorded behind k_bm_entries, as well as for the counted gather.
// Host-route windows hand all their records to itx_bamout_mates_append_host, which applies the same header on the host and uploads
// bytes and entries behind what is there.
//
// at the first sort_next, before the sort (bm_join); everything is allocated, and the held stream and the pool are grown to their
// final size, before anything changes:
//   sort           (key, candidate number) pairs by itx_radixsort.h, stable: passes over h32, then pos, then tid (as many as -s counts).
//   k_bm_join      one lane per held counted record: wanted() -> binary search of the sorted keys for (mtid, mpos, h32), a walk over
//                  the run of equal keys (stream order, the sort is stable), match() on the two records' bytes, and on the first match
//                  atomicMin(sel[candidate], this entry's number). Wanted and found are counted per workgroup through LDS.
//   k_bm_total     the chosen candidates' bytes (with the tags' under -a) and number, for the one growth of the held stream and pool.
//   rounds of at most batch_capacity candidates, in candidate (= stream) order: k_bm_chosen (lengths, 64-bit offsets, rows, tile sums),
//                  k_tile_scan2, k_bo_gather<ull, ANN> from the candidate stream to the end of the held stream (under -a with the row
//                  of the earliest counted entry that chose the candidate), k_bm_append: the BoSortEnt entries behind the counted ones.
//   then the candidate stream, the pool and the join's arrays are freed.
// Plain C++ over bytes and integers; vector loads, stores and atomics. No kernel uses scratch (DESIGN.md has the figures).
#include "itx_bamout_priv.h"
#include "itx_bamsortrule.h"
#include "itx_devbuf.h"
#include "itx_materule.h"
#include "itx_radixsort.h"
#include "itx_textpack.h"

#include <stdlib.h>
#include <string.h>

struct BmCand {
    uint32_t tid, pos, h32, len;     // the key (itx_materule.h); 4 + block_size
    ull off;                         // the candidate's first byte in the candidate stream
};
static_assert(sizeof(BmCand) == 24, "BmCand");

#define BM_NONE 0xffffffffu          // sel: no counted record chose the candidate
#define BM_TOT_BYTES 64u

__global__ __launch_bounds__(BO_TILE) void k_bm_measure(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, uint32_t n, uint32_t *__restrict__ len_out,
                                                         ull *__restrict__ tile_sum, ull *__restrict__ tot)
{
    __shared__ ull s_sum[2];
    __shared__ uint32_t s_max;
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 2) s_max = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    if (i < n) {
        uint32_t len = 0;
        const uint8_t *p = u + rec_off[i];
        const uint32_t bs = itx_mate_u32(p);
        if (bs < BO_MAX_RECORD && itx_mate_candidate(p, 4u + bs)) {
            len = 4u + bs;
            atomicAdd(&s_sum[0], (ull)len);
            atomicAdd(&s_sum[1], 1ull);
            atomicMax(&s_max, itx_mate_u32(p + 4));
        }
        len_out[i] = len;
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
    if (threadIdx.x == 2 && s_max) atomicMax(&tot[2], (ull)s_max);
}

__global__ __launch_bounds__(BO_TILE) void k_bm_entries(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, uint32_t n, const uint32_t *__restrict__ len_in,
                                                         const ull *__restrict__ tile_base, ull stream_at, ull ent_at, BmCand *__restrict__ ent)
{
    __shared__ uint32_t s_w[BO_TILE / 64u], s_c[BO_TILE / 64u];
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0, count = 0;
    const uint32_t moff = itx_tile_offsets<BO_TILE>(len, s_w, &total);
    const uint32_t rank = itx_tile_offsets<BO_TILE>(len ? 1u : 0u, s_c, &count);
    if (len) {
        const ItxMateKey k = itx_mate_key_candidate(u + rec_off[i]);
        BmCand e;
        e.tid = k.tid;
        e.pos = k.pos;
        e.h32 = k.h32;
        e.len = len;
        e.off = stream_at + tile_base[2u * blockIdx.x] + moff;
        ent[ent_at + tile_base[2u * blockIdx.x + 1u] + rank] = e;
    }
}

// the pairs the radix sort moves: (h32, the candidate's number); then the key becomes pos, then tid
__global__ __launch_bounds__(256) void k_bm_keys(const BmCand *__restrict__ ent, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = make_uint2(ent[i].h32, i);
}

__global__ __launch_bounds__(256) void k_bm_rekey(const BmCand *__restrict__ ent, uint32_t n, uint2 *__restrict__ keys, int by_tid)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const BmCand e = ent[keys[i].y];
        keys[i].x = by_tid ? e.tid : e.pos;
    }
}

__device__ __forceinline__ int bm_cmp(const BmCand &e, const ItxMateKey &k)
{
    ItxMateKey c;
    c.tid = e.tid;
    c.pos = e.pos;
    c.h32 = e.h32;
    return itx_mate_key_cmp(&c, &k);
}

// cnt[0] wanted, cnt[1] found
__global__ __launch_bounds__(256) void k_bm_join(const BoSortEnt *__restrict__ ent, uint32_t n_ent, const uint8_t *__restrict__ held, const uint2 *__restrict__ sorted,
                                                  const BmCand *__restrict__ cent, uint32_t n_cand, const uint8_t *__restrict__ cand, uint32_t *__restrict__ sel,
                                                  ull *__restrict__ cnt)
{
    __shared__ uint32_t s_c[2];
    if (threadIdx.x < 2) s_c[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_ent) {
        const BoSortEnt e = ent[i];
        const uint8_t *r = held + e.off;
        if (itx_mate_wanted(r, e.len)) {
            atomicAdd(&s_c[0], 1u);
            if (itx_mate_whole(r, e.len)) {
                const ItxMateKey k = itx_mate_key_wanted(r);
                uint32_t lo = 0, hi = n_cand;                              // the first sorted candidate whose key is not below k
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2u;
                    if (bm_cmp(cent[sorted[mid].y], k) < 0) lo = mid + 1u;
                    else hi = mid;
                }
                for (; lo < n_cand; lo++) {
                    const uint32_t c = sorted[lo].y;
                    const BmCand ce = cent[c];
                    if (bm_cmp(ce, k) != 0) break;
                    if (itx_mate_match(r, e.len, cand + ce.off, ce.len)) {
                        atomicMin(&sel[c], i);
                        atomicAdd(&s_c[1], 1u);
                        break;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_c[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (ull)s_c[threadIdx.x]);
}

// the length candidate c leaves with: its own and, under -a, the tags of the row of the counted entry that chose it; 0: not chosen.
// *bad: the row lies outside the table, or the record with its tags reaches BO_MAX_RECORD.
__device__ __forceinline__ uint32_t bm_chosen_len(const uint32_t *__restrict__ sel, const BmCand *__restrict__ cent, const BoSortEnt *__restrict__ ent, uint32_t c, bool ann_on,
                                                  const BoAnn &ann, uint32_t *row, bool *bad)
{
    const uint32_t s = sel[c];
    *bad = false;
    *row = 0;
    if (s == BM_NONE) return 0u;
    uint32_t len = cent[c].len;
    if (ann_on) {
        *row = ent[s].pad;
        if (*row >= ann.n_rows) {
            *bad = true;
            return 0u;
        }
        const ItxRepTag t = bo_row_tag(ann, *row);
        len += itx_reptag_len(&t);
        if (len - 4u >= BO_MAX_RECORD) {
            *bad = true;
            return 0u;
        }
    }
    return len;
}

// tot[2] bytes, tot[3] candidates chosen, tot[4] bad ones
__global__ __launch_bounds__(256) void k_bm_total(const uint32_t *__restrict__ sel, const BmCand *__restrict__ cent, const BoSortEnt *__restrict__ ent, uint32_t n_cand, int ann_on,
                                                   BoAnn ann, ull *__restrict__ tot)
{
    __shared__ ull s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < n_cand) {
        uint32_t row;
        bool bad;
        const uint32_t len = bm_chosen_len(sel, cent, ent, c, ann_on != 0, ann, &row, &bad);
        if (len) {
            atomicAdd(&s_sum[0], (ull)len);
            atomicAdd(&s_sum[1], 1ull);
        }
        if (bad) atomicAdd(&s_sum[2], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&tot[2u + threadIdx.x], s_sum[threadIdx.x]);
}

// one round, candidates c0 .. c0 + n: lengths, where they lie in the candidate stream and their rows, for the gather; a tile's bytes
// and records as k_bo_measure leaves them
__global__ __launch_bounds__(BO_TILE) void k_bm_chosen(const uint32_t *__restrict__ sel, const BmCand *__restrict__ cent, const BoSortEnt *__restrict__ ent, uint32_t c0, uint32_t n,
                                                        int ann_on, BoAnn ann, uint32_t *__restrict__ len_out, ull *__restrict__ off_out, int32_t *__restrict__ row_out,
                                                        ull *__restrict__ tile_sum)
{
    __shared__ ull s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    if (i < n) {
        uint32_t row;
        bool bad;
        const uint32_t len = bm_chosen_len(sel, cent, ent, c0 + i, ann_on != 0, ann, &row, &bad);
        len_out[i] = len;
        off_out[i] = cent[c0 + i].off;
        row_out[i] = (int32_t)row;
        if (len) {
            atomicAdd(&s_sum[0], (ull)len);
            atomicAdd(&s_sum[1], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

// behind a round's gather: the BoSortEnt of every chosen candidate behind those of the pool (k_bs_entries' arrangement); flag[1] is
// the highest tid, which counts the sort's tid passes. A candidate has tid >= 0 and pos >= 0: none can be unsortable.
__global__ __launch_bounds__(BO_TILE) void k_bm_append(const uint8_t *__restrict__ cand, const ull *__restrict__ off_in, uint32_t n, const uint32_t *__restrict__ len_in,
                                                        const int32_t *__restrict__ row_in, const ull *__restrict__ tile_base, ull stream_at, ull ent_at, BoSortEnt *__restrict__ ent,
                                                        uint32_t *__restrict__ flag)
{
    __shared__ uint32_t s_w[BO_TILE / 64u], s_c[BO_TILE / 64u], s_max;
    if (threadIdx.x == 0) s_max = 0;                                       // (the barriers of itx_tile_offsets order this)
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0, count = 0;
    const uint32_t moff = itx_tile_offsets<BO_TILE>(len, s_w, &total);
    const uint32_t rank = itx_tile_offsets<BO_TILE>(len ? 1u : 0u, s_c, &count);
    if (len) {
        ItxBamSortKey k;
        (void)itx_bamsort_key(cand + off_in[i], ITX_MATE_FIXED, &k);
        BoSortEnt e;
        e.tid = itx_bamsort_high(&k);
        e.low = itx_bamsort_low(&k);
        e.off = stream_at + tile_base[2u * blockIdx.x] + moff;
        e.len = len;
        e.pad = (uint32_t)row_in[i];
        ent[ent_at + tile_base[2u * blockIdx.x + 1u] + rank] = e;
        atomicMax(&s_max, e.tid);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(&flag[1], s_max);
}

// ---- host side
void bm_destroy(itx_bamout *bo)
{
    (void)hipFree(bo->d_mlen);
    (void)hipFree(bo->d_mtile_sum);
    (void)hipFree(bo->d_mtile_base);
    (void)hipFree(bo->d_mtot);
    (void)hipFree(bo->d_moff64);
    (void)hipFree(bo->d_mrow);
    (void)hipFree(bo->d_cand);
    (void)hipFree(bo->d_cent);
    if (bo->h_mtot) (void)hipHostFree(bo->h_mtot);
    for (auto &e : bo->mev)
        if (e) (void)hipEventDestroy(e);
    free(bo->host_rows);
    bo->d_mlen = nullptr;
    bo->d_mtile_sum = bo->d_mtile_base = bo->d_mtot = bo->h_mtot = bo->d_moff64 = nullptr;
    bo->d_mrow = nullptr;
    bo->d_cand = nullptr;
    bo->d_cent = nullptr;
    bo->mev[0] = bo->mev[1] = nullptr;
    bo->host_rows = nullptr;
}

extern "C" int itx_bamout_mates_enable(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_mates_enable: bad argument");
        return ITX_E_ARG;
    }
    if (!bo->sort) {
        itx_set_error("itx_bamout_mates_enable: the mates join the held stream of a sort (itx_bamout_sort_enable first)");
        return ITX_E_STATE;
    }
    if (bo_not_begun(bo, "itx_bamout_mates_enable", bo->mates) != ITX_OK) return ITX_E_STATE;
    int rc = ITX_OK;
    const size_t n = bo->cap + 64, nt = (bo->cap + BO_TILE - 1) / BO_TILE + 1;
    ITX_TRY(hipSetDevice(bo->device));
    if (hipMalloc((void **)&bo->d_mlen, 4 * n) != hipSuccess || hipMalloc((void **)&bo->d_mtile_sum, 16 * nt) != hipSuccess ||
        hipMalloc((void **)&bo->d_mtile_base, 16 * nt) != hipSuccess || hipMalloc((void **)&bo->d_mtot, BM_TOT_BYTES) != hipSuccess ||
        hipMalloc((void **)&bo->d_moff64, 8 * n) != hipSuccess || hipMalloc((void **)&bo->d_mrow, 4 * n) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_mates_enable: no device memory for batches of %zu records (run without -m)", bo->cap);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipHostMalloc((void **)&bo->h_mtot, BM_TOT_BYTES, hipHostMallocDefault));
    ITX_TRY(hipEventCreate(&bo->mev[0]));
    ITX_TRY(hipEventCreate(&bo->mev[1]));
    bo->mates = 1;
    return ITX_OK;
out:
    bm_destroy(bo);
    return rc;
}

// room for `bytes` more candidate bytes and n_more more entries; bo->st is idle. What does not fit leaves the object as it was.
static int bm_reserve(itx_bamout *bo, ull bytes, ull n_more)
{
    const ull want_n = bo->n_cent + n_more, want_b = (ull)bo->cand_len + bytes;
    if (want_n >= 0xfffffffeull) {
        itx_set_error("itx_bamout: %llu candidate mates (run without -m)", want_n);
        return ITX_E_LIMIT;
    }
    const size_t new_b = want_b > bo->cand_cap ? (size_t)(want_b + want_b / 2) : 0;
    const ull new_n = want_n > bo->cent_cap ? want_n + want_n / 2 + 64 : 0;
    if (!new_b && !new_n) return ITX_OK;
    ItxGrow g[2] = {{(void **)&bo->d_cand, bo->cand_len, new_b ? new_b + 16 : 0}, {(void **)&bo->d_cent, sizeof(BmCand) * bo->n_cent, sizeof(BmCand) * new_n}};
    if (itx_grow_alloc(g, 2) >= 0) {
        itx_set_error("itx_bamout: no device memory for %llu candidate mates of %llu bytes beside a held stream of %zu bytes (run without -m)", want_n, want_b, bo->carry);
        return ITX_E_NOMEM;
    }
    const int rc = itx_grow_commit(bo->st, g, 2);
    if (rc != ITX_OK) return rc;
    if (new_b) {
        if (bo->cand_cap) bo->mstats.grows++;
        bo->cand_cap = new_b;
    }
    if (new_n) bo->cent_cap = new_n;
    return ITX_OK;
}

int bm_batch(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, uint32_t n)
{
    int rc = ITX_OK;
    const uint32_t nt = (n + BO_TILE - 1) / BO_TILE;
    ull bytes = 0, count = 0;
    ITX_TRY(hipEventRecord(bo->mev[0], bo->st));
    ITX_TRY(hipMemsetAsync(bo->d_mtot, 0, BM_TOT_BYTES, bo->st));
    hipLaunchKernelGGL(k_bm_measure, dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, n, bo->d_mlen, bo->d_mtile_sum, bo->d_mtot);
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_mtile_sum, nt, bo->d_mtile_base, bo->d_mtot);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipMemcpyAsync(bo->h_mtot, bo->d_mtot, 24, hipMemcpyDeviceToHost, bo->st));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));                              // (the counted gather is through as well)
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bo_read_gather_time(bo);
    bytes = bo->h_mtot[0];
    count = bo->h_mtot[1];
    if (count) {
        if ((rc = bm_reserve(bo, bytes, count)) != ITX_OK) goto out;
        if ((rc = bo_launch_gather_at(bo, 0, 0, u, rec_off, n, bo->d_mlen, bo->d_mtile_base, (ull)bo->cand_len, bo->d_cand, nullptr)) != ITX_OK) goto out;
        hipLaunchKernelGGL(k_bm_entries, dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, n, bo->d_mlen, bo->d_mtile_base, (ull)bo->cand_len, bo->n_cent, bo->d_cent);
        ITX_TRY(hipGetLastError());
        bo->cand_len += (size_t)bytes;
        bo->n_cent += count;
        if ((uint32_t)bo->h_mtot[2] > bo->cand_maxtid) bo->cand_maxtid = (uint32_t)bo->h_mtot[2];
        bo->mstats.candidates += count;
        bo->mstats.candidate_bytes += bytes;
    }
    ITX_TRY(hipEventRecord(bo->mev[1], bo->st));
    bo->mates_timed = 1;
out:
    return rc;
}

static int bm_collecting(const itx_bamout *bo, const char *fn)
{
    if (bo->mates == 1 && bo->sort == 1 && !bo->finished) return ITX_OK;
    itx_set_error("%s: %s", fn, bo->mates ? "the stream is being replayed in sorted order" : "no mates were asked for (itx_bamout_mates_enable)");
    return ITX_E_STATE;
}

extern "C" int itx_bamout_mates_append_host(itx_bamout *bo, const void *bytes, size_t len)
{
    if (!bo || (len && !bytes)) {
        itx_set_error("itx_bamout_mates_append_host: bad argument");
        return ITX_E_ARG;
    }
    if (bm_collecting(bo, "itx_bamout_mates_append_host") != ITX_OK) return ITX_E_STATE;
    const uint8_t *b = (const uint8_t *)bytes;
    size_t n_rec = 0, n_cand = 0, cand_bytes = 0;
    for (size_t at = 0, next = 0; at < len; at = next) {                    // whole records, or nothing is appended
        if (itx_mate_next(b, len, at, &next)) {
            itx_set_error("itx_bamout_mates_append_host: the bytes are not whole records (record %zu at byte %zu of %zu)", n_rec, at, len);
            return ITX_E_ARG;
        }
        if (itx_mate_candidate(b + at, (uint32_t)(next - at))) {
            n_cand++;
            cand_bytes += next - at;
        }
        n_rec++;
    }
    if (!n_cand) return ITX_OK;
    int rc = ITX_OK;
    uint32_t maxtid = 0;
    uint8_t *h_bytes = (uint8_t *)malloc(cand_bytes);
    BmCand *h_ent = (BmCand *)malloc(sizeof(BmCand) * n_cand);
    if (!h_bytes || !h_ent) {
        itx_set_error("itx_bamout_mates_append_host: no memory for %zu candidate mates", n_cand);
        rc = ITX_E_NOMEM;
        goto out;
    }
    {
        size_t k = 0, w = 0;
        for (size_t at = 0, next = 0; at < len; at = next) {
            (void)itx_mate_next(b, len, at, &next);
            if (!itx_mate_candidate(b + at, (uint32_t)(next - at))) continue;
            const ItxMateKey key = itx_mate_key_candidate(b + at);
            h_ent[k].tid = key.tid;
            h_ent[k].pos = key.pos;
            h_ent[k].h32 = key.h32;
            h_ent[k].len = (uint32_t)(next - at);
            h_ent[k].off = (ull)bo->cand_len + w;
            if (key.tid > maxtid) maxtid = key.tid;
            memcpy(h_bytes + w, b + at, next - at);
            w += next - at;
            k++;
        }
    }
    ITX_TRY(hipSetDevice(bo->device));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));                              // device batches before this one have their place
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bo_read_gather_time(bo);
    if ((rc = bm_reserve(bo, cand_bytes, n_cand)) != ITX_OK) goto out;
    ITX_TRY(hipMemcpyAsync(bo->d_cand + bo->cand_len, h_bytes, cand_bytes, hipMemcpyHostToDevice, bo->st));
    ITX_TRY(hipMemcpyAsync(bo->d_cent + bo->n_cent, h_ent, sizeof(BmCand) * n_cand, hipMemcpyHostToDevice, bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));                                  // the staging bytes are freed below
    bo->cand_len += cand_bytes;
    bo->n_cent += n_cand;
    if (maxtid > bo->cand_maxtid) bo->cand_maxtid = maxtid;
    bo->mstats.candidates += n_cand;
    bo->mstats.candidate_bytes += cand_bytes;
out:
    free(h_bytes);
    free(h_ent);
    return rc;
}

extern "C" int itx_bamout_mates_host_rows(itx_bamout *bo, const int32_t *rows, size_t n)
{
    if (!bo || (n && !rows)) {
        itx_set_error("itx_bamout_mates_host_rows: bad argument");
        return ITX_E_ARG;
    }
    if (bm_collecting(bo, "itx_bamout_mates_host_rows") != ITX_OK) return ITX_E_STATE;
    if (bo->annotate)
        for (size_t i = 0; i < n; i++)
            if (rows[i] < 0 || (uint32_t)rows[i] >= bo->ann.n_rows) {
                itx_set_error("itx_bamout_mates_host_rows: record %zu chose row %d of %u", i, rows[i], bo->ann.n_rows);
                return ITX_E_ARG;
            }
    int32_t *copy = (int32_t *)malloc(4 * (n ? n : 1));
    if (!copy) {
        itx_set_error("itx_bamout_mates_host_rows: no memory for %zu rows", n);
        return ITX_E_NOMEM;
    }
    if (n) memcpy(copy, rows, 4 * n);
    free(bo->host_rows);
    bo->host_rows = copy;
    bo->n_host_rows = n;
    return ITX_OK;
}

// the candidate store goes (the kernels that read it are through)
static void bm_release(itx_bamout *bo)
{
    (void)hipFree(bo->d_cand);
    (void)hipFree(bo->d_cent);
    bo->d_cand = nullptr;
    bo->d_cent = nullptr;
    bo->cand_cap = bo->cand_len = 0;
    bo->cent_cap = 0;
    bo->mates = 2;
}

int bm_join(itx_bamout *bo)
{
    int rc = ITX_OK;
    const uint32_t N = (uint32_t)bo->n_sent, C = (uint32_t)bo->n_cent;
    uint2 *k0 = nullptr, *k1 = nullptr, *sorted = nullptr;
    uint32_t *hist = nullptr, *sel = nullptr, n_ref = 0, high = 0;
    ull *tot = nullptr, sel_bytes = 0, sel_count = 0;
    float ms = 0;
    if (!N) {                                                              // nothing was counted: nothing is wanted
        bm_release(bo);
        return ITX_OK;
    }
    if (hipMalloc((void **)&tot, BM_TOT_BYTES) != hipSuccess ||
        (C && (hipMalloc((void **)&k0, 8 * (size_t)C) != hipSuccess || hipMalloc((void **)&k1, 8 * (size_t)C) != hipSuccess ||
               hipMalloc((void **)&hist, itx_sort_hist_bytes(C)) != hipSuccess || hipMalloc((void **)&sel, 4 * (size_t)C) != hipSuccess))) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_sort_next: no device memory to join %u candidate mates to %u held records (run without -m)", C, N);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipEventRecord(bo->mev[0], bo->st));
    ITX_TRY(hipMemsetAsync(tot, 0, BM_TOT_BYTES, bo->st));
    if (C) {
        ITX_TRY(hipMemsetAsync(sel, 0xff, 4 * (size_t)C, bo->st));
        n_ref = bo->n_ref > 0 ? (uint32_t)bo->n_ref : 0u;
        if (bo->cand_maxtid + 1u > n_ref) n_ref = bo->cand_maxtid + 1u;
        high = itx_bamsort_high_passes(n_ref);
        hipLaunchKernelGGL(k_bm_keys, dim3((C + 255u) / 256u), dim3(256), 0, bo->st, bo->d_cent, C, k0);
        ITX_TRY(hipGetLastError());
        if ((rc = itx_sort_run(bo->st, k0, k1, C, 0u, 4u, hist, &sorted)) != ITX_OK) goto out;
        hipLaunchKernelGGL(k_bm_rekey, dim3((C + 255u) / 256u), dim3(256), 0, bo->st, bo->d_cent, C, sorted, 0);
        ITX_TRY(hipGetLastError());
        if ((rc = itx_sort_run(bo->st, sorted, sorted == k0 ? k1 : k0, C, 0u, 4u, hist, &sorted)) != ITX_OK) goto out;
        if (high) {
            hipLaunchKernelGGL(k_bm_rekey, dim3((C + 255u) / 256u), dim3(256), 0, bo->st, bo->d_cent, C, sorted, 1);
            ITX_TRY(hipGetLastError());
            if ((rc = itx_sort_run(bo->st, sorted, sorted == k0 ? k1 : k0, C, 0u, high, hist, &sorted)) != ITX_OK) goto out;
        }
    }
    hipLaunchKernelGGL(k_bm_join, dim3((N + 255u) / 256u), dim3(256), 0, bo->st, bo->d_sent, N, bo->d_pay, sorted, bo->d_cent, C, bo->d_cand, sel, tot);
    ITX_TRY(hipGetLastError());
    if (C) {
        hipLaunchKernelGGL(k_bm_total, dim3((C + 255u) / 256u), dim3(256), 0, bo->st, sel, bo->d_cent, bo->d_sent, C, bo->annotate, bo->ann, tot);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipMemcpyAsync(bo->h_mtot, tot, 40, hipMemcpyDeviceToHost, bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));
    sel_bytes = bo->h_mtot[2];
    sel_count = bo->h_mtot[3];
    if (bo->h_mtot[4]) {
        itx_set_error("itx_bamout_sort_next: %llu mates whose READ1 names no row of the table, or that reach a gibibyte with their tags", bo->h_mtot[4]);
        rc = ITX_E_ARG;
        goto out;
    }
    // the held stream and the pool take their final size here: the rounds below cannot run out of memory
    if ((rc = bo_reserve(bo, (ull)bo->carry + sel_bytes, 0)) != ITX_OK) goto out;
    if ((rc = bs_reserve(bo, sel_count)) != ITX_OK) goto out;
    bo->mstats.wanted = bo->h_mtot[0];
    bo->mstats.found = bo->h_mtot[1];
    for (ull c0 = 0; sel_count && c0 < C; c0 += bo->cap) {
        const uint32_t n = (uint32_t)(C - c0 < bo->cap ? C - c0 : bo->cap), nt = (n + BO_TILE - 1) / BO_TILE;
        hipLaunchKernelGGL(k_bm_chosen, dim3(nt), dim3(BO_TILE), 0, bo->st, sel, bo->d_cent, bo->d_sent, (uint32_t)c0, n, bo->annotate, bo->ann, bo->d_mlen, bo->d_moff64,
                           bo->d_mrow, bo->d_mtile_sum);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_mtile_sum, nt, bo->d_mtile_base, bo->d_mtot);
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(bo->h_mtot, bo->d_mtot, 16, hipMemcpyDeviceToHost, bo->st));
        ITX_TRY(hipStreamSynchronize(bo->st));
        const ull bytes = bo->h_mtot[0], count = bo->h_mtot[1];
        if (!count) continue;
        if ((ull)bo->carry + bytes > bo->pay_cap || bo->n_sent + count > bo->sent_cap) {
            itx_set_error("itx_bamout_sort_next: the chosen mates outgrow what was counted for them");
            rc = ITX_E_LIMIT;
            goto out;
        }
        if ((rc = bo_launch_gather_at(bo, 1, bo->annotate, bo->d_cand, bo->d_moff64, n, bo->d_mlen, bo->d_mtile_base, (ull)bo->carry, bo->d_pay, bo->d_mrow)) != ITX_OK) goto out;
        hipLaunchKernelGGL(k_bm_append, dim3(nt), dim3(BO_TILE), 0, bo->st, bo->d_cand, bo->d_moff64, n, bo->d_mlen, bo->d_mrow, bo->d_mtile_base, (ull)bo->carry, bo->n_sent,
                           bo->d_sent, bo->d_sflag);
        ITX_TRY(hipGetLastError());
        bo->carry += (size_t)bytes;
        bo->n_sent += count;
    }
    ITX_TRY(hipEventRecord(bo->mev[1], bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));
    if (hipEventElapsedTime(&ms, bo->mev[0], bo->mev[1]) == hipSuccess) bo->mstats.join_ms += (double)ms;
    bm_release(bo);
out:
    if (rc != ITX_OK) (void)hipStreamSynchronize(bo->st);                  // (kernels that were enqueued before something failed)
    (void)hipFree(tot);
    (void)hipFree(k0);
    (void)hipFree(k1);
    (void)hipFree(hist);
    (void)hipFree(sel);
    return rc;
}

extern "C" int itx_bamout_mates_get_stats(const itx_bamout *bo, itx_bamout_mates_stats *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_mates_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *out = bo->mstats;
    return ITX_OK;
}
