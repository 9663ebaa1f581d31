// itx_bamout.hip — the BAM of `iteres filter -b` (an extension: the reference has no such output) built where the records lie:
// every record of a batch that chose a table row goes, block_size and bytes unchanged and in file order, into one stream of
// payload bytes in HBM; every ITX_BAMOUT_PAYLOAD bytes of that stream become one BGZF member (itx_bgzfmember.h), and only the
// members, compressed and packed, cross the link back. The header's members and the EOF marker are the host's (bamout.c).
// This file has the object and the batch path; itx_bamout_priv.h is what the writer's files share.
//
// per batch (records in device memory, the chosen rows in d_hit_row):
//   k_bo_measure   one lane per record: 4 + block_size for a record with hit_row >= 0, else 0. A tile of BO_TILE records adds up
//                  its bytes (64 bit) and its records.
//   k_tile_scan2   (itx_textpack.h) exclusive sums over the tiles, one workgroup; the totals are all the host waits for: they
//                  say how many whole payloads the stream now holds, and every buffer is sized before anything is written.
//   k_bo_gather    one workgroup per tile: the tile's records are ONE contiguous range of the stream, behind what the call before
//                  left over; staged in LDS a window at a time and stored with 16-byte vectors (itx_textpack.h says why and how).
//   bo_emit        (itx_bamout_members.hip) one wave per whole payload makes it a member, at the level of filter -b -l; the
//                  members' sizes are scanned and the members packed one behind the other; the stream's rest, less than one
//                  payload, moves to its front, and the packed total follows to the host.
// itx_bamout_collect hands a batch's members out: it waits for that batch's kernels only (the next batch's are queued behind them
// and go on), copies the packed bytes on the copy stream into one of two page-locked buffers, and the host writes them to the file
// while the next batch's kernels run — the bed route's arrangement.
// What the host route counted joins the same stream in stream order (itx_bamout_append_host), so the file is one ordered stream
// whatever route a window took. itx_bamout_finish makes the last, short payload a member.
// With itx_bamout_index_enable (filter -b -i) the stream's .bai index is collected beside it and made at the end
// (csrc/itx_bamidx.hip): an entry per counted record behind every gather, every batch's member sizes behind those before.
//
// With itx_bamout_sort_enable (filter -b -s, itx_bamout_sort.hip) the stream is held whole instead of being cut: every gather
// appends to it and an entry per record to a pool (bs_entries); after the last batch itx_bamout_sort_next replays the records in
// sorted order through bo_totals, bo_launch_gather and bo_emit of the path above.
//
// With itx_bamout_annotate_enable (filter -b -a, itx_bamout_annotate.hip) a counted record leaves with the tags of its row behind it
// (csrc/itx_reptag.h): k_bo_measure<true> adds the tags' length, a function of the row alone, k_bo_gather<uint32_t, true> lays the
// record with itx_reptag_write in place of the byte copy. Everything behind the gather sees a longer record: the members, the index's
// chunks, the held stream of -s (annotated at the first gather; the replay copies byte for byte). Without the call the <false>
// instantiations run.
//
// With itx_bamout_mates_enable (filter -b -s -m, itx_bamout_mates.hip) a batch's candidate mates are gathered into a store of their
// own behind the counted gather (bm_batch), and the first sort_next joins the wanted ones to the held stream (bm_join).
//
// Every buffer that grows (bo_reserve) grows by the two-phase rule of itx_devbuf.h.
// Byte and integer work. No kernel of this file uses scratch (DESIGN.md has the figures).
#include "itx_bamout_priv.h"
#include "itx_bamsortrule.h"
#include "itx_devbuf.h"
#include "itx_textpack.h"

#include <stdlib.h>
#include <string.h>

// ANN: the record's length includes the tags of its row (a row outside the table counts as bad, as a record too long does)
template <bool ANN>
__global__ __launch_bounds__(BO_TILE) void k_bo_measure(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, const int32_t *__restrict__ hit_row,
                                                         uint32_t n, uint32_t *__restrict__ len_out, ull *__restrict__ tile_sum, ull *__restrict__ tot, BoAnn ann)
{
    __shared__ ull s_sum[ANN ? 3 : 2];                                     // bytes, records; ANN: and the tag bytes among them
    if (threadIdx.x < (ANN ? 3 : 2)) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    bool bad = false, bad_row = false;
    if (i < n) {
        uint32_t len = 0;
        if (hit_row[i] >= 0) {
            const uint8_t *p = u + rec_off[i];
            const uint32_t bs = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            bad = bs >= BO_MAX_RECORD;
            uint32_t tag = 0;
            if constexpr (ANN) {
                bad_row = (uint32_t)hit_row[i] >= ann.n_rows;
                if (!bad && !bad_row) {
                    const ItxRepTag t = bo_row_tag(ann, (uint32_t)hit_row[i]);
                    tag = itx_reptag_len(&t);                              // (below 2^18: three names below 2^16 each)
                    bad = bs + tag >= BO_MAX_RECORD;
                }
            }
            if (!bad && !bad_row) {
                len = 4u + bs + tag;
                atomicAdd(&s_sum[0], (ull)len);
                atomicAdd(&s_sum[1], 1ull);
                if constexpr (ANN) atomicAdd(&s_sum[2], (ull)tag);
            }
        }
        len_out[i] = len;
    }
    const ull badm = __ballot(bad);
    if ((threadIdx.x & 63u) == 0 && badm) atomicAdd(&tot[2], (ull)__popcll(badm));
    if constexpr (ANN) {
        const ull rowm = __ballot(bad_row);
        if ((threadIdx.x & 63u) == 0 && rowm) atomicAdd(&tot[3], (ull)__popcll(rowm));
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
    if constexpr (ANN) {
        if (threadIdx.x == 2 && s_sum[2]) atomicAdd(&tot[4], s_sum[2]);
    }
}

// OFF: uint32_t offsets into a window; 64-bit offsets into the held stream (the replay of filter -b -s)
// ANN: len_in are annotated lengths and the record is laid with its row's tags behind it (hit_row and ann are read only then)
template <class OFF, bool ANN>
__global__ __launch_bounds__(BO_TILE) void k_bo_gather(const uint8_t *__restrict__ u, const OFF *__restrict__ rec_off, uint32_t n,
                                                        const uint32_t *__restrict__ len_in, const ull *__restrict__ tile_base, ull base, uint8_t *__restrict__ pay,
                                                        const int32_t *__restrict__ hit_row, BoAnn ann)
{
    __shared__ uint4 s_buf[BO_LDS / 16u];
    __shared__ uint32_t s_w[BO_TILE / 64u];
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<BO_TILE>(len, s_w, &total);
    const ull tb = base + tile_base[2u * blockIdx.x], te = tb + total;
    const ull mb = tb + moff, me = mb + len;
    const uint8_t *src = len ? u + rec_off[i] : u;
    if constexpr (ANN) {
        // the measure pass has checked the row; the names are a few cached bytes per lane, read where they are laid
        ItxRepTag t = {};
        if (len) t = bo_row_tag(ann, (uint32_t)hit_row[i]);
        const uint32_t rec_len = len - (len ? itx_reptag_len(&t) : 0u);
        itx_pack_tile<BO_TILE, BO_LDS>(s_buf, pay, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) { itx_reptag_write(src, rec_len, &t, from, to, dst); });
    } else {
        itx_pack_tile<BO_TILE, BO_LDS>(s_buf, pay, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) {
            // a record starts wherever the one before it ended: kept a byte loop (names' gather says why)
#pragma clang loop vectorize(disable)
            for (uint32_t k = from; k < to; k++) dst[k - from] = src[k];
        });
    }
}

// ---- host side
extern "C" void itx_bamout_destroy(itx_bamout *bo)
{
    if (!bo) return;
    (void)hipSetDevice(bo->device);
    if (bo->st) (void)hipStreamSynchronize(bo->st);
    if (bo->cst) (void)hipStreamSynchronize(bo->cst);
    for (auto &e : bo->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &s : bo->slot) {
        if (s.e0) (void)hipEventDestroy(s.e0);
        if (s.e1) (void)hipEventDestroy(s.e1);
        (void)hipFree(s.d_packed);
        if (s.h_pin) (void)hipHostFree(s.h_pin);
        if (s.h_total) (void)hipHostFree(s.h_total);
    }
    if (bo->st) (void)hipStreamDestroy(bo->st);
    if (bo->cst) (void)hipStreamDestroy(bo->cst);
    (void)hipFree(bo->d_hits);
    (void)hipFree(bo->d_len);
    (void)hipFree(bo->d_tile_sum);
    (void)hipFree(bo->d_tile_base);
    (void)hipFree(bo->d_tot);
    (void)hipFree(bo->d_pay);
    (void)hipFree(bo->d_mem);
    (void)hipFree(bo->d_msize);
    (void)hipFree(bo->d_moff);
    if (bo->h_tot) (void)hipHostFree(bo->h_tot);
    for (auto &e : bo->sev)
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(bo->d_sent);
    (void)hipFree(bo->d_sflag);
    if (bo->h_sflag) (void)hipHostFree(bo->h_sflag);
    (void)hipFree(bo->d_held);
    (void)hipFree(bo->d_k0);
    (void)hipFree(bo->d_k1);
    (void)hipFree(bo->d_hist);
    (void)hipFree(bo->d_soff);
    (void)hipFree(bo->d_ann);
    bm_destroy(bo);
    itx_bamidx_destroy(bo->ix);
    delete bo;
}

extern "C" int itx_bamout_create(int device, size_t batch_capacity, size_t stream_bytes, itx_bamout **out)
{
    if (!out || batch_capacity == 0 || batch_capacity > 0xffffff00u) {
        itx_set_error("itx_bamout_create: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    int rc = ITX_OK;
    itx_bamout *bo = new itx_bamout();
    bo->device = device;
    bo->cap = batch_capacity;
    bo->n_ref = -1;
    bo->level = 6;
    const size_t n = batch_capacity + 64, nt = (batch_capacity + BO_TILE - 1) / BO_TILE + 1;
    if (stream_bytes < 4 * (size_t)BO_P) stream_bytes = 4 * (size_t)BO_P;
    bo->pay_cap = stream_bytes;
    ITX_TRY(hipSetDevice(device));
    if (hipMalloc((void **)&bo->d_hits, 4 * n) != hipSuccess || hipMalloc((void **)&bo->d_len, 4 * n) != hipSuccess ||
        hipMalloc((void **)&bo->d_tile_sum, 16 * nt) != hipSuccess || hipMalloc((void **)&bo->d_tile_base, 16 * nt) != hipSuccess ||
        hipMalloc((void **)&bo->d_tot, BO_TOT_BYTES) != hipSuccess || hipMalloc((void **)&bo->d_pay, bo->pay_cap + 16) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_create: no device memory for batches of %zu records and a stream of %zu bytes", batch_capacity, stream_bytes);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipHostMalloc((void **)&bo->h_tot, BO_TOT_BYTES, hipHostMallocDefault));
    ITX_TRY(hipStreamCreateWithFlags(&bo->st, hipStreamNonBlocking));
    ITX_TRY(hipStreamCreateWithFlags(&bo->cst, hipStreamNonBlocking));
    for (auto &e : bo->ev) ITX_TRY(hipEventCreate(&e));
    for (auto &s : bo->slot) {
        ITX_TRY(hipEventCreate(&s.e0));
        ITX_TRY(hipEventCreate(&s.e1));
        ITX_TRY(hipHostMalloc((void **)&s.h_total, 16, hipHostMallocDefault));
    }
out:
    if (rc != ITX_OK) {
        itx_bamout_destroy(bo);
        return rc;
    }
    *out = bo;
    return ITX_OK;
}

extern "C" int32_t *itx_bamout_hits(itx_bamout *bo) { return bo ? bo->d_hits : nullptr; }
extern "C" void *itx_bamout_stream(itx_bamout *bo) { return bo ? (void *)bo->st : nullptr; }

// ---- the steps the writer's files share (itx_bamout_priv.h says who calls each, and when)
int bo_not_begun(const itx_bamout *bo, const char *fn, int already)
{
    if (!already && !bo->finished && !bo->stats.batches && !bo->stats.host_batches) return ITX_OK;
    itx_set_error("%s: %s", fn, already ? "called twice" : "the stream has begun");
    return ITX_E_STATE;
}

void bo_read_gather_time(itx_bamout *bo)
{
    if (bo->ix) itx_bamidx_batch_time(bo->ix);
    if (!bo->gather_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, bo->ev[2], bo->ev[3]) == hipSuccess) *(bo->sort == 2 ? &bo->replay_ms : &bo->stats.gather_ms) += (double)ms;
    bo->gather_timed = 0;
}

int bo_totals(itx_bamout *bo, uint32_t nt, size_t tot_bytes, double *acc_ms)
{
    int rc = ITX_OK;
    float ms = 0;
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_tile_sum, nt, bo->d_tile_base, bo->d_tot);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(bo->ev[1], bo->st));
    ITX_TRY(hipMemcpyAsync(bo->h_tot, bo->d_tot, tot_bytes, hipMemcpyDeviceToHost, bo->st));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bo_read_gather_time(bo);                                               // (the batch or round before this one)
    ITX_TRY(hipEventElapsedTime(&ms, bo->ev[0], bo->ev[1]));
    *acc_ms += (double)ms;
out:
    return rc;
}

int bo_launch_gather_at(itx_bamout *bo, int wide, int ann, const uint8_t *u, const void *rec_off, uint32_t n, const uint32_t *len_in, const ull *tile_base, ull base,
                        uint8_t *pay, const int32_t *hit_row)
{
    int rc = ITX_OK;
    const dim3 grid((n + BO_TILE - 1) / BO_TILE), wg(BO_TILE);
    if (wide && ann)
        hipLaunchKernelGGL((k_bo_gather<ull, true>), grid, wg, 0, bo->st, u, (const ull *)rec_off, n, len_in, tile_base, base, pay, hit_row, bo->ann);
    else if (wide)
        hipLaunchKernelGGL((k_bo_gather<ull, false>), grid, wg, 0, bo->st, u, (const ull *)rec_off, n, len_in, tile_base, base, pay, hit_row, bo->ann);
    else if (ann)
        hipLaunchKernelGGL((k_bo_gather<uint32_t, true>), grid, wg, 0, bo->st, u, (const uint32_t *)rec_off, n, len_in, tile_base, base, pay, hit_row, bo->ann);
    else
        hipLaunchKernelGGL((k_bo_gather<uint32_t, false>), grid, wg, 0, bo->st, u, (const uint32_t *)rec_off, n, len_in, tile_base, base, pay, hit_row, bo->ann);
    ITX_TRY(hipGetLastError());
out:
    return rc;
}

int bo_launch_gather(itx_bamout *bo, const uint8_t *u, const void *rec_off, uint32_t n, const int32_t *hit_row)
{
    return bo_launch_gather_at(bo, bo->sort == 2, bo->sort != 2 && bo->annotate, u, rec_off, n, bo->d_len, bo->d_tile_base, (ull)bo->carry, bo->d_pay, hit_row);
}

int bo_reserve(itx_bamout *bo, ull total, ull n_mem)
{
    bo_slot *s = &bo->slot[(bo->head + bo->pending) & 1];
    size_t want_pay = 0, want_mem = 0, want_pk = 0;
    if (n_mem > 0x7fffff00ull) {
        itx_set_error("itx_bamout: %llu members in one batch", n_mem);
        return ITX_E_LIMIT;
    }
    if (n_mem && bo->pending == 2) {
        itx_set_error("itx_bamout: two batches wait to be collected (itx_bamout_collect)");
        return ITX_E_STATE;
    }
    if (total > bo->pay_cap) want_pay = (size_t)(total + (total > 2 * (ull)bo->pay_cap ? total / 4 : total));
    if (n_mem > bo->mem_cap) want_mem = (size_t)(n_mem + n_mem / 4 + 16);
    if (n_mem && n_mem * BO_STRIDE > s->cap) want_pk = (size_t)((n_mem + n_mem / 4 + 16) * BO_STRIDE);
    // taken together: the stream, of which the carry is kept; the members' slots, sizes and offsets; the slot's packed buffer and its
    // page-locked twin (the slot is not busy: nothing reads its buffers). Of the last five nothing is kept.
    ItxGrow g[6] = {{(void **)&bo->d_pay, bo->carry, want_pay ? want_pay + 16 : 0},
                    {(void **)&bo->d_mem, 0, want_mem * BO_STRIDE},
                    {(void **)&bo->d_msize, 0, 4 * want_mem},
                    {(void **)&bo->d_moff, 0, want_mem ? 8 * (want_mem + 1) : 0},
                    {(void **)&s->d_packed, 0, want_pk},
                    {(void **)&s->h_pin, 0, want_pk, 1}};
    if (itx_grow_alloc(g, 6) >= 0) {
        itx_set_error("itx_bamout: no memory for a stream of %llu bytes in %llu members%s", total, n_mem, bo->sort ? " (run without -s)" : "");
        return ITX_E_NOMEM;
    }
    const int rc = itx_grow_commit(bo->st, g, 6);
    if (rc != ITX_OK) return rc;
    if (want_pay) {
        bo->pay_cap = want_pay;
        bo->stats.grows++;
    }
    if (want_mem) bo->mem_cap = want_mem;
    if (want_pk) s->cap = want_pk;
    return ITX_OK;
}

// ---- the batch path
int itx_bamout_start(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, const int32_t *d_hit_row, size_t n, void *stream)
{
    if (!bo || (n && (!u || !rec_off || !d_hit_row))) {
        itx_set_error("itx_bamout: bad argument");
        return ITX_E_ARG;
    }
    if (n > bo->cap) {
        itx_set_error("itx_bamout: batch exceeds the capacity");
        return ITX_E_ARG;
    }
    if (bo->finished || bo->sort == 2) {
        itx_set_error("itx_bamout: the stream is %s", bo->finished ? "finished" : "being replayed in sorted order");
        return ITX_E_STATE;
    }
    if (!n) return ITX_OK;
    int rc = ITX_OK;
    ull total = 0;
    const uint32_t nt = (uint32_t)((n + BO_TILE - 1) / BO_TILE);
    ITX_TRY(hipSetDevice(bo->device));
    if ((hipStream_t)stream != bo->st) {                                   // the chosen rows were left on another stream
        ITX_TRY(hipEventRecord(bo->ev[4], (hipStream_t)stream));
        ITX_TRY(hipStreamWaitEvent(bo->st, bo->ev[4], 0));
    }
    ITX_TRY(hipEventRecord(bo->ev[0], bo->st));
    ITX_TRY(hipMemsetAsync(bo->d_tot, 0, BO_TOT_BYTES, bo->st));
    if (bo->annotate)
        hipLaunchKernelGGL((k_bo_measure<true>), dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, d_hit_row, (uint32_t)n, bo->d_len, bo->d_tile_sum, bo->d_tot, bo->ann);
    else
        hipLaunchKernelGGL((k_bo_measure<false>), dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, d_hit_row, (uint32_t)n, bo->d_len, bo->d_tile_sum, bo->d_tot, bo->ann);
    ITX_TRY(hipGetLastError());
    if ((rc = bo_totals(bo, nt, BO_TOT_BYTES, &bo->stats.gather_ms)) != ITX_OK) goto out;
    if (bo->h_tot[3]) {
        itx_set_error("itx_bamout: %llu records chose a row outside the %u rows given to itx_bamout_annotate_enable", bo->h_tot[3], bo->ann.n_rows);
        rc = ITX_E_ARG;
        goto out;
    }
    if (bo->h_tot[2]) {
        itx_set_error("itx_bamout: %llu records of a gibibyte or more%s", bo->h_tot[2], bo->annotate ? " with their tags" : "");
        rc = ITX_E_LIMIT;
        goto out;
    }
    total = (ull)bo->carry + bo->h_tot[0];
    // (sort mode: the stream is held whole, no member is made and nothing is indexed before the replay)
    if ((rc = bo_reserve(bo, total, bo->sort ? 0 : total / BO_P)) != ITX_OK) goto out;
    if (bo->sort && (rc = bs_reserve(bo, bo->h_tot[1])) != ITX_OK) goto out;
    if (bo->ix && !bo->sort && (rc = itx_bamidx_reserve(bo->ix, bo->st, bo->h_tot[1], total / BO_P)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(bo->ev[2], bo->st));
    if (bo->h_tot[0] && (rc = bo_launch_gather(bo, u, rec_off, (uint32_t)n, d_hit_row)) != ITX_OK) goto out;
    if (bo->sort && bo->h_tot[1] && (rc = bs_entries(bo, u, rec_off, (uint32_t)n, bo->h_tot[1], bo->mates ? d_hit_row : nullptr)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(bo->ev[3], bo->st));
    bo->gather_timed = 1;
    if (bo->ix && !bo->sort &&
        (rc = itx_bamidx_entries(bo->ix, bo->st, u, rec_off, (uint32_t)n, bo->d_len, bo->d_tile_base, bo->stream_base + bo->carry, bo->h_tot[1])) != ITX_OK)
        goto out;
    bo->stats.batches++;
    bo->stats.records += bo->h_tot[1];
    bo->stats.payload_bytes += bo->h_tot[0];
    bo->tag_bytes += bo->h_tot[4];
    if (bo->sort) bo->carry = (size_t)total;
    else rc = bo_emit(bo, total, 0);
    if (rc == ITX_OK && bo->mates == 1) rc = bm_batch(bo, u, rec_off, (uint32_t)n);
out:
    return rc;
}

extern "C" int itx_bamout_run(itx_bamout *bo, const void *d_bytes, const uint32_t *d_rec_off, const int32_t *d_hit_row, size_t n, void *stream)
{
    return itx_bamout_start(bo, (const uint8_t *)d_bytes, d_rec_off, d_hit_row, n, stream);
}

// the batch's records have been read (its members may still be in the making): the window's arrays are the decoder's again
extern "C" int itx_bamout_wait_kernels(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_wait_kernels: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(bo->device));
    if (bo->gather_timed) {
        const double t0 = itx_wall_now();
        ITX_TRY(hipEventSynchronize(bo->ev[3]));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
        bo_read_gather_time(bo);
    }
    if (bo->mates_timed) {                                                 // (-m: the candidate gather and its entry kernel read the window too)
        float ms = 0;
        const double t0 = itx_wall_now();
        ITX_TRY(hipEventSynchronize(bo->mev[1]));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
        if (hipEventElapsedTime(&ms, bo->mev[0], bo->mev[1]) == hipSuccess) bo->mstats.gather_ms += (double)ms;
        bo->mates_timed = 0;
    }
out:
    return rc;
}

extern "C" int itx_bamout_append_host(itx_bamout *bo, const void *bytes, size_t len)
{
    if (!bo || (len && !bytes)) {
        itx_set_error("itx_bamout_append_host: bad argument");
        return ITX_E_ARG;
    }
    if (bo->finished || bo->sort == 2) {
        itx_set_error("itx_bamout_append_host: the stream is %s", bo->finished ? "finished" : "being replayed in sorted order");
        return ITX_E_STATE;
    }
    size_t at = 0, n_rec = 0;
    uint32_t *h_off = nullptr;                                             // with an index: where every record starts
    BoSortEnt *h_ent = nullptr;                                            // sort mode: the records' entries, made here
    ull bad = 0;
    uint32_t maxtid = 0;
    if (bo->ix && !bo->sort && len >= 0xffffff00ull) {
        itx_set_error("itx_bamout_append_host: %zu bytes in one call while an index is built", len);
        return ITX_E_LIMIT;
    }
    while (at < len) {                                                     // whole records, or nothing is appended
        uint32_t bs = 0;
        if (len - at >= 4) memcpy(&bs, (const uint8_t *)bytes + at, 4);
        if (len - at < 4 || bs >= BO_MAX_RECORD || (size_t)bs > len - at - 4) {
            itx_set_error("itx_bamout_append_host: the bytes are not whole records (record %zu at byte %zu of %zu)", n_rec, at, len);
            return ITX_E_ARG;
        }
        at += 4 + (size_t)bs;
        n_rec++;
    }
    if (!len) return ITX_OK;
    if (bo->mates && bo->annotate && (!bo->host_rows || bo->n_host_rows != n_rec)) {
        itx_set_error("itx_bamout_append_host: %s", bo->host_rows ? "the rows of itx_bamout_mates_host_rows are not one per record" : "mates mode with tags needs the records' rows first (itx_bamout_mates_host_rows)");
        return bo->host_rows ? ITX_E_ARG : ITX_E_STATE;
    }
    int rc = ITX_OK;
    const ull total = (ull)bo->carry + len;
    if (bo->sort) {
        if (!(h_ent = (BoSortEnt *)malloc(sizeof(BoSortEnt) * n_rec))) {
            itx_set_error("itx_bamout_append_host: no memory for the sort entries of %zu records", n_rec);
            return ITX_E_NOMEM;
        }
        at = 0;
        for (size_t i = 0; i < n_rec; i++) {
            uint32_t bs;
            ItxBamSortKey k;
            memcpy(&bs, (const uint8_t *)bytes + at, 4);
            if (itx_bamsort_key((const uint8_t *)bytes + at, 4u + bs, &k)) bad++;
            else if ((uint32_t)k.tid > maxtid) maxtid = (uint32_t)k.tid;
            h_ent[i].tid = itx_bamsort_high(&k);
            h_ent[i].low = itx_bamsort_low(&k);
            h_ent[i].off = (ull)bo->carry + at;
            h_ent[i].len = 4u + bs;
            h_ent[i].pad = bo->mates ? (bo->host_rows && bo->n_host_rows == n_rec ? (uint32_t)bo->host_rows[i] : BO_NO_ROW) : 0u;
            at += 4 + (size_t)bs;
        }
    } else if (bo->ix) {
        if (!(h_off = (uint32_t *)malloc(4 * n_rec))) {
            itx_set_error("itx_bamout_append_host: no memory for the offsets of %zu records", n_rec);
            return ITX_E_NOMEM;
        }
        at = 0;
        for (size_t i = 0; i < n_rec; i++) {
            uint32_t bs;
            memcpy(&bs, (const uint8_t *)bytes + at, 4);
            h_off[i] = (uint32_t)at;
            at += 4 + (size_t)bs;
        }
    }
    ITX_TRY(hipSetDevice(bo->device));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));                              // device batches before this one have their place
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bo_read_gather_time(bo);
    if ((rc = bo_reserve(bo, total, bo->sort ? 0 : total / BO_P)) != ITX_OK) goto out;
    if (bo->sort && (rc = bs_reserve(bo, n_rec)) != ITX_OK) goto out;
    if (bo->ix && !bo->sort && (rc = itx_bamidx_reserve(bo->ix, bo->st, n_rec, total / BO_P)) != ITX_OK) goto out;
    ITX_TRY(hipMemcpyAsync(bo->d_pay + bo->carry, bytes, len, hipMemcpyHostToDevice, bo->st));
    if (bo->sort) ITX_TRY(hipMemcpyAsync(bo->d_sent + bo->n_sent, h_ent, sizeof(BoSortEnt) * n_rec, hipMemcpyHostToDevice, bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));                                  // the caller's bytes are its own again
    if (bo->ix && !bo->sort &&
        (rc = itx_bamidx_host_records(bo->ix, bo->st, bo->d_pay + bo->carry, h_off, (uint32_t)n_rec, bo->stream_base + bo->carry)) != ITX_OK)
        goto out;
    bo->stats.host_batches++;
    bo->stats.records += n_rec;
    bo->stats.payload_bytes += len;
    if (bo->sort) {                                                        // held whole: the entries stand in the pool in stream order
        bo->n_sent += n_rec;
        bo->host_bad += bad;
        if (maxtid > bo->host_maxtid) bo->host_maxtid = maxtid;
        bo->carry = (size_t)total;
    } else {
        rc = bo_emit(bo, total, 0);
    }
out:
    free(h_off);
    free(h_ent);
    free(bo->host_rows);                                                   // (the rows were this call's)
    bo->host_rows = nullptr;
    bo->n_host_rows = 0;
    return rc;
}

extern "C" int itx_bamout_finish(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_finish: bad argument");
        return ITX_E_ARG;
    }
    if (bo->finished) {
        itx_set_error("itx_bamout_finish: called twice");
        return ITX_E_STATE;
    }
    if (bo->sort) {
        itx_set_error("itx_bamout_finish: the stream is to be sorted (itx_bamout_sort_next)");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(bo->device));
    ITX_TRY(hipStreamSynchronize(bo->st));
    bo_read_gather_time(bo);
    if (bo->carry) {
        if ((rc = bo_reserve(bo, bo->carry, 1)) != ITX_OK) goto out;
        if (bo->ix && (rc = itx_bamidx_reserve(bo->ix, bo->st, 0, 1)) != ITX_OK) goto out;
        if ((rc = bo_emit(bo, bo->carry, 1)) != ITX_OK) goto out;
    }
    bo->finished = 1;
out:
    return rc;
}

extern "C" int itx_bamout_collect(itx_bamout *bo, itx_bamout_members *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_collect: bad argument");
        return ITX_E_ARG;
    }
    memset(out, 0, sizeof *out);
    if (!bo->pending) return ITX_OK;
    int rc = ITX_OK;
    float ms = 0;
    bo_slot *s = &bo->slot[bo->head];
    ITX_TRY(hipSetDevice(bo->device));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipEventSynchronize(s->e1));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    if (hipEventElapsedTime(&ms, s->e0, s->e1) == hipSuccess) bo->stats.member_ms += (double)ms;
    if (*s->h_total > s->cap) {
        itx_set_error("itx_bamout_collect: %llu packed bytes in a buffer of %zu", *s->h_total, s->cap);
        rc = ITX_E_LIMIT;
        goto out;
    }
    if (*s->h_total) {
        ITX_TRY(hipMemcpyAsync(s->h_pin, s->d_packed, (size_t)*s->h_total, hipMemcpyDeviceToHost, bo->cst));
        ITX_TRY(hipStreamSynchronize(bo->cst));
    }
    out->bytes = s->h_pin;
    out->len = *s->h_total;
    out->room = s->cap;
    out->n_members = s->n_mem;
    bo->stats.out_bytes += *s->h_total;
    s->busy = 0;
    bo->head ^= 1;
    bo->pending--;
out:
    return rc;
}

extern "C" int itx_bamout_pending(const itx_bamout *bo) { return bo ? bo->pending : 0; }

extern "C" int itx_bamout_get_stats(const itx_bamout *bo, itx_bamout_stats *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *out = bo->stats;
    out->carry = bo->carry;
    return ITX_OK;
}

// ---- the .bai index of the stream (csrc/itx_bamidx.hip)
extern "C" int itx_bamout_index_enable(itx_bamout *bo, int32_t n_ref, const int32_t *l_ref)
{
    if (!bo || n_ref < 0 || (n_ref && !l_ref)) {
        itx_set_error("itx_bamout_index_enable: bad argument");
        return ITX_E_ARG;
    }
    if (bo_not_begun(bo, "itx_bamout_index_enable", bo->ix != nullptr) != ITX_OK) return ITX_E_STATE;
    const int rc = itx_bamidx_create(bo->device, n_ref, l_ref, &bo->ix);
    if (rc == ITX_OK) bo->n_ref = n_ref;
    return rc;
}

extern "C" int itx_bamout_index_finish(itx_bamout *bo, uint64_t first_member_offset, itx_bamout_index_result *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_index_finish: bad argument");
        return ITX_E_ARG;
    }
    if (!bo->ix || !bo->finished) {
        itx_set_error("itx_bamout_index_finish: %s", bo->ix ? "the stream is not finished (itx_bamout_finish)" : "no index was asked for (itx_bamout_index_enable)");
        return ITX_E_STATE;
    }
    if (first_member_offset >> 47) {
        itx_set_error("itx_bamout_index_finish: a first member at byte %llu", (ull)first_member_offset);
        return ITX_E_LIMIT;
    }
    return itx_bamidx_finish(bo->ix, bo->st, first_member_offset, out);
}
