// itx_bamout_sort.hip — filter -b -s: the BAM writer's stream (itx_bamout.hip) held, sorted by coordinate and replayed.
// With itx_bamout_sort_enable the stream is held whole instead of being cut: every gather appends to it, and one lane per record
// appends {tid, pos << 1 | reverse, where the record lies, its length} to a pool (k_bs_entries, launched by itx_bamout_start; the
// rule is csrc/itx_bamsortrule.h). After the last batch itx_bamout_sort_next sorts (key, index) pairs with itx_radixsort.h, by the
// low key and then by tid, stable, and replays the records in sorted order a round of at most batch_capacity at a time through the
// batch path: k_bs_lengths lays the round's lengths and 64-bit offsets out in sorted order, k_tile_scan2 (bo_totals), then
// k_bo_gather reads the held stream (scattered, a record each) and writes the payload stream (coalesced), then members, scan and
// pack as for any batch (bo_emit).
// The pool grows by the two-phase rule of itx_devbuf.h; the sort's passes are itx_sort_run's. No kernel uses scratch.
#include "itx_bamout_priv.h"
#include "itx_bamsortrule.h"
#include "itx_devbuf.h"
#include "itx_radixsort.h"
#include "itx_textpack.h"

// behind a batch's gather: one entry per counted record (len != 0). Its place in the held stream comes from the gather's own tile
// bases and itx_tile_offsets, its place in the pool from the tile's record count the same way (k_bi_entries' arrangement).
// flag[0] counts the records that cannot be sorted, flag[1] is the highest tid seen; a workgroup adds to them once.
__global__ __launch_bounds__(BO_TILE) void k_bs_entries(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, uint32_t n, const uint32_t *__restrict__ len_in,
                                                         const ull *__restrict__ tile_base, ull stream_at, ull ent_at, BoSortEnt *__restrict__ ent, uint32_t *__restrict__ flag,
                                                         const int32_t *__restrict__ hit_row)
{
    __shared__ uint32_t s_w[BO_TILE / 64u], s_c[BO_TILE / 64u], s_f[2];
    if (threadIdx.x < 2) s_f[threadIdx.x] = 0;                             // (the barriers of itx_tile_offsets order this)
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0, count = 0;
    const uint32_t moff = itx_tile_offsets<BO_TILE>(len, s_w, &total);
    const uint32_t rank = itx_tile_offsets<BO_TILE>(len ? 1u : 0u, s_c, &count);
    if (len) {
        ItxBamSortKey k;
        // (under -a `len` is the annotated length while the bytes here are the source record's: the fields lie inside the shorter)
        const uint8_t *p = u + rec_off[i];
        const uint32_t src_len = 4u + itx_bamsort_u32(p);
        const int bad = itx_bamsort_key(p, src_len < len ? src_len : len, &k);
        BoSortEnt e;
        e.tid = itx_bamsort_high(&k);
        e.low = itx_bamsort_low(&k);
        e.off = stream_at + tile_base[2u * blockIdx.x] + moff;
        e.len = len;
        e.pad = hit_row ? (uint32_t)hit_row[i] : 0u;                      // (mates mode: the mate's tags are made from this row)
        ent[ent_at + tile_base[2u * blockIdx.x + 1u] + rank] = e;
        if (bad) atomicAdd(&s_f[0], 1u);
        else atomicMax(&s_f[1], e.tid);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_f[0]) atomicAdd(&flag[0], s_f[0]);
        if (s_f[1]) atomicMax(&flag[1], s_f[1]);
    }
}

// the pairs the radix sort moves: (low key, the entry's number); after the passes over the low key the key becomes the entry's tid
__global__ __launch_bounds__(256) void k_bs_keys(const BoSortEnt *__restrict__ ent, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = make_uint2(ent[i].low, i);
}

__global__ __launch_bounds__(256) void k_bs_rekey(const BoSortEnt *__restrict__ ent, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i].x = ent[keys[i].y].tid;
}

// one round of the replay, records sorted[0 .. n): their lengths and where they lie in the held stream, laid out in sorted order
// for the gather; a tile's bytes (64 bit) and records as k_bo_measure leaves them
__global__ __launch_bounds__(BO_TILE) void k_bs_lengths(const uint2 *__restrict__ sorted, const BoSortEnt *__restrict__ ent, uint32_t n, uint32_t *__restrict__ len_out,
                                                         ull *__restrict__ off_out, ull *__restrict__ tile_sum)
{
    __shared__ ull s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    if (i < n) {
        const BoSortEnt e = ent[sorted[i].y];
        len_out[i] = e.len;
        off_out[i] = e.off;
        atomicAdd(&s_sum[0], (ull)e.len);
        atomicAdd(&s_sum[1], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

extern "C" int itx_bamout_sort_enable(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_sort_enable: bad argument");
        return ITX_E_ARG;
    }
    if (bo_not_begun(bo, "itx_bamout_sort_enable", bo->sort) != ITX_OK) return ITX_E_STATE;
    int rc = ITX_OK;
    uint32_t *flag = nullptr, *h_flag = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ITX_TRY(hipSetDevice(bo->device));
    if (hipMalloc((void **)&flag, 16) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_sort_enable: no device memory (run without -s)");
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipHostMalloc((void **)&h_flag, 16, hipHostMallocDefault));
    ITX_TRY(hipMemset(flag, 0, 16));
    ITX_TRY(hipEventCreate(&ev[0]));
    ITX_TRY(hipEventCreate(&ev[1]));
    bo->d_sflag = flag;
    bo->h_sflag = h_flag;
    bo->sev[0] = ev[0];
    bo->sev[1] = ev[1];
    bo->sort = 1;
    return ITX_OK;
out:
    (void)hipFree(flag);
    if (h_flag) (void)hipHostFree(h_flag);
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

int bs_reserve(itx_bamout *bo, ull n_more)
{
    const ull want = bo->n_sent + n_more;
    if (want >= 0xfffffffeull) {
        itx_set_error("itx_bamout: %llu records to sort (run without -s)", want);
        return ITX_E_LIMIT;
    }
    if (want <= bo->sent_cap) return ITX_OK;
    const ull cap = want + want / 2 + 1024;
    const bool first = !bo->d_sent;
    ItxGrow g = {(void **)&bo->d_sent, sizeof(BoSortEnt) * bo->n_sent, sizeof(BoSortEnt) * cap};       // the pool alone; its entries are kept
    if (itx_grow_alloc(&g, 1) >= 0) {
        itx_set_error("itx_bamout: no device memory for the sort entries of %llu records (run without -s)", want);
        return ITX_E_NOMEM;
    }
    const int rc = itx_grow_commit(bo->st, &g, 1);
    if (rc != ITX_OK) return rc;
    bo->sent_cap = cap;
    if (!first) bo->sent_grows++;
    return ITX_OK;
}

int bs_entries(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, uint32_t n, ull n_counted, const int32_t *hit_row)
{
    int rc = ITX_OK;
    hipLaunchKernelGGL(k_bs_entries, dim3((n + BO_TILE - 1) / BO_TILE), dim3(BO_TILE), 0, bo->st, u, rec_off, n, bo->d_len, bo->d_tile_base, (ull)bo->carry, bo->n_sent,
                       bo->d_sent, bo->d_sflag, hit_row);
    ITX_TRY(hipGetLastError());
    bo->n_sent += n_counted;
out:
    return rc;
}

// the sort's device time is read once its events are through (the round's wait for its totals is behind them)
static void bs_read_sort_time(itx_bamout *bo)
{
    if (!bo->sort_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, bo->sev[0], bo->sev[1]) == hipSuccess) bo->sort_ms += (double)ms;
    bo->sort_timed = 0;
}

// The first sort_next: the flags are read, the replay's buffers allocated, and the sort of the pool enqueued. bo->st is idle.
// Nothing of the object changes before every check has passed and every buffer is there.
static int bs_begin(itx_bamout *bo)
{
    int rc = ITX_OK;
    const uint32_t N = (uint32_t)bo->n_sent;
    uint2 *k0 = nullptr, *k1 = nullptr, *sorted = nullptr;
    uint32_t *hist = nullptr, n_ref = 0, high = 0;
    ull *soff = nullptr, bad = 0;
    uint8_t *npay = nullptr;
    const size_t pay_cap = 4 * (size_t)BO_P;
    ITX_TRY(hipMemcpyAsync(bo->h_sflag, bo->d_sflag, 8, hipMemcpyDeviceToHost, bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));
    bad = bo->host_bad + bo->h_sflag[0];
    if (bad) {
        itx_set_error("itx_bamout_sort_next: %llu counted records name no reference or no position (tid or pos below 0): they cannot be sorted by coordinate", bad);
        rc = ITX_E_LIMIT;
        goto out;
    }
    if (N) {
        if (hipMalloc((void **)&k0, 8 * (size_t)N) != hipSuccess || hipMalloc((void **)&k1, 8 * (size_t)N) != hipSuccess ||
            hipMalloc((void **)&hist, itx_sort_hist_bytes(N)) != hipSuccess || hipMalloc((void **)&soff, 8 * (bo->cap + 64)) != hipSuccess ||
            hipMalloc((void **)&npay, pay_cap + 16) != hipSuccess) {
            (void)hipGetLastError();
            itx_set_error("itx_bamout_sort_next: no device memory to sort %u records beside a held stream of %zu bytes (run without -s)", N, bo->carry);
            rc = ITX_E_NOMEM;
            goto out;
        }
        n_ref = bo->n_ref > 0 ? (uint32_t)bo->n_ref : 0u;
        {
            const uint32_t seen = (bo->h_sflag[1] > bo->host_maxtid ? bo->h_sflag[1] : bo->host_maxtid) + 1u;
            if (seen > n_ref) n_ref = seen;                                // (a tid beyond the header's list still finds its place)
        }
        high = itx_bamsort_high_passes(n_ref);
        ITX_TRY(hipEventRecord(bo->sev[0], bo->st));
        hipLaunchKernelGGL(k_bs_keys, dim3((N + 255u) / 256u), dim3(256), 0, bo->st, bo->d_sent, N, k0);
        ITX_TRY(hipGetLastError());
        // four passes by the low key; then the keys become the tids, and the shift starts again at 0
        if ((rc = itx_sort_run(bo->st, k0, k1, N, 0u, 4u, hist, &sorted)) != ITX_OK) goto out;
        if (high) {
            hipLaunchKernelGGL(k_bs_rekey, dim3((N + 255u) / 256u), dim3(256), 0, bo->st, bo->d_sent, N, sorted);
            ITX_TRY(hipGetLastError());
            if ((rc = itx_sort_run(bo->st, sorted, sorted == k0 ? k1 : k0, N, 0u, high, hist, &sorted)) != ITX_OK) goto out;
        }
        ITX_TRY(hipEventRecord(bo->sev[1], bo->st));
        bo->sort_timed = 1;
    }
    // the held stream is what d_pay was; the payload stream starts anew
    bo->d_held = bo->d_pay;
    bo->d_pay = npay;
    bo->pay_cap = npay ? pay_cap : 0;
    bo->carry = 0;
    bo->d_k0 = k0;
    bo->d_k1 = k1;
    bo->sorted = sorted;
    bo->d_hist = hist;
    bo->d_soff = soff;
    bo->sort = 2;
    return ITX_OK;
out:
    if (k0 || k1) (void)hipStreamSynchronize(bo->st);                      // (kernels that were enqueued before something failed)
    (void)hipFree(k0);
    (void)hipFree(k1);
    (void)hipFree(hist);
    (void)hipFree(soff);
    (void)hipFree(npay);
    return rc;
}

// the sort's work arrays and the held stream go (the kernels that read them are through)
static void bs_release(itx_bamout *bo)
{
    (void)hipFree(bo->d_held);
    (void)hipFree(bo->d_k0);
    (void)hipFree(bo->d_k1);
    (void)hipFree(bo->d_hist);
    (void)hipFree(bo->d_soff);
    (void)hipFree(bo->d_sent);
    bo->d_held = nullptr;
    bo->d_k0 = bo->d_k1 = bo->sorted = nullptr;
    bo->d_hist = nullptr;
    bo->d_soff = nullptr;
    bo->d_sent = nullptr;
    bo->sent_cap = 0;
}

extern "C" int itx_bamout_sort_next(itx_bamout *bo, int *more)
{
    if (!bo || !more) {
        itx_set_error("itx_bamout_sort_next: bad argument");
        return ITX_E_ARG;
    }
    *more = 0;
    if (!bo->sort || bo->finished) {
        itx_set_error("itx_bamout_sort_next: %s", bo->sort ? "the stream is finished" : "no sort was asked for (itx_bamout_sort_enable)");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    ull total = 0, n_mem = 0;
    ull N = 0;
    uint32_t n = 0, nt = 0;
    int last = 0;
    ITX_TRY(hipSetDevice(bo->device));
    ITX_TRY(hipStreamSynchronize(bo->st));
    bo_read_gather_time(bo);
    // (-m: the mates join the held stream and the pool before the sort sees either)
    if (bo->sort == 1 && bo->mates == 1 && (rc = bm_join(bo)) != ITX_OK) goto out;
    if (bo->sort == 1 && (rc = bs_begin(bo)) != ITX_OK) goto out;
    N = bo->n_sent;
    if (!N) {                                                              // nothing was counted: no member
        bs_release(bo);
        bo->finished = 1;
        goto out;
    }
    n = (uint32_t)(N - bo->sort_done < bo->cap ? N - bo->sort_done : bo->cap);
    nt = (n + BO_TILE - 1) / BO_TILE;
    last = bo->sort_done + n == N;
    ITX_TRY(hipEventRecord(bo->ev[0], bo->st));
    ITX_TRY(hipMemsetAsync(bo->d_tot, 0, 32, bo->st));
    hipLaunchKernelGGL(k_bs_lengths, dim3(nt), dim3(BO_TILE), 0, bo->st, bo->sorted + bo->sort_done, bo->d_sent, n, bo->d_len, bo->d_soff, bo->d_tile_sum);
    ITX_TRY(hipGetLastError());
    if ((rc = bo_totals(bo, nt, 32, &bo->replay_ms)) != ITX_OK) goto out;  // (its wait: the members of the round before are through as well)
    bs_read_sort_time(bo);
    total = (ull)bo->carry + bo->h_tot[0];
    n_mem = total / BO_P + (last && total % BO_P ? 1 : 0);
    if ((rc = bo_reserve(bo, total, n_mem)) != ITX_OK) goto out;
    if (bo->ix && (rc = itx_bamidx_reserve(bo->ix, bo->st, n, n_mem)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(bo->ev[2], bo->st));
    // (under -a the held records are annotated already: the replay copies them byte for byte)
    if ((rc = bo_launch_gather(bo, bo->d_held, bo->d_soff, n, nullptr)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(bo->ev[3], bo->st));
    bo->gather_timed = 1;
    if (bo->ix && (rc = itx_bamidx_entries64(bo->ix, bo->st, bo->d_held, bo->d_soff, n, bo->d_len, bo->d_tile_base, bo->stream_base + bo->carry, n)) != ITX_OK) goto out;
    bo->sort_done += n;
    bo->rounds++;
    if ((rc = bo_emit(bo, total, last)) != ITX_OK) goto out;
    if (last) {
        // the held stream goes as soon as the last gather (and the index's entry kernel behind it) has read it
        if (bo->ix) itx_bamidx_batch_time(bo->ix);
        ITX_TRY(hipEventSynchronize(bo->ev[3]));
        bo_read_gather_time(bo);
        bs_release(bo);
        bo->finished = 1;
    }
    *more = !last;
out:
    return rc;
}

extern "C" int itx_bamout_sort_get_stats(const itx_bamout *bo, itx_bamout_sort_stats *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_sort_get_stats: bad argument");
        return ITX_E_ARG;
    }
    out->records = bo->n_sent;
    out->rounds = bo->rounds;
    out->pool_grows = bo->sent_grows;
    out->sort_ms = bo->sort_ms;
    out->replay_ms = bo->replay_ms;
    return ITX_OK;
}
