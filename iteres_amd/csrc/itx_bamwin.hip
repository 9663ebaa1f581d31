// itx_bamwin.hip — the decoded stream stays on the device: a WINDOW of inflated bytes per chunk (filled by the push pipeline,
// itx_inflate.hip), the BAM records in it located and
// parsed there (cussamtools/bam.c:179-210 bam_read1 + the fields generic.c:745-905 takes from bam1_core_t, bam.h:169-177),
// and only the 26-byte-per-record SoA crosses PCIe on the way back.
//
// Locating the records is a chain (a record's length says where the next one starts). The window is cut into pieces; a
// thread per piece GUESSES the first record start in its piece (three well-formed records in a row) and walks on from
// there; the host then checks the pieces in stream order — a piece counts only if its guess is exactly where the chain
// of the pieces before it arrives, otherwise it is walked again from there (k_rewalk) — which makes the result exact
// whatever the guesses were (same scheme as the host reader's locate_records, iteres_amd/host/bamio.c).
#include "itx_auxwalk.h"
#include "itx_bamout_priv.h"         /* itx_bamout_start */
#include "itx_device.h"
#include "itx_inflater.h"

#define PIECE (16u << 10)            /* bytes per located piece */
#define PIECE_SLOTS (PIECE / 36u + 2u)

struct PieceSum {
    uint32_t c, end, n, why;         /* guessed start (0xffffffff none), where the walk stopped, starts found; why as the host reader */
};

static __device__ inline uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static __device__ inline uint32_t walk(const uint8_t *u, uint32_t p, uint32_t lim, uint32_t L, uint32_t *off, uint32_t *pn, uint32_t *why)
{
    uint32_t n = 0;
    while (p < lim) {
        if (p + 4u > L) {
            *why = 1;
            *pn = n;
            return p;
        }
        const int32_t bl = (int32_t)ld32(u + p);
        if (bl < 32) {                                            /* bam.c:186-190: a malformed length ends the file */
            *why = 2;
            *pn = n;
            return p;
        }
        if ((uint64_t)p + 4u + (uint32_t)bl > L) {
            *why = 1;
            *pn = n;
            return p;
        }
        off[n++] = p;
        p += 4u + (uint32_t)bl;
    }
    *why = 0;
    *pn = n;
    return p;
}

static __device__ inline uint32_t looks_like_record(const uint8_t *u, uint32_t p, uint32_t L, int32_t n_targets)
{
    if ((uint64_t)p + 36u > L) return 0;
    const int32_t bl = (int32_t)ld32(u + p);
    if (bl < 32 || (uint64_t)p + 4u + (uint32_t)bl > L) return 0;
    const uint8_t *core = u + p + 4;
    const int32_t tid = (int32_t)ld32(core), pos = (int32_t)ld32(core + 4), l_qseq = (int32_t)ld32(core + 16), mtid = (int32_t)ld32(core + 20),
                  mpos = (int32_t)ld32(core + 24);
    const uint32_t x1 = ld32(core + 8), x2 = ld32(core + 12);
    const uint32_t l_qname = x1 & 0xffu, n_cigar = x2 & 0xffffu;
    if (tid < -1 || tid >= n_targets || mtid < -1 || mtid >= n_targets || pos < -1 || mpos < -1 || l_qseq < 0 || l_qname == 0) return 0;
    const uint64_t need = (uint64_t)l_qname + 4ull * n_cigar + ((uint64_t)l_qseq + 1) / 2 + (uint64_t)l_qseq;
    if (need > (uint64_t)bl - 32u) return 0;
    if (u[p + 36u + l_qname - 1u] != 0) return 0;
    return 4u + (uint32_t)bl;
}

__global__ __launch_bounds__(64) void k_guess(const uint8_t *__restrict__ u, uint32_t p0, uint32_t L, uint32_t T, int32_t n_targets, PieceSum *__restrict__ sum,
                                              uint32_t *__restrict__ spec)
{
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= T) return;
    const uint32_t b = p0 + t * PIECE, lim = L - b > PIECE ? b + PIECE : L;       // T = ceil((L - p0) / PIECE): b < L
    uint32_t c = 0xffffffffu;
    if (t == 0) {
        c = b;
    } else {
        for (uint32_t x = b; x < lim; x++) {
            uint32_t a = x, k = 0;
            while (k < 3 && a < L) {
                const uint32_t step = looks_like_record(u, a, L, n_targets);
                if (!step) break;
                a += step;
                k++;
            }
            if (k == 3 || (k > 0 && a >= L)) {
                c = x;
                break;
            }
        }
    }
    PieceSum s{c, c, 0, 0};
    if (c != 0xffffffffu) s.end = walk(u, c, lim, L, spec + (size_t)t * PIECE_SLOTS, &s.n, &s.why);
    sum[t] = s;
}

// one piece walked again from where the chain really arrives (one thread: it happens when a guess was misled)
__global__ void k_rewalk(const uint8_t *__restrict__ u, uint32_t from, uint32_t lim, uint32_t L, uint32_t t, PieceSum *__restrict__ sum, uint32_t *__restrict__ spec)
{
    if (threadIdx.x || blockIdx.x) return;
    PieceSum s{from, from, 0, 0};
    s.end = walk(u, from, lim, L, spec + (size_t)t * PIECE_SLOTS, &s.n, &s.why);
    sum[t] = s;
}

// accepted pieces' starts, in stream order, into one array: base[t] = records before piece t, cnt[t] = its records
__global__ __launch_bounds__(64) void k_compact(const uint32_t *__restrict__ spec, const uint32_t *__restrict__ base, const uint32_t *__restrict__ cnt, uint32_t T,
                                                uint32_t *__restrict__ rec_off)
{
    const uint32_t t = blockIdx.x;
    if (t >= T) return;
    const uint32_t n = cnt[t], b = base[t];
    for (uint32_t j = threadIdx.x; j < n; j += 64u) rec_off[b + j] = spec[(size_t)t * PIECE_SLOTS + j];
}

// one thread per record: the fields generic.c:745-905 reads, bam_calend (bam.c:17-27: M, D, N advance) or pos + l_qseq
__global__ __launch_bounds__(256) void k_parse(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, uint32_t n, int32_t *__restrict__ tid_o,
                                               int32_t *__restrict__ pos_o, int32_t *__restrict__ end_o, uint8_t *__restrict__ mapq_o, uint8_t *__restrict__ f5_o,
                                               int32_t *__restrict__ mpos_o, int32_t *__restrict__ isize_o, uint8_t *__restrict__ xa_o, uint32_t *__restrict__ flags,
                                               uint8_t *__restrict__ seen, int32_t n_targets)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool paired = false, xa = false;
    if (i < n) {
        const uint8_t *p = u + rec_off[i];
        const uint32_t block_len = ld32(p);
        const uint8_t *core = p + 4, *data = p + 36;
        const uint32_t dlen = block_len - 32u;
        const int32_t tid = (int32_t)ld32(core), pos = (int32_t)ld32(core + 4);
        const uint32_t x1 = ld32(core + 8), x2 = ld32(core + 12);
        const uint32_t l_qname = x1 & 0xffu, qual = (x1 >> 8) & 0xffu, flag = x2 >> 16, n_cigar = x2 & 0xffffu;
        const int32_t l_qseq = (int32_t)ld32(core + 16), mpos = (int32_t)ld32(core + 24), isize = (int32_t)ld32(core + 28);
        int32_t tmpend;
        if (n_cigar && (uint64_t)l_qname + 4ull * n_cigar <= dlen) {
            uint32_t e = (uint32_t)pos;
            const uint8_t *cg = data + l_qname;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = ld32(cg + 4 * k), op = c & 0xfu;
                if (op == 0 || op == 2 || op == 3) e += c >> 4;
            }
            tmpend = (int32_t)e;
        } else {
            tmpend = (int32_t)((uint32_t)pos + (uint32_t)l_qseq);             /* generic.c:820 */
        }
        tid_o[i] = tid;
        pos_o[i] = pos;
        end_o[i] = tmpend;
        mapq_o[i] = (uint8_t)qual;
        f5_o[i] = ITX_FLAG5(flag);
        mpos_o[i] = mpos;
        isize_o[i] = isize;
        paired = flag & 1u;
        if (!(flag & 4u) && tid >= 0 && tid < n_targets) seen[tid] = 1;          /* a mapped record on this reference (generic.c:764,781) */
        const uint8_t *as, *ae, *xt;                                             /* is there an XA tag? (itx_auxwalk.h) */
        if (itx_aux_bounds(p, &as, &ae)) {
            itx_aux_find(as, ae, ITX_AUX_TAG('X', 'A'), &xt, 0, nullptr);
            xa = xt != nullptr;
        }
        xa_o[i] = xa ? 1 : 0;
    }
    const unsigned long long bp = __ballot(paired), bx = __ballot(xa);
    if ((threadIdx.x & 63u) == 0 && (bp | bx)) atomicOr(flags, (bp ? 1u : 0u) | (bx ? 2u : 0u));
}

// bytes [src, src + n) of a buffer moved UP by `shift` bytes (0 < shift; the ranges overlap): ONE workgroup walks the range from
// its end in chunks; a chunk is loaded whole, then — behind a barrier — stored: its destination lies above every source byte that is
// still to be read. For shifts too small to move the bytes in a few device-to-device copies (itx_bamwin_carry).
#define MOVE_THREADS 1024u
#define MOVE_PER_THREAD 64u                  /* bytes per thread and chunk */
__global__ __launch_bounds__(MOVE_THREADS) void k_move_up(uint8_t *__restrict__ buf, size_t src, size_t n, size_t shift)
{
    const size_t chunk = (size_t)MOVE_THREADS * MOVE_PER_THREAD;
    for (size_t left = n; left > 0;) {
        const size_t m = left < chunk ? left : chunk, c0 = src + left - m;
        uint8_t v[MOVE_PER_THREAD];
        const size_t a = (size_t)threadIdx.x * MOVE_PER_THREAD;
        uint32_t k_n = 0;
        if (a < m) k_n = (uint32_t)(m - a < MOVE_PER_THREAD ? m - a : MOVE_PER_THREAD);
#pragma unroll
        for (uint32_t k = 0; k < MOVE_PER_THREAD; k++) v[k] = k < k_n ? buf[c0 + a + k] : (uint8_t)0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < MOVE_PER_THREAD; k++)
            if (k < k_n) buf[c0 + a + k + shift] = v[k];
        __syncthreads();
        left -= m;
    }
}

/* the parse buffers (itx_inflater_destroy) */
void bamwin_free(itx_inflater *h)
{
    auto &P = h->parse;
    (void)hipFree(P.d_sum);
    (void)hipFree(P.d_spec);
    (void)hipFree(P.d_pb);
    (void)hipFree(P.d_recoff);
    (void)hipFree(P.d_flags);
    (void)hipFree(P.d_seen);
    (void)hipFree(P.d_tid);
    (void)hipFree(P.d_pos);
    (void)hipFree(P.d_end);
    (void)hipFree(P.d_mpos);
    (void)hipFree(P.d_isize);
    (void)hipFree(P.d_mapq);
    (void)hipFree(P.d_f5);
    (void)hipFree(P.d_xa);
    if (P.h_sum) (void)hipHostFree(P.h_sum);
    if (P.h_pb) (void)hipHostFree(P.h_pb);
}

extern "C" int itx_bamwin_patch(itx_inflater *h, int w, size_t uoff, const void *bytes, size_t len)
{
    if (!h || BAD_W(w) || !bytes || WIN_HEAD + uoff + len > h->wins.win[w].len) return ITX_E_ARG;
    ITX_HIP(hipSetDevice(h->device));
    ITX_HIP(hipMemcpy(h->wins.win[w].buf + WIN_HEAD + uoff, bytes, len, hipMemcpyHostToDevice));
    return ITX_OK;
}

extern "C" int itx_bamwin_truncate(itx_inflater *h, int w, size_t n_new)
{
    if (!h || BAD_W(w) || WIN_HEAD + n_new > h->wins.win[w].len) return ITX_E_ARG;
    h->wins.win[w].len = WIN_HEAD + (uint32_t)n_new;
    return ITX_OK;
}

extern "C" int itx_bamwin_carry(itx_inflater *h, int from, int to)
{
    if (!h || BAD_W(from) || BAD_W(to) || from == to) return ITX_E_ARG;
    const uint32_t tail = h->wins.win[from].len - h->wins.win[from].consumed;
    if (h->wins.win[to].start != WIN_HEAD) return ITX_E_STATE;
    ITX_HIP(hipSetDevice(h->device));
    if (tail > WIN_HEAD) {
        // A record of more than 4 MiB straddles the chunks (a very long read): the head room in front of the fresh bytes is too
        // small, so the fresh bytes move back instead — as long as the window's buffer holds both (the reference reads such
        // files, bam.c:179-210 just reallocs; so does the host decoder).
        const size_t fresh = h->wins.win[to].len - WIN_HEAD;
        if ((size_t)tail + fresh + 64 > h->wins.win[to].cap || (size_t)tail + fresh > 0xfffffff0u) {
            itx_set_error("a BAM record of more than %u bytes straddles two chunks and does not fit the window (%zu bytes): beyond the device decoder "
                          "(ITX_HOST_INFLATE=1 reads such files)",
                          tail, h->wins.win[to].cap);
            return ITX_E_LIMIT;
        }
        // move [WIN_HEAD, WIN_HEAD + fresh) to [tail, tail + fresh): from the end, in pieces no longer than the shift (no piece
        // overlaps its source) — when the shift is a megabyte or more; a tail only just over the head room would mean millions of
        // tiny copies (a shift of 100 bytes over a 1 GiB window: 10 M calls), so small shifts are one kernel that walks backwards
        const size_t shift = (size_t)tail - WIN_HEAD;
        if (shift >= (1u << 20)) {
            for (size_t done = 0; done < fresh;) {
                const size_t n = fresh - done < shift ? fresh - done : shift;
                const size_t src = WIN_HEAD + fresh - done - n;
                ITX_HIP(hipMemcpyAsync(h->wins.win[to].buf + src + shift, h->wins.win[to].buf + src, n, hipMemcpyDeviceToDevice, h->st[1]));
                done += n;
            }
        } else if (fresh) {
            hipLaunchKernelGGL(k_move_up, dim3(1), dim3(MOVE_THREADS), 0, h->st[1], h->wins.win[to].buf, (size_t)WIN_HEAD, fresh, shift);
            ITX_HIP(hipGetLastError());
        }
        ITX_HIP(hipMemcpyAsync(h->wins.win[to].buf, h->wins.win[from].buf + h->wins.win[from].consumed, tail, hipMemcpyDeviceToDevice, h->st[1]));
        ITX_HIP(hipStreamSynchronize(h->st[1]));
        h->wins.win[to].start = h->wins.win[to].consumed = 0;
        h->wins.win[to].len = tail + (uint32_t)fresh;
        h->wins.win[from].consumed = h->wins.win[from].len;
        return ITX_OK;
    }
    if (tail) {
        ITX_HIP(hipMemcpyAsync(h->wins.win[to].buf + WIN_HEAD - tail, h->wins.win[from].buf + h->wins.win[from].consumed, tail, hipMemcpyDeviceToDevice, h->st[1]));
        ITX_HIP(hipStreamSynchronize(h->st[1]));
    }
    h->wins.win[to].start = h->wins.win[to].consumed = WIN_HEAD - tail;
    h->wins.win[from].consumed = h->wins.win[from].len;
    return ITX_OK;
}

extern "C" int itx_bamwin_avail(const itx_inflater *h, int w, size_t *bytes)
{
    if (!h || BAD_W(w) || !bytes) return ITX_E_ARG;
    *bytes = h->wins.win[w].len - h->wins.win[w].consumed;
    return ITX_OK;
}

/* bytes [off, off + len) of the window's unconsumed part, to the host */
extern "C" int itx_bamwin_peek(itx_inflater *h, int w, size_t off, void *dst, size_t len)
{
    if (!h || BAD_W(w) || !dst || (size_t)h->wins.win[w].consumed + off + len > h->wins.win[w].len) return ITX_E_ARG;
    ITX_HIP(hipSetDevice(h->device));
    if (len) ITX_HIP(hipMemcpy(dst, h->wins.win[w].buf + h->wins.win[w].consumed + off, len, hipMemcpyDeviceToHost));
    return ITX_OK;
}

extern "C" int itx_bamwin_skip(itx_inflater *h, int w, size_t n)
{
    if (!h || BAD_W(w) || (size_t)h->wins.win[w].consumed + n > h->wins.win[w].len) return ITX_E_ARG;
    h->wins.win[w].consumed += (uint32_t)n;
    h->wins.win[w].start = h->wins.win[w].consumed;
    return ITX_OK;
}

extern "C" int itx_bamwin_parse(itx_inflater *h, int w, int n_targets, size_t *n_rec, int *malformed, int *flags, size_t *rewalked)
{
    if (!h || BAD_W(w) || !n_rec || !malformed || !flags) return ITX_E_ARG;
    *n_rec = 0;
    *malformed = 0;
    *flags = 0;
    h->parse.n_rec = 0;
    h->parse.parsed_w = w;
    const uint32_t p0 = h->wins.win[w].consumed, L = h->wins.win[w].len;
    if (p0 >= L) return ITX_OK;
    ITX_HIP(hipSetDevice(h->device));
    hipStream_t st = h->st[1];
    const uint32_t T = (L - p0 + PIECE - 1) / PIECE;
    int rc;
    {
        size_t cap = h->parse.sum_cap;
        if ((rc = grow((PieceSum **)&h->parse.d_sum, &cap, (size_t)T)) != ITX_OK) return rc;
        if (cap != h->parse.sum_cap) {
            if (h->parse.h_sum) (void)hipHostFree(h->parse.h_sum);
            h->parse.h_sum = nullptr;
            ITX_HIP(hipHostMalloc(&h->parse.h_sum, cap * sizeof(PieceSum), hipHostMallocDefault));
            h->parse.sum_cap = cap;
        }
        cap = h->parse.pb_cap;
        if ((rc = grow(&h->parse.d_pb, &cap, 2 * (size_t)T)) != ITX_OK) return rc;
        if (cap != h->parse.pb_cap) {
            if (h->parse.h_pb) (void)hipHostFree(h->parse.h_pb);
            h->parse.h_pb = nullptr;
            ITX_HIP(hipHostMalloc((void **)&h->parse.h_pb, cap * sizeof(uint32_t), hipHostMallocDefault));
            h->parse.pb_cap = cap;
        }
    }
    if ((rc = grow(&h->parse.d_spec, &h->parse.spec_cap, (size_t)T * PIECE_SLOTS)) != ITX_OK) return rc;
    if (!h->parse.d_flags) ITX_HIP(hipMalloc((void **)&h->parse.d_flags, 16));
    if ((rc = grow(&h->parse.d_seen, &h->parse.seen_cap, (size_t)(n_targets > 0 ? n_targets : 1))) != ITX_OK) return rc;
    ITX_HIP(hipMemsetAsync(h->parse.d_seen, 0, (size_t)(n_targets > 0 ? n_targets : 1), st));
    PieceSum *d_sum = (PieceSum *)h->parse.d_sum, *sum = (PieceSum *)h->parse.h_sum;
    const uint8_t *u = h->wins.win[w].buf;
    hipLaunchKernelGGL(k_guess, dim3((T + 63) / 64), dim3(64), 0, st, u, p0, L, T, (int32_t)n_targets, d_sum, h->parse.d_spec);
    ITX_HIP(hipGetLastError());
    ITX_HIP(hipMemcpyAsync(sum, d_sum, (size_t)T * sizeof(PieceSum), hipMemcpyDeviceToHost, st));
    ITX_HIP(hipStreamSynchronize(st));
    // in stream order: a piece counts if its guess is where the chain arrives, else it is walked again from there
    uint32_t cur = p0, endp = p0, why = 0, tot = 0;
    uint32_t *base = h->parse.h_pb, *cnt = h->parse.h_pb + T;
    size_t redo = 0;
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t b = p0 + t * PIECE, lim = L - b > PIECE ? b + PIECE : L;
        base[t] = tot;
        cnt[t] = 0;
        if (why || cur >= lim) continue;                        // the stream ended, or a record reaches over the whole piece
        if (sum[t].c != cur) {
            hipLaunchKernelGGL(k_rewalk, dim3(1), dim3(1), 0, st, u, cur, lim, L, t, d_sum, h->parse.d_spec);
            ITX_HIP(hipGetLastError());
            ITX_HIP(hipMemcpyAsync(&sum[t], d_sum + t, sizeof(PieceSum), hipMemcpyDeviceToHost, st));
            ITX_HIP(hipStreamSynchronize(st));
            redo++;
        }
        cnt[t] = sum[t].n;
        tot += sum[t].n;
        endp = cur = sum[t].end;
        why = sum[t].why;
    }
    if (rewalked) *rewalked = redo;
    if (why == 2) {                                               // bam.c:186-190: a malformed length ends the file
        *malformed = 1;
        h->wins.win[w].len = endp;
    }
    h->wins.win[w].consumed = tot ? endp : p0;
    if (why == 2 && tot == 0) h->wins.win[w].consumed = endp;
    if (tot == 0) return ITX_OK;
    if ((rc = grow(&h->parse.d_recoff, &h->parse.recoff_cap, (size_t)tot)) != ITX_OK) return rc;
    if (h->parse.soa_cap < tot) {
        const size_t want = (size_t)tot + tot / 4;
        int32_t **i32s[5] = {&h->parse.d_tid, &h->parse.d_pos, &h->parse.d_end, &h->parse.d_mpos, &h->parse.d_isize};
        uint8_t **u8s[3] = {&h->parse.d_mapq, &h->parse.d_f5, &h->parse.d_xa};
        for (auto pp : i32s) {
            if (*pp) ITX_HIP(hipFree(*pp));
            *pp = nullptr;
            ITX_HIP(hipMalloc((void **)pp, want * 4));
        }
        for (auto pp : u8s) {
            if (*pp) ITX_HIP(hipFree(*pp));
            *pp = nullptr;
            ITX_HIP(hipMalloc((void **)pp, want));
        }
        h->parse.soa_cap = want;
    }
    ITX_HIP(hipMemcpyAsync(h->parse.d_pb, h->parse.h_pb, 2 * (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ITX_HIP(hipMemsetAsync(h->parse.d_flags, 0, 4, st));
    hipLaunchKernelGGL(k_compact, dim3(T), dim3(64), 0, st, h->parse.d_spec, h->parse.d_pb, h->parse.d_pb + T, T, h->parse.d_recoff);
    ITX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_parse, dim3((tot + 255) / 256), dim3(256), 0, st, u, h->parse.d_recoff, tot, h->parse.d_tid, h->parse.d_pos, h->parse.d_end, h->parse.d_mapq, h->parse.d_f5, h->parse.d_mpos, h->parse.d_isize,
                       h->parse.d_xa, h->parse.d_flags, h->parse.d_seen, (int32_t)n_targets);
    ITX_HIP(hipGetLastError());
    uint32_t fl = 0;
    ITX_HIP(hipMemcpyAsync(&fl, h->parse.d_flags, 4, hipMemcpyDeviceToHost, st));
    ITX_HIP(hipStreamSynchronize(st));
    *flags = (int)fl;
    *n_rec = tot;
    h->parse.n_rec = tot;
    return ITX_OK;
}

/* records [first, first + n) of the last parse: SoA into host arrays (any may be NULL), their offsets in the window and
 * XA marks on request */
extern "C" int itx_bamwin_fetch(itx_inflater *h, size_t first, size_t n, const itx_staging *dst, size_t dst_at, uint32_t *rec_off, uint8_t *xa)
{
    if (!h || first + n > h->parse.n_rec) return ITX_E_ARG;
    if (n == 0) return ITX_OK;
    ITX_HIP(hipSetDevice(h->device));
    hipStream_t st = h->st[1];
    if (dst) {
        if (dst_at + n > dst->capacity) return ITX_E_ARG;
        if (dst->tid) ITX_HIP(hipMemcpyAsync(dst->tid + dst_at, h->parse.d_tid + first, n * 4, hipMemcpyDeviceToHost, st));
        if (dst->pos) ITX_HIP(hipMemcpyAsync(dst->pos + dst_at, h->parse.d_pos + first, n * 4, hipMemcpyDeviceToHost, st));
        if (dst->tmpend) ITX_HIP(hipMemcpyAsync(dst->tmpend + dst_at, h->parse.d_end + first, n * 4, hipMemcpyDeviceToHost, st));
        if (dst->mapq) ITX_HIP(hipMemcpyAsync(dst->mapq + dst_at, h->parse.d_mapq + first, n, hipMemcpyDeviceToHost, st));
        if (dst->flag5) ITX_HIP(hipMemcpyAsync(dst->flag5 + dst_at, h->parse.d_f5 + first, n, hipMemcpyDeviceToHost, st));
        if (dst->mpos) ITX_HIP(hipMemcpyAsync(dst->mpos + dst_at, h->parse.d_mpos + first, n * 4, hipMemcpyDeviceToHost, st));
        if (dst->isize) ITX_HIP(hipMemcpyAsync(dst->isize + dst_at, h->parse.d_isize + first, n * 4, hipMemcpyDeviceToHost, st));
    }
    if (rec_off) ITX_HIP(hipMemcpyAsync(rec_off, h->parse.d_recoff + first, n * 4, hipMemcpyDeviceToHost, st));
    if (xa) ITX_HIP(hipMemcpyAsync(xa, h->parse.d_xa + first, n, hipMemcpyDeviceToHost, st));
    ITX_HIP(hipStreamSynchronize(st));
    return ITX_OK;
}

/* raw bytes [off, off + len) of the parsed window (offsets as itx_bamwin_fetch's rec_off), to the host */
extern "C" int itx_bamwin_bytes(itx_inflater *h, size_t off, void *dst, size_t len)
{
    if (!h || !dst) return ITX_E_ARG;
    const int w = h->parse.parsed_w;
    if (off + len > h->wins.win[w].cap) return ITX_E_ARG;
    ITX_HIP(hipSetDevice(h->device));
    if (len) ITX_HIP(hipMemcpy(dst, h->wins.win[w].buf + off, len, hipMemcpyDeviceToHost));
    return ITX_OK;
}

extern "C" int itx_bamwin_tids(itx_inflater *h, uint8_t *seen, int n_targets)
{
    if (!h || !seen || n_targets < 0 || (size_t)n_targets > h->parse.seen_cap) return ITX_E_ARG;
    ITX_HIP(hipSetDevice(h->device));
    if (n_targets) ITX_HIP(hipMemcpy(seen, h->parse.d_seen, (size_t)n_targets, hipMemcpyDeviceToHost));
    return ITX_OK;
}

int itx_xaveto_run(itx_xaveto *x, const uint8_t *u, const uint32_t *rec_off, const uint8_t *xa_mark, const int32_t *tid, const int32_t *pos, const int32_t *end,
                   uint8_t *f5, const int32_t *mpos, const int32_t *isize, size_t n, uint64_t *n_vetoed, uint64_t *n_hard);      // itx_xaveto.hip

/* the XA veto over records [first, first + n) of the last parsed window (chosen rows already in the veto object's buffer) */
extern "C" int itx_bamwin_xa_veto(itx_inflater *h, itx_xaveto *x, size_t first, size_t n, uint64_t *n_vetoed, uint64_t *n_hard)
{
    if (!h || !x || !n_vetoed || !n_hard || first + n > h->parse.n_rec) return ITX_E_ARG;
    const int w = h->parse.parsed_w;
    return itx_xaveto_run(x, h->wins.win[w].buf, h->parse.d_recoff + first, h->parse.d_xa + first, h->parse.d_tid + first, h->parse.d_pos + first, h->parse.d_end + first, h->parse.d_f5 + first,
                          h->parse.d_mpos + first, h->parse.d_isize + first, n, n_vetoed, n_hard);
}

/* -R over all records of the last parsed window (csrc/itx_dedup.hip): the dropped ones get ITX_F5_NOLOOKUP where the window's flags lie */
extern "C" int itx_bamwin_dedup(itx_inflater *h, itx_dedup *d)
{
    if (!h || !d) return ITX_E_ARG;
    return itx_dedup_run(d, h->parse.d_tid, h->parse.d_pos, h->parse.d_end, h->parse.d_mapq, h->parse.d_f5, h->parse.d_mpos, h->parse.d_isize, h->parse.n_rec);
}

int itx_bed_start(itx_bed *b, const uint8_t *u, const uint32_t *rec_off, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint8_t *mapq,
                  const uint8_t *f5, const int32_t *mpos, const int32_t *isize, size_t n, uint64_t *n_hard);      // itx_bed.hip

/* the bed text of records [first, first + n) of the last parsed window (csrc/itx_bed.hip): started, collected with itx_bed_collect */
extern "C" int itx_bamwin_bed(itx_inflater *h, itx_bed *b, size_t first, size_t n, uint64_t *n_hard)
{
    if (!h || !b || !n_hard || first + n > h->parse.n_rec) return ITX_E_ARG;
    const int w = h->parse.parsed_w;
    return itx_bed_start(b, h->wins.win[w].buf, h->parse.d_recoff + first, h->parse.d_tid + first, h->parse.d_pos + first, h->parse.d_end + first, h->parse.d_mapq + first, h->parse.d_f5 + first,
                         h->parse.d_mpos + first, h->parse.d_isize + first, n, n_hard);
}

int itx_names_start(itx_names *nm, const uint8_t *u, const uint32_t *rec_off, const int32_t *d_hit_row, size_t n, void *stream, uint64_t *n_hard);   // itx_names.hip

/* the names of records [first, first + n) of the last parsed window that chose a row, appended to the lists (csrc/itx_names.hip) */
extern "C" int itx_bamwin_names(itx_inflater *h, itx_names *nm, size_t first, size_t n, const int32_t *d_hit_row, void *stream, uint64_t *n_hard)
{
    if (!h || !nm || !n_hard || first + n > h->parse.n_rec) return ITX_E_ARG;
    const int w = h->parse.parsed_w;
    return itx_names_start(nm, h->wins.win[w].buf, h->parse.d_recoff + first, d_hit_row, n, stream, n_hard);
}

/* records [first, first + n) of the last parsed window that chose a row, appended to the BAM of filter -b (csrc/itx_bamout.hip) */
extern "C" int itx_bamwin_bamout(itx_inflater *h, itx_bamout *bo, size_t first, size_t n, const int32_t *d_hit_row, void *stream)
{
    if (!h || !bo || first + n > h->parse.n_rec) return ITX_E_ARG;
    const int w = h->parse.parsed_w;
    return itx_bamout_start(bo, h->wins.win[w].buf, h->parse.d_recoff + first, d_hit_row, n, stream);
}

extern "C" int itx_bamwin_device_batch(itx_inflater *h, size_t first, int with_mates, itx_batch *out)
{
    if (!h || !out || first > h->parse.n_rec || (first & 15u)) return ITX_E_ARG;
    out->tid = h->parse.d_tid + first;
    out->pos = h->parse.d_pos + first;
    out->tmpend = h->parse.d_end + first;
    out->mapq = h->parse.d_mapq + first;
    out->flag5 = h->parse.d_f5 + first;
    out->mpos = with_mates ? h->parse.d_mpos + first : nullptr;
    out->isize = with_mates ? h->parse.d_isize + first : nullptr;
    return ITX_OK;
}
