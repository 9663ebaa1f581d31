// itx_inflate.hip — BGZF blocks inflated on the device: one wavefront per block (itx_inflate_core.h), thousands of blocks
// per launch. Replaces the reference's sequential zlib inflate of every 64 KiB block (cussamtools/bgzf.c:367-397
// inflate_block, reached from bgzf_read -> bgzf_read_block, bgzf.c:425-521): only compressed bytes cross PCIe on the way in.
//
// HBM layout: the caller's compressed chunk is mirrored at the same offsets in d_comp (so a block's position keeps its
// alignment), the inflated bytes of all blocks are contiguous in d_out at the offsets the caller computed from the ISIZE
// trailers. A call is cut into groups of blocks that alternate between two streams: copy-in, kernel and copy-out of one
// group overlap the neighbours'.
//
// This file: the decoder's kernels, the inflater object (itx_inflater.h) and the push pipeline that feeds the windows, which
// carries out what the schedule (itx_pushsched.h) says. What is done with a window's bytes is itx_bamwin.hip.
#include "itx_device.h"

#define ITXI_WAVE 64u
#define ITXI_SIMPLE_IN          /* one word of input look-ahead: 10.96 ms per 24 k blocks against 11.27 with the 16-byte FIFO */
#define ITXI_FN static __device__ inline
#define ITXI_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(x)))
#define ITXI_BCAST(v, j) ((uint32_t)__builtin_amdgcn_readlane((int32_t)(v), (int32_t)(j)))
#define ITXI_SCAN_ADD(v, lane) wave_incl_scan_u32(v, lane)
#define ITXI_LANE_READ(v, j) ((uint32_t)__builtin_amdgcn_ds_bpermute((int32_t)((j) << 2), (int32_t)(v)))
#define ITXI_BALLOT(p) ((uint64_t)__ballot(p))
#define ITXI_MBCNT(m, lane) ((uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)((m) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)(m), 0u)))
#define ITXI_LDS_OR(ptr, v) ((void)atomicOr((ptr), (v)))
#define ITXI_AT(p, i) (p)[(i) * 64u + ln]          /* a decoder's table element i: lane-interleaved (bank = lane) */
#define ITXI_BITREV32(x) __builtin_bitreverse32(x)
typedef uint16_t itxi_u16x2 __attribute__((ext_vector_type(2)));
static __device__ inline uint32_t itxi_pksign16(uint32_t a, uint32_t b)
{
    const itxi_u16x2 d = (__builtin_bit_cast(itxi_u16x2, a) - __builtin_bit_cast(itxi_u16x2, b)) >> (itxi_u16x2)15;     // v_pk_sub_u16, v_pk_lshrrev_b16
    return __builtin_bit_cast(uint32_t, d);
}
#define ITXI_PKSIGN16(a, b) itxi_pksign16(a, b)
#define ITXI_LOADW(w, i) ((w)[(i)])
#define ITXI_LOAD4(WORDS, AT, R0, R1, R2, R3)                                    \
    do {                                                                         \
        const uint4 v4__ = *reinterpret_cast<const uint4 *>((WORDS) + (AT));     \
        (R0) = v4__.x;                                                           \
        (R1) = v4__.y;                                                           \
        (R2) = v4__.z;                                                           \
        (R3) = v4__.w;                                                           \
    } while (0)
#define ITXI_LOADB(p, i) ((p)[(i)])
// A far match reads bytes this wave stored earlier through other lanes. Workgroup scope is all it takes — the wave's
// stores have to be acknowledged before its loads go out (s_waitcnt vmcnt(0)); the lines read are whole stripes written
// once, so no cached copy can be stale. (An agent-scope fence here writes the L2 back: measured 4 500 cycles per token.)
#define ITXI_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup")
#include "itx_inflate_core.h"
#define ITXG_FN static __host__ __device__ inline
#include "itx_inflate_group.h"
#define ITXD_FN static __host__ __device__ inline
#include "itx_decode_roles.h"
#include "itx_inflater.h"

#include <string.h>
#include <time.h>

#define BGZF_HEADER 18u      /* gzip header with the one "BC" extra field (bgzf.c:401-411) */
#define BGZF_TRAILER 8u      /* CRC32 + ISIZE */
#define SCR_STRIDE ITXI_REGION                    /* bytes of scratch per block: literals from its bottom, tokens from its top (itx_inflate_core.h) */

template <typename T> static __host__ __device__ inline T itxg_pick(T const (&a)[ITXG_SLOTS], uint32_t k)
{
    T v = a[0];
#pragma unroll
    for (uint32_t j = 1; j < ITXG_SLOTS; j++)
        if (k == j) v = a[j];
    return v;
}

// pass 1 of one wave: lane ln takes the group-wide index g = first + ln (first: a multiple of 64). meta[3g] = status,
// [3g+1] = literals, [3g+2] = tokens. lds: ITXD_LDS bytes, the wave's own
#ifndef ITXI_SYM16
#define ITXD_LDS ((9u * 4u + 16u * 2u + 16u * 2u + 288u + 32u) * 64u)          /* 26 880 bytes in all: six of these workgroups to a CU */
#else
#define ITXD_LDS ((288u * 2u + 16u * 2u + 16u * 2u + 32u) * 64u)              /* 43 008 bytes: three to a CU (experiment builds) */
#endif
static __device__ inline void pass1_wave(const GroupArgs &G, uint32_t first, uint32_t ln, uint32_t *lds, uint8_t *__restrict__ scr, uint32_t *__restrict__ meta)
{
    const uint32_t g = first + ln;
    uint32_t slot, wb;
    (void)itxg_locate(G.x, first, &slot, &wb);                          // a slot starts at a multiple of 64: the whole wave is in one
    const uint32_t b = wb + ln;
    if (b >= itxg_pick(G.x.n, slot)) return;
    const itx_bgzf_block *__restrict__ blk = itxg_pick(G.blk, slot);
    const uint32_t *__restrict__ comp = itxg_pick(G.comp, slot);
    const uint32_t coff = blk[b].coff, csize = blk[b].csize, usize = blk[b].usize;
#ifndef ITXI_SYM16
    uint32_t *s_lhi = lds;                                              // [9 * 64]
    uint16_t *s_loffs = reinterpret_cast<uint16_t *>(s_lhi + 9 * 64), *s_doffs = s_loffs + 16 * 64;
    uint8_t *s_lsym8 = reinterpret_cast<uint8_t *>(s_doffs + 16 * 64), *s_dsym = s_lsym8 + 288 * 64;
    ItxiTab T{s_lsym8, s_lhi, s_dsym, s_loffs, s_doffs};
#else
    uint16_t *s_lsym16 = reinterpret_cast<uint16_t *>(lds), *s_loffs = s_lsym16 + 288 * 64, *s_doffs = s_loffs + 16 * 64;
    uint8_t *s_dsym = reinterpret_cast<uint8_t *>(s_doffs + 16 * 64);
    ItxiTab T{s_lsym16, s_dsym, s_loffs, s_doffs};
#endif
    uint8_t *region = scr + (size_t)g * SCR_STRIDE;
    ItxiTokens K{region, reinterpret_cast<uint32_t *>(region + SCR_STRIDE), 0, 0};
    int rc = ITXI_E_INPUT;
    if (csize >= BGZF_HEADER + BGZF_TRAILER + 2u && usize <= ITXI_MAX_BLOCK)
        rc = itxi_tokens(T, ln, comp, coff + BGZF_HEADER, coff + csize - BGZF_TRAILER, usize, K);
    meta[3 * g] = (uint32_t)rc;
    meta[3 * g + 1] = K.n_lit;
    meta[3 * g + 2] = K.n_tok;
}

// pass 2 of one wave: all 64 lanes on the block at the group-wide index g. lds: ITXD_LDS2 bytes, the wave's own: the ring, right
// behind it the literal stage, then the bitmap of token starts
#define ITXD_LDS2 (ITXI_RING + ITXI_LSTAGE + ITXI_BMAP / 8u + 8u)
static __device__ inline void pass2_wave(const GroupArgs &G, uint32_t g, uint32_t lane, uint32_t *lds, const uint8_t *__restrict__ scr, const uint32_t *__restrict__ meta)
{
    uint32_t *s_ring = lds, *s_stage = lds + ITXI_RING / 4, *s_bmap = lds + (ITXI_RING + ITXI_LSTAGE) / 4;
    uint32_t slot, b;
    if (!itxg_locate(G.x, g, &slot, &b)) return;                         // padding between two slots
    const itx_bgzf_block *__restrict__ blk = itxg_pick(G.blk, slot);
    int rc = (int)meta[3 * g];
    if (rc == ITXI_OK) {
        const uint8_t *region = scr + (size_t)g * SCR_STRIDE;
        rc = itxi_resolve(s_ring, s_stage, s_bmap, region, reinterpret_cast<const uint32_t *>(region + SCR_STRIDE), meta[3 * g + 1], meta[3 * g + 2], itxg_pick(G.out, slot),
                          blk[b].uoff, blk[b].usize, lane);
    }
    if (lane == 0) itxg_pick(G.status, slot)[b] = (uint8_t)rc;
}

// pass 1 alone: lane = block
__global__ __launch_bounds__(64) void k_tokens(const GroupArgs G, uint8_t *__restrict__ scr, uint32_t *__restrict__ meta)
{
    __shared__ uint32_t s_mem[ITXD_LDS / 4];
    pass1_wave(G, blockIdx.x * 64u, threadIdx.x, s_mem, scr, meta);
}

// pass 2 alone: wave = block, the group-wide indices [first, first + n)
__global__ __launch_bounds__(64) void k_resolve(const GroupArgs G, uint32_t first, uint32_t n, const uint8_t *__restrict__ scr, const uint32_t *__restrict__ meta)
{
    __shared__ uint32_t s_mem[ITXD_LDS2 / 4];
    if (blockIdx.x >= n) return;
    pass2_wave(G, first + blockIdx.x, threadIdx.x, s_mem, scr, meta);
}

// Both at once (itx_decode_roles.h): pass 1 of the group C (current) in the first workgroups' wave 0, pass 2 of the group P (the
// one whose pass 1 the launch before carried) a block per wave in the others. The two share nothing — P's tokens lie in the
// other scratch buffer — so pass 2's waves fill the CUs that pass 1's few, latency-bound waves leave empty. One static LDS block
// of pass 1's size: a pass-2 wave uses its own quarter of it.
#ifndef ITXI_SYM16
#define ITXD_LDS2_STRIDE ((ITXD_LDS2 + 15u) & ~15u)                /* a wave's quarter starts 16-byte aligned, as k_resolve's block does */
static_assert(ITXD_WAVES * ITXD_LDS2_STRIDE <= ITXD_LDS, "four pass-2 waves' rings, stages and bitmaps fit pass 1's tables");
static_assert(ITXD_LDS == 26880u, "six workgroups to a CU");
// (167 VGPRs, pass 1's 170 less three, no scratch: three waves to a SIMD. Held to 128 — four waves — the compiler spills 20 of them
// and 34 SGPRs into pass 1's chain, 80 bytes of scratch a lane: the chain is the launch's length, so it keeps its registers.)
__global__ __launch_bounds__(ITXD_THREADS) void k_decode(const GroupArgs C, const GroupArgs P, const itxd_grid R, uint8_t *__restrict__ scr_c, uint32_t *__restrict__ meta_c,
                                                         const uint8_t *__restrict__ scr_p, const uint32_t *__restrict__ meta_p)
{
    __shared__ uint32_t s_mem[ITXD_LDS / 4];
    const uint32_t wave = ITXI_UNI(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t first;
    const uint32_t role = itxd_role(R, blockIdx.x, wave, &first);
    if (role == ITXD_PASS1)
        pass1_wave(C, first, lane, s_mem, scr_c, meta_c);                // wave 0: lane == threadIdx.x
    else if (role == ITXD_PASS2)
        pass2_wave(P, first, lane, s_mem + wave * (ITXD_LDS2_STRIDE / 4), scr_p, meta_p);
}
#endif

// launched once when an inflater is made: loading the library's code objects costs a tenth of a second, and the helper
// thread that creates the inflater has it to spare
__global__ void k_warm(uint32_t *p)
{
    if (p) *p = 0;
}

static void report_at_exit();

extern "C" int itx_inflater_create(int device, itx_inflater **out)
{
    if (!out) return ITX_E_ARG;
    *out = nullptr;
    int rc = ITX_OK;
    itx_inflater *h = nullptr;
    const bool tim = getenv("ITX_TIMING_SETUP") != nullptr;
    struct timespec tsa, tsb;
#define SETUP_TICK(what)                                                                                                      \
    do {                                                                                                                      \
        if (tim) {                                                                                                            \
            clock_gettime(CLOCK_MONOTONIC, &tsb);                                                                             \
            fprintf(stderr, "[itx timing] inflater setup: %s %.3f s\n", what, (double)(tsb.tv_sec - tsa.tv_sec) + 1e-9 * (double)(tsb.tv_nsec - tsa.tv_nsec)); \
            tsa = tsb;                                                                                                        \
        }                                                                                                                     \
    } while (0)
    clock_gettime(CLOCK_MONOTONIC, &tsa);
    ITX_TRY(hipSetDevice(device));
    SETUP_TICK("hipSetDevice");
    h = (itx_inflater *)calloc(1, sizeof *h);
    if (!h) return ITX_E_NOMEM;
    h->device = device;
    itxp_init(&h->dec.sched, lanes_in_use(), group_size(), compute_lanes(), fuse_on());
    // st[1] carries the carry-over, locate and parse of every window; st[0] only itx_inflate_bgzf's calls: made when one comes
    // (a stream that is never launched on still shares a hardware queue with one that is)
    ITX_TRY(hipStreamCreateWithFlags(&h->st[1], hipStreamNonBlocking));
    SETUP_TICK("first stream");
    for (int k = 0; k < 4; k++) ITX_TRY(hipEventCreate(&h->dec.ev[k]));
    for (int k = 0; k < 2; k++) ITX_TRY(hipEventCreate(&h->dec.ev_res_end[k]));
    for (int k = 0; k < lanes_in_use(); k++) {
        ITX_TRY(hipEventCreateWithFlags(&h->dec.lane[k].copied, hipEventDisableTiming));
        for (int q = 0; q < 3; q++) ITX_TRY(hipEventCreate(&h->dec.grp[k].ev[q]));
        ITX_TRY(hipEventCreateWithFlags(&h->dec.grp[k].done, hipEventDisableTiming));
    }
    // ONE stream carries every push's bytes across PCIe, in push order (the link is one: copies side by side only finish later,
    // all of them); a stream per slot also meant more streams than hardware queues, and streams that share a queue run one
    // after the other — two compute lanes on one queue halved pass 1's overlap (1.8 kernels in flight instead of 3)
    ITX_TRY(hipStreamCreateWithFlags(&h->dec.copy_st, hipStreamNonBlocking));
    SETUP_TICK("lane streams, events, counters");
    h->dec.n_cu = 256;
    if (hipDeviceGetAttribute(&h->dec.n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->dec.n_cu <= 0) h->dec.n_cu = 256;
    if (getenv("ITX_TIMING")) {
        static bool once;
        if (!once) {
            once = true;
            atexit(report_at_exit);
        }
    }
    hipLaunchKernelGGL(k_warm, dim3(1), dim3(1), 0, h->st[1], (uint32_t *)nullptr);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipStreamSynchronize(h->st[1]));
    SETUP_TICK("first kernel (code object load)");
#undef SETUP_TICK
out:
    if (rc != ITX_OK) {
        itx_inflater_destroy(h);               // the partial object: its streams and events as far as they were made
        return rc;
    }
    *out = h;
    return ITX_OK;
}

extern "C" void itx_inflater_destroy(itx_inflater *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    auto &D = h->dec;
    for (int k = 0; k < 2; k++)
        if (h->st[k]) {
            (void)hipStreamSynchronize(h->st[k]);
            (void)hipStreamDestroy(h->st[k]);
        }
    (void)hipFree(D.d_comp);
    (void)hipFree(D.d_out);
    (void)hipFree(D.d_status);
    (void)hipFree(D.d_blk);
    (void)hipFree(D.d_lit);
    (void)hipFree(D.d_meta);
    const bool own = !h->wins.arena;           // without an arena every buffer is an allocation of its own
    for (int k = own ? 0 : h->wins.n_reserved_win; k < ITX_BAMWIN_WINDOWS; k++) (void)hipFree(h->wins.win[k].buf);
    for (int k = 0; k < ITX_BAMWIN_LANES; k++) {
        if (D.lane[k].copied) (void)hipEventDestroy(D.lane[k].copied);
        for (int q = 0; q < 3; q++)
            if (D.grp[k].ev[q]) (void)hipEventDestroy(D.grp[k].ev[q]);
        if (D.grp[k].done) (void)hipEventDestroy(D.grp[k].done);
        if (D.clane[k].cst) {
            (void)hipStreamSynchronize(D.clane[k].cst);
            (void)hipStreamDestroy(D.clane[k].cst);
        }
        if (own) {
            (void)hipFree(D.lane[k].d_comp);
            (void)hipFree(D.lane[k].d_status);
            for (int q = 0; q < 2; q++) {
                (void)hipFree(D.clane[k].d_lit[q]);
                (void)hipFree(D.clane[k].d_meta[q]);
            }
            (void)hipFree(D.lane[k].d_blk);
        }
        if (D.lane[k].h_blk) (void)hipHostFree(D.lane[k].h_blk);
        if (D.lane[k].h_status) (void)hipHostFree(D.lane[k].h_status);
    }
    if (D.copy_st) {
        (void)hipStreamSynchronize(D.copy_st);
        (void)hipStreamDestroy(D.copy_st);
    }
    (void)hipFree(h->wins.arena);
    bamwin_free(h);
    for (int k = 0; k < 4; k++)
        if (D.ev[k]) (void)hipEventDestroy(D.ev[k]);
    for (int k = 0; k < 2; k++)
        if (D.ev_res_end[k]) (void)hipEventDestroy(D.ev_res_end[k]);
    free(h);
}

// ITX_TIMING: where the decoder's device-side time goes (printed when the process ends)
double g_alloc_s;
unsigned long g_allocs;
static double g_tok_ms, g_res_ms;
static unsigned long g_pushes, g_launches, g_blocks, g_flushes;
static bool g_reported;
static void report_at_exit()
{
    if (g_reported || !g_pushes) return;
    g_reported = true;
    const double nl = g_launches ? (double)g_launches : 1.0;
    if (fuse_on()) {
        // a fused launch: pass 1 of its group beside pass 2 of the group before; a flush: pass 2 alone, of a group that no later one followed
        fprintf(stderr, "[itx timing] device decoder: %lu pushes in %lu fused launches of %.0f blocks, %.1f ms per launch (pass 1 beside the previous group's pass 2; "
                        "HIP events), %lu flush launches, %lu device allocations %.3f s\n", g_pushes, g_launches, (double)g_blocks / nl, g_tok_ms / nl, g_flushes, g_allocs,
                g_alloc_s);
        return;
    }
    fprintf(stderr, "[itx timing] device decoder: %lu pushes in %lu launches of %.0f blocks, pass 1 %.1f ms and pass 2 %.1f ms per launch (HIP events, launches overlap), "
                    "%lu device allocations %.3f s\n", g_pushes, g_launches, (double)g_blocks / nl, g_tok_ms / nl, g_res_ms / nl, g_allocs, g_alloc_s);
}

extern "C" void itx_timing_report(void) { report_at_exit(); }

extern "C" int itx_inflate_bgzf(itx_inflater *h, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk, void *out, size_t out_len,
                                uint8_t *status)
{
    if (!h || !comp || !blk || !status) return ITX_E_ARG;          // out == NULL: the bytes stay on the device (timing runs)
    if (n_blk == 0) return ITX_OK;
    if (comp_len > 0xfffffff0u || out_len > 0xfffffff0u || n_blk > 0x7fffffffu) return ITX_E_LIMIT;
    // what the kernel assumes about every block, checked here: inside the buffers, outputs disjoint and in order
    size_t uat = 0;
    for (size_t i = 0; i < n_blk; i++) {
        const itx_bgzf_block &b = blk[i];
        if ((size_t)b.coff + b.csize > comp_len || b.csize < BGZF_HEADER + BGZF_TRAILER || b.uoff != uat || (size_t)b.uoff + b.usize > out_len ||
            b.usize > 65536u) {
            itx_set_error("itx_inflate_bgzf: block %zu does not fit its buffers", i);
            return ITX_E_ARG;
        }
        uat += b.usize;
    }
    ITX_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = grow(&h->dec.d_comp, &h->dec.comp_cap, comp_len + 64)) != ITX_OK) return rc;
    if ((rc = grow(&h->dec.d_out, &h->dec.out_cap, out_len + 64)) != ITX_OK) return rc;
    if ((rc = grow(&h->dec.d_status, &h->dec.status_cap, n_blk)) != ITX_OK) return rc;
    if ((rc = grow(&h->dec.d_blk, &h->dec.blk_cap, n_blk)) != ITX_OK) return rc;
    if ((rc = grow(&h->dec.d_lit, &h->dec.lit_cap, n_blk * (size_t)SCR_STRIDE)) != ITX_OK) return rc;
    if ((rc = grow(&h->dec.d_meta, &h->dec.meta_cap, 3 * n_blk)) != ITX_OK) return rc;
    if (!h->st[0]) ITX_HIP(hipStreamCreateWithFlags(&h->st[0], hipStreamNonBlocking));
    GroupArgs G;                                                   // a group of one
    memset(&G, 0, sizeof G);
    const uint32_t one = (uint32_t)n_blk;
    (void)itxg_layout(&G.x, &one, 1);
    G.comp[0] = (const uint32_t *)h->dec.d_comp;
    G.blk[0] = h->dec.d_blk;
    G.out[0] = h->dec.d_out;
    G.status[0] = h->dec.d_status;
    // pass 1 over all blocks at once (a lane per block: it takes many blocks to fill the chip)
    ITX_HIP(hipMemcpyAsync(h->dec.d_blk, blk, n_blk * sizeof *blk, hipMemcpyHostToDevice, h->st[0]));
    ITX_HIP(hipMemcpyAsync(h->dec.d_comp, comp, comp_len, hipMemcpyHostToDevice, h->st[0]));
    ITX_HIP(hipEventRecord(h->dec.ev[0], h->st[0]));
    hipLaunchKernelGGL(k_tokens, dim3((unsigned)((n_blk + 63) / 64)), dim3(64), 0, h->st[0], G, h->dec.d_lit, h->dec.d_meta);
    ITX_HIP(hipGetLastError());
    ITX_HIP(hipEventRecord(h->dec.ev[1], h->st[0]));
    ITX_HIP(hipStreamSynchronize(h->st[0]));
    // pass 2 in groups that alternate between two streams: one group's copy-out overlaps the next one's kernel
    const size_t per = n_blk < 2048 ? n_blk : (n_blk + 3) / 4;
    int s = 0;
    ITX_HIP(hipEventRecord(h->dec.ev[2], h->st[0]));
    for (size_t b0 = 0; b0 < n_blk; b0 += per, s ^= 1) {
        const size_t b1 = b0 + per < n_blk ? b0 + per : n_blk;
        hipLaunchKernelGGL(k_resolve, dim3((unsigned)(b1 - b0)), dim3(64), 0, h->st[s], G, (uint32_t)b0, (uint32_t)(b1 - b0), h->dec.d_lit, h->dec.d_meta);
        ITX_HIP(hipGetLastError());
        if (b0 == 0) ITX_HIP(hipEventRecord(h->dec.ev[3], h->st[0]));
        const size_t u0 = blk[b0].uoff, u1 = (size_t)blk[b1 - 1].uoff + blk[b1 - 1].usize;
        if (out && u1 > u0) ITX_HIP(hipMemcpyAsync((uint8_t *)out + u0, h->dec.d_out + u0, u1 - u0, hipMemcpyDeviceToHost, h->st[s]));
        ITX_HIP(hipEventRecord(h->dec.ev_res_end[s], h->st[s]));
        ITX_HIP(hipMemcpyAsync(status + b0, h->dec.d_status + b0, b1 - b0, hipMemcpyDeviceToHost, h->st[s]));
    }
    ITX_HIP(hipStreamSynchronize(h->st[0]));
    ITX_HIP(hipStreamSynchronize(h->st[1]));
    (void)hipEventElapsedTime(&h->dec.ms_tokens, h->dec.ev[0], h->dec.ev[1]);
    (void)hipEventElapsedTime(&h->dec.ms_resolve, h->dec.ev[2], h->dec.ev[3]);
    {
        float a = 0, b = 0;                                          // all groups of pass 2 (with the copies out, when there are any)
        (void)hipEventElapsedTime(&a, h->dec.ev[2], h->dec.ev_res_end[0]);
        if (per < n_blk) (void)hipEventElapsedTime(&b, h->dec.ev[2], h->dec.ev_res_end[1]);
        h->dec.ms_resolve_all = a > b ? a : b;
    }
    return ITX_OK;
}

// internal (itx_common.h): both passes over one block list whose blocks, compressed bytes, output, status bytes and scratch all
// lie on the device already, enqueued on `st` one behind the other and not waited for (the synchronisation between the passes in
// itx_inflate_bgzf is there for its timers). The caller has checked the list as itx_inflate_bgzf does; d_out takes 64 bytes more
// than the blocks inflate to, d_comp 64 more than comp_len, d_scr itx_inflate_scratch_bytes(n_blk), d_meta 3 words a block.
size_t itx_inflate_scratch_bytes(size_t n_blk) { return n_blk * (size_t)SCR_STRIDE; }

int itx_inflate_enqueue(hipStream_t st, const void *d_comp, const itx_bgzf_block *d_blk, uint32_t n_blk, uint8_t *d_out, uint8_t *d_status, uint8_t *d_scr,
                        uint32_t *d_meta)
{
    if (!n_blk) return ITX_OK;
    GroupArgs G;                                                   // a group of one
    memset(&G, 0, sizeof G);
    (void)itxg_layout(&G.x, &n_blk, 1);
    G.comp[0] = (const uint32_t *)d_comp;
    G.blk[0] = d_blk;
    G.out[0] = d_out;
    G.status[0] = d_status;
    hipLaunchKernelGGL(k_tokens, dim3((n_blk + 63u) / 64u), dim3(64), 0, st, G, d_scr, d_meta);
    ITX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_resolve, dim3(n_blk), dim3(64), 0, st, G, 0u, n_blk, d_scr, d_meta);
    ITX_HIP(hipGetLastError());
    return ITX_OK;
}

/* device time of the two passes of the last itx_inflate_bgzf call (pass 2: its first group), milliseconds */
extern "C" int itx_inflater_last_ms(const itx_inflater *h, float *tokens_ms, float *resolve_ms)
{
    if (!h) return ITX_E_ARG;
    if (tokens_ms) *tokens_ms = h->dec.ms_tokens;
    if (resolve_ms) *resolve_ms = h->dec.ms_resolve;
    return ITX_OK;
}

/* pass 2 over all groups of the last itx_inflate_bgzf call (kernels only when that call was given out == NULL) */
extern "C" int itx_inflater_last_resolve_all_ms(const itx_inflater *h, float *ms)
{
    if (!h || !ms) return ITX_E_ARG;
    *ms = h->dec.ms_resolve_all;
    return ITX_OK;
}

// ----------------------------------------------------------------------------------------------- the push pipeline

static int check_blocks(const itx_bgzf_block *blk, size_t n_blk, size_t comp_len, size_t *total)
{
    size_t uat = 0;
    for (size_t i = 0; i < n_blk; i++) {
        const itx_bgzf_block &b = blk[i];
        if ((size_t)b.coff + b.csize > comp_len || b.csize < BGZF_HEADER + BGZF_TRAILER || b.uoff != uat || b.usize > 65536u) {
            itx_set_error("BGZF block %zu does not fit its buffers", i);
            return ITX_E_ARG;
        }
        uat += b.usize;
    }
    *total = uat;
    return ITX_OK;
}

#define BAD_S(s) ((s) < 0 || (s) >= lanes_in_use())

/* the slot's page-locked block list and status bytes made anew, for `want` blocks: both, or on failure neither */
static int host_pair(itxi_slot &Ln, size_t want)
{
    int rc = ITX_OK;
    if (Ln.h_blk) (void)hipHostFree(Ln.h_blk);
    if (Ln.h_status) (void)hipHostFree(Ln.h_status);
    Ln.h_blk = nullptr;
    Ln.h_status = nullptr;
    Ln.h_cap = 0;
    ITX_TRY(hipHostMalloc((void **)&Ln.h_blk, want * sizeof(itx_bgzf_block), hipHostMallocDefault));
    ITX_TRY(hipHostMalloc((void **)&Ln.h_status, want, hipHostMallocDefault));
    Ln.h_cap = want;
out:
    if (rc != ITX_OK && Ln.h_blk) {
        (void)hipHostFree(Ln.h_blk);
        Ln.h_blk = nullptr;
    }
    return rc;
}

/* pass 2 of group gi is enqueued on st: behind it the status bytes of its members, and the event their push_end waits for */
static int finish_group(itx_inflater *h, int gi, hipStream_t st)
{
    const auto &Gr = h->dec.sched.grp[gi];
    for (int m = 0; m < Gr.n; m++) {
        auto &Ln = h->dec.lane[Gr.slot[m]];
        ITX_HIP(hipMemcpyAsync(Ln.h_status, Ln.d_status, Ln.n_blk, hipMemcpyDeviceToHost, st));
    }
    ITX_HIP(hipEventRecord(h->dec.grp[gi].done, st));
    return ITX_OK;
}

#ifndef ITXI_SYM16
/* one fused launch on compute lane CL: pass 1 of the group *cur (span blocks, scratch buffer buf; NULL: none, a FLUSH) and pass 2 of
 * the lane's pending group (prev, its tokens in scratch buffer prev_buf; -1: none) */
static int launch_decode(itxi_lane &CL, const GroupArgs *cur, uint32_t span, int buf, int prev, int prev_buf)
{
    static const GroupArgs none = {};
    itxd_grid R;
    const uint32_t n_wg = itxd_layout(&R, cur ? span : 0u, prev >= 0 ? CL.pend_span : 0u);
    if (!n_wg) return ITX_OK;
    const int pb = prev >= 0 ? prev_buf : buf;
    hipLaunchKernelGGL(k_decode, dim3(n_wg), dim3(ITXD_THREADS), 0, CL.cst, cur ? *cur : none, prev >= 0 ? CL.pend_args : none, R, CL.d_lit[buf], CL.d_meta[buf],
                       CL.d_lit[pb], CL.d_meta[pb]);
    ITX_HIP(hipGetLastError());
    return ITX_OK;
}
#endif

/* FLUSH: the lane's pending group gets its pass 2 in a launch of its own: no later group has come that would carry it */
static int flush_lane(itx_inflater *h, const itxp_action &a)
{
#ifndef ITXI_SYM16
    auto &CL = h->dec.clane[a.lane];
    int rc = launch_decode(CL, nullptr, 0, 0, a.group, h->dec.sched.lane[a.lane].pend_buf);
    if (rc != ITX_OK) return rc;
    if ((rc = finish_group(h, a.group, CL.cst)) != ITX_OK) return rc;
    g_flushes++;
#endif
    return ITX_OK;
}

/* LAUNCH: one launch over the group's blocks on the compute lane the schedule gave it: behind every member's copy, and behind the
 * group that had the lane before. Two kernels, pass 1 then pass 2, on the lane's scratch buffer 0 — or (fused) one k_decode: pass 1 of
 * this group into the lane's scratch buffer a.buf, beside pass 2 of the group a.carries that the lane's last launch left pending */
static int launch_group(itx_inflater *h, const itxp_action &a)
{
    auto &D = h->dec;
    const auto &Gr = D.sched.grp[a.group];
    auto &CL = D.clane[a.lane];
    auto &Ev = D.grp[a.group];
    GroupArgs G;
    memset(&G, 0, sizeof G);
    uint32_t counts[ITXG_SLOTS] = {0};
    for (int m = 0; m < Gr.n; m++) counts[m] = (uint32_t)D.lane[Gr.slot[m]].n_blk;
    const uint32_t span = itxg_layout(&G.x, counts, (uint32_t)Gr.n);
    for (int m = 0; m < Gr.n; m++) {
        auto &Ln = D.lane[Gr.slot[m]];
        G.comp[m] = (const uint32_t *)Ln.d_comp;
        G.blk[m] = Ln.d_blk;
        G.out[m] = Ln.win_buf;
        G.status[m] = Ln.d_status;
    }
    int rc;
    if ((rc = grow(&CL.d_lit[a.buf], &CL.lit_cap[a.buf], (size_t)span * SCR_STRIDE)) != ITX_OK) return rc;      // (growing frees: that waits for whatever still runs)
    if ((rc = grow(&CL.d_meta[a.buf], &CL.meta_cap[a.buf], 3 * (size_t)span)) != ITX_OK) return rc;
    if (!CL.cst) ITX_HIP(hipStreamCreateWithFlags(&CL.cst, hipStreamNonBlocking));
    hipStream_t st = CL.cst;
    for (int m = 0; m < Gr.n; m++) ITX_HIP(hipStreamWaitEvent(st, D.lane[Gr.slot[m]].copied, 0));
    ITX_HIP(hipEventRecord(Ev.ev[0], st));
    Ev.timed = false;
#ifndef ITXI_SYM16
    if (D.sched.fused) {
        if ((rc = launch_decode(CL, &G, span, a.buf, a.carries, D.sched.lane[a.lane].pend_buf)) != ITX_OK) return rc;
        ITX_HIP(hipEventRecord(Ev.ev[1], st));
        if (a.carries >= 0 && (rc = finish_group(h, a.carries, st)) != ITX_OK) return rc;
        CL.pend_span = span;
        CL.pend_args = G;
    } else
#endif
    {
        hipLaunchKernelGGL(k_tokens, dim3((span + 63u) / 64u), dim3(64), 0, st, G, CL.d_lit[0], CL.d_meta[0]);
        ITX_HIP(hipGetLastError());
        // pass 2 on the same stream, one wave per block (every push's pass 2 on one shared stream, or a fixed set of waves
        // that take blocks in turn, were measured slower: DESIGN.md)
        ITX_HIP(hipEventRecord(Ev.ev[1], st));
        hipLaunchKernelGGL(k_resolve, dim3(span), dim3(64), 0, st, G, 0u, span, CL.d_lit[0], CL.d_meta[0]);
        ITX_HIP(hipGetLastError());
        ITX_HIP(hipEventRecord(Ev.ev[2], st));
        if ((rc = finish_group(h, a.group, st)) != ITX_OK) return rc;
    }
    g_launches++;
    for (int m = 0; m < Gr.n; m++) g_blocks += counts[m];
    return ITX_OK;
}

/* the launches and flushes a transition of the schedule asks for, in order; each is reported back once it is enqueued */
static int carry_out(itx_inflater *h, const itxp_actions &A)
{
    for (int i = 0; i < A.n && A.a[i].kind != ITXP_WAIT; i++) {
        const int rc = A.a[i].kind == ITXP_LAUNCH ? launch_group(h, A.a[i]) : flush_lane(h, A.a[i]);
        if (rc != ITX_OK) return rc;
        itxp_done(&h->dec.sched, A.a[i]);
    }
    return ITX_OK;
}

/* push, first half: the copies are enqueued on the copy stream, then whatever the schedule asks for once the push has joined
 * (itxp_join); the caller's buffers are in use until itx_bamwin_push_copied (comp) / this call's return (blk) */
extern "C" int itx_bamwin_push_begin(itx_inflater *h, int w, int s, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk)
{
    if (!h || BAD_W(w) || BAD_S(s) || !comp || !blk) return ITX_E_ARG;
    auto &Ln = h->dec.lane[s];
    auto &W = h->wins.win[w];
    itxp_sched &S = h->dec.sched;
    if (S.slot[s].busy) return ITX_E_STATE;
    size_t total = 0;
    int rc = check_blocks(blk, n_blk, comp_len, &total);
    if (rc != ITX_OK) return rc;
    if (comp_len > 0xfffffff0u || total + WIN_HEAD > 0xfffffff0u || n_blk > 0x7fffffffu / ITXG_SLOTS) return ITX_E_LIMIT;
    ITX_HIP(hipSetDevice(h->device));
    if (h->wins.arena && (w >= h->wins.n_reserved_win || WIN_HEAD + total + 64 > W.cap || comp_len + 64 > Ln.comp_cap || n_blk > Ln.status_cap)) {
        itx_set_error("push of %zu blocks / %zu bytes into window %d exceeds what itx_inflater_reserve set up", n_blk, total, w);
        return ITX_E_LIMIT;
    }
    if ((rc = grow(&W.buf, &W.cap, WIN_HEAD + total + 64)) != ITX_OK) return rc;
    W.start = W.consumed = WIN_HEAD;
    W.len = WIN_HEAD + (uint32_t)total;
    Ln.n_blk = n_blk;
    Ln.total = total;
    if ((rc = itxp_begin(&S, s, n_blk != 0)) != ITX_OK || n_blk == 0) return rc;
    if (Ln.h_cap < n_blk && (rc = host_pair(Ln, n_blk + n_blk / 4 + 64)) != ITX_OK) return rc;
    for (size_t i = 0; i < n_blk; i++) {
        Ln.h_blk[i] = blk[i];
        Ln.h_blk[i].uoff += WIN_HEAD;
    }
    if ((rc = grow(&Ln.d_comp, &Ln.comp_cap, comp_len + 64)) != ITX_OK) return rc;
    if ((rc = grow(&Ln.d_status, &Ln.status_cap, n_blk)) != ITX_OK) return rc;
    if ((rc = grow(&Ln.d_blk, &Ln.blk_cap, n_blk)) != ITX_OK) return rc;
    // the bytes cross PCIe on the copy stream ...
    ITX_HIP(hipMemcpyAsync(Ln.d_blk, Ln.h_blk, n_blk * sizeof *blk, hipMemcpyHostToDevice, h->dec.copy_st));
    ITX_HIP(hipMemcpyAsync(Ln.d_comp, comp, comp_len, hipMemcpyHostToDevice, h->dec.copy_st));
    ITX_HIP(hipEventRecord(Ln.copied, h->dec.copy_st));
    __atomic_store_n(&Ln.copy_live, 1, __ATOMIC_RELEASE);
    Ln.win_buf = W.buf;
    // ... and both passes run with the group's, on a compute lane
    itxp_actions A;
    if ((rc = itxp_join(&S, s, &A)) != ITX_OK) return rc;
    return carry_out(h, A);
}

/* the compressed bytes of lane s's push have been copied: the caller may reuse that buffer. (Never launches a group: the
 * reader's io thread calls this, and the copies do not wait for the group. copy_live is all it reads of the slot: the producer
 * stores it with release behind the event's record, so the record is seen here too) */
extern "C" int itx_bamwin_push_copied(itx_inflater *h, int s)
{
    if (!h || BAD_S(s)) return ITX_E_ARG;
    if (!__atomic_load_n(&h->dec.lane[s].copy_live, __ATOMIC_ACQUIRE)) return ITX_OK;
    ITX_HIP(hipSetDevice(h->device));
    ITX_HIP(hipEventSynchronize(h->dec.lane[s].copied));
    return ITX_OK;
}

/* push, second half: what the schedule asks for (itxp_end), then the wait for lane s's push; status[n_blk] as for
 * itx_inflate_bgzf, *n_new = bytes the window gained */
extern "C" int itx_bamwin_push_end(itx_inflater *h, int s, uint8_t *status, size_t *n_new)
{
    if (!h || BAD_S(s) || !status || !n_new) return ITX_E_ARG;
    auto &Ln = h->dec.lane[s];
    itxp_sched &S = h->dec.sched;
    if (!S.slot[s].busy) return ITX_E_STATE;
    ITX_HIP(hipSetDevice(h->device));
    itxp_actions A;
    int rc = itxp_end(&S, s, &A);
    if (rc == ITX_OK) rc = carry_out(h, A);
    if (rc != ITX_OK) return rc;
    if (A.n) {
        const itxp_action &wait = A.a[A.n - 1];                      // its group is resolved by what was carried out, now or earlier
        auto &Ev = h->dec.grp[wait.group];
        ITX_HIP(hipEventSynchronize(Ev.done));
        if (!Ev.timed) {
            Ev.timed = true;
            float a = 0, b = 0;
            if (S.fused) {
                if (hipEventElapsedTime(&a, Ev.ev[0], Ev.ev[1]) == hipSuccess) g_tok_ms += a;       // (done lies behind the next launch: ev[1] is through)
            } else if (hipEventElapsedTime(&a, Ev.ev[0], Ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, Ev.ev[1], Ev.ev[2]) == hipSuccess) {
                g_tok_ms += a;
                g_res_ms += b;
            }
        }
        g_pushes++;
        itxp_done(&S, wait);
        memcpy(status, Ln.h_status, Ln.n_blk);
    }
    *n_new = Ln.total;
    __atomic_store_n(&Ln.copy_live, 0, __ATOMIC_RELEASE);
    return ITX_OK;
}

/* Everything a stream of pushes will need, allocated once while the device is idle: growing a buffer in the middle of the
 * pipeline means hipFree, which waits for every kernel in flight. Per lane: the compressed chunk (comp_bytes), block list,
 * status, literal and token scratch for max_blocks blocks. Windows: as many of max_bytes (+ the carry-over head) as a share
 * of the free memory allows, at most ITX_BAMWIN_WINDOWS and at most *n_windows on entry when that is >= 1; on return
 * *n_windows says how many the caller may use (w < *n_windows). A failure leaves nothing reserved and *n_windows as it was. */
extern "C" int itx_inflater_reserve(itx_inflater *h, size_t comp_bytes, size_t max_blocks, size_t max_bytes, int *n_windows)
{
    if (!h || !n_windows || max_blocks == 0 || max_blocks > 0x7fffffffu || max_bytes + WIN_HEAD > 0xfffffff0u) return ITX_E_ARG;
    if (h->wins.arena) return ITX_E_STATE;
    ITX_HIP(hipSetDevice(h->device));
    auto &D = h->dec;
    const int n_lanes = lanes_in_use();
    for (int k = 0; k < n_lanes; k++)
        if (D.sched.slot[k].busy || D.lane[k].d_comp) return ITX_E_STATE;
    size_t free_b = 0, total_b = 0;
    ITX_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t per = (WIN_HEAD + max_bytes + 64 + 255) & ~(size_t)255;
    size_t n = (free_b / 5 * 2) / per;                              // two fifths of what is free now
    if (n > ITX_BAMWIN_WINDOWS) n = ITX_BAMWIN_WINDOWS;
    if (*n_windows >= 1 && (size_t)*n_windows < n) n = (size_t)*n_windows;       // the caller cannot use more
    if (const char *e = getenv("ITX_RESERVE_WINDOWS"))
        if (atol(e) >= 2 && (size_t)atol(e) < n) n = (size_t)atol(e);
    if (n < 4) n = 4;
    // ONE allocation for all of it: on some hosts every hipMalloc costs ~15 ms whatever its size (and holds up the other
    // threads' HIP calls meanwhile) — seventy of them were 1.2 s of a 4 s run
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t sz_comp = al(comp_bytes + 64), sz_status = al(max_blocks), sz_blk = al(max_blocks * sizeof(itx_bgzf_block));
    // a compute lane's scratch holds a whole group: each member's blocks start at a multiple of ITXG_ALIGN
    const size_t grp_blocks = (size_t)group_size() * ((max_blocks + ITXG_ALIGN - 1) / ITXG_ALIGN * ITXG_ALIGN);
    const size_t sz_lit = al(grp_blocks * (size_t)SCR_STRIDE), sz_meta = al(3 * grp_blocks * 4);
    const int n_comp = compute_lanes();
    const int n_scr = fuse_on() ? 2 : 1;                             // fused launches: a lane's two scratch buffers
    const size_t total = (sz_comp + sz_status + sz_blk) * (size_t)n_lanes + (sz_lit + sz_meta) * (size_t)(n_comp * n_scr) + per * n;
    uint8_t *base = nullptr, *p = nullptr;
    int rc = ITX_OK;
    const double t0 = itx_wall_now();
    hipError_t he = hipMalloc((void **)&base, total);
    g_alloc_s += itx_wall_now() - t0;
    g_allocs++;
    if (he != hipSuccess) {
        itx_set_error("itx_inflater_reserve: hipMalloc(%zu) failed: %s", total, hipGetErrorString(he));
        return ITX_E_NOMEM;
    }
    // the page-locked pairs first: the last thing that can fail, while nothing of the arena is handed out
    for (int k = 0; k < n_lanes; k++)
        if (D.lane[k].h_cap < max_blocks && (rc = host_pair(D.lane[k], max_blocks + 64)) != ITX_OK) goto out;
    h->wins.arena = p = base;
    h->wins.n_reserved_win = (int)n;
    for (int k = 0; k < n_lanes; k++) {
        auto &Ln = D.lane[k];
        Ln.d_comp = p; p += sz_comp; Ln.comp_cap = comp_bytes + 64;
        Ln.d_status = p; p += sz_status; Ln.status_cap = max_blocks;
        Ln.d_blk = (itx_bgzf_block *)p; p += sz_blk; Ln.blk_cap = max_blocks;
    }
    for (int k = 0; k < n_comp; k++) {
        auto &CL = D.clane[k];
        for (int q = 0; q < n_scr; q++) {
            CL.d_lit[q] = p; p += sz_lit; CL.lit_cap[q] = grp_blocks * (size_t)SCR_STRIDE;
            CL.d_meta[q] = (uint32_t *)p; p += sz_meta; CL.meta_cap[q] = 3 * grp_blocks;
        }
    }
    for (size_t w = 0; w < n; w++) {
        auto &W = h->wins.win[w];
        if (W.buf) (void)hipFree(W.buf);
        W.buf = p;
        W.cap = per;
        p += per;
    }
    *n_windows = (int)n;
out:
    if (rc != ITX_OK) (void)hipFree(base);
    return rc;
}

extern "C" int itx_bamwin_push(itx_inflater *h, int w, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk, uint8_t *status, size_t *n_new)
{
    if (!status || !n_new) return ITX_E_ARG;
    *n_new = 0;
    int rc = itx_bamwin_push_begin(h, w, 0, comp, comp_len, blk, n_blk);
    if (rc != ITX_OK) return rc;
    return itx_bamwin_push_end(h, 0, status, n_new);
}
