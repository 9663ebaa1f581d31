// itx_inflater.h — the device decoder's object, private to the two files that share it: itx_inflate.hip (the decoder's kernels,
// the push pipeline, create / reserve / destroy) and itx_bamwin.hip (the windows of inflated bytes: carry-over, record location,
// the parse and what is handed on from it). Host side only; plain data that calloc sets up. What crosses the two files besides
// the object — bamwin_free, the allocation counters — stays inside the library (ITXI_LOCAL).
#pragma once
#include "itx_common.h"
#ifndef ITXG_FN
#define ITXG_FN static __host__ __device__ inline
#endif
#include "itx_inflate_group.h"
#include "itx_pushsched.h"
static_assert(ITXP_GROUP == ITXG_SLOTS, "a group of the schedule is a group of one launch");

#include <stdio.h>
#include <stdlib.h>

#define WIN_HEAD (4u << 20)          /* room before a window's new bytes for the unconsumed tail of the previous one */
#define BAD_W(w) ((w) < 0 || (w) >= ITX_BAMWIN_WINDOWS)

// One launch covers a GROUP of up to ITXG_SLOTS pushes (itx_inflate_group.h): each slot brings its own compressed bytes, block
// list, output base and status bytes; the scratch regions and meta are indexed by the group-wide block index.
struct GroupArgs {
    itxg_index x;
    const uint32_t *comp[ITXG_SLOTS];
    const itx_bgzf_block *blk[ITXG_SLOTS];
    uint8_t *out[ITXG_SLOTS], *status[ITXG_SLOTS];
};

// pushes an inflater can hold in flight (a SLOT each: copy stream, events, compressed bytes, block list, status): ITX_PUSHES,
// 1 .. ITX_BAMWIN_LANES
static inline int lanes_in_use()
{
    static int v;
    if (!v) {
        const char *e = getenv("ITX_PUSHES");
        const int x = e ? atoi(e) : 0;
        v = x >= 1 && x <= ITX_BAMWIN_LANES ? x : ITX_BAMWIN_LANES_DEFAULT;
    }
    return v;
}
// ... and the COMPUTE lanes their kernels run on (a stream and the 88 KB of token scratch per block each): ITX_LANES, at most
// the slots. Slot s computes on lane s % n. A push used to copy and compute on one stream: a lane was busy copy + pass 1 + pass 2
// = 46 ms per push of which the kernels are 34 — on average 2.6 of 4 pass-1 kernels were running (profiles/r03_cli_500M_trace_*).
// With more slots than lanes the next push's bytes cross PCIe while the lane still computes; more LANES instead cost a gigabyte
// of scratch each and their kernels crowd the engine's out of the CUs (k_hist 0.67 -> 3.1 ms with 8).
// (Since the launches are grouped — below — one lane is the default: four pushes a launch on one stream, 2.50 s per run at the runtime's four
// hardware queues against 2.44 s with two lanes of two and 3.01 s with four lanes of one, profiles/r10_grouped_launches_parent_vs_branch.json.)
#define ITX_COMPUTE_LANES_DEFAULT 1
static inline int compute_lanes()
{
    static int v;
    if (!v) {
        const char *e = getenv("ITX_LANES");
        const int x = e ? atoi(e) : 0;
        v = x >= 1 && x <= ITX_BAMWIN_LANES ? x : ITX_COMPUTE_LANES_DEFAULT;
        if (v > lanes_in_use()) v = lanes_in_use();
    }
    return v;
}

// ... and the pushes one launch covers (ITX_GROUP, 1 .. ITXG_SLOTS). Pass 1 is a lane per block: its time is the length of a
// block's decode chain, hardly the number of blocks, until waves share a CU. Four pushes' pass 1 therefore had to overlap, on
// four streams that need a hardware queue each — and the runtime has four in all by default, shared with the copy stream, the
// parse stream and the engine. One launch over G pushes' blocks keeps as many blocks in flight from 1 / G of the streams.
#define ITX_GROUP_DEFAULT 4
static inline int group_size()
{
    static int v;
    if (!v) {
        const char *e = getenv("ITX_GROUP");
        const int x = e ? atoi(e) : 0;
        v = x >= 1 && x <= (int)ITXG_SLOTS ? x : ITX_GROUP_DEFAULT;
        if (v > lanes_in_use()) v = lanes_in_use();
    }
    return v;
}

// ... and whether a launch is FUSED (ITX_FUSE, 0 or 1): one k_decode that carries pass 1 of a group and pass 2 of the group
// before it on the lane, instead of k_tokens and k_resolve one behind the other. On one lane the pair is strictly serial — pass 2
// runs alone, 8.3 of every 36.7 ms, on a chip that pass 1's 700 waves left nearly empty a moment before — although pass 2 only
// needs the tokens of the PREVIOUS launch. With more than one compute lane the launches of different lanes overlap already: those
// keep the two kernels (ITX_LANES > 1 switches the fusion off).
#define ITX_FUSE_DEFAULT 1
static inline bool fuse_on()
{
    static int v = -1;
    if (v < 0) {
#ifndef ITXI_SYM16
        const char *e = getenv("ITX_FUSE");
        v = ((e && *e) ? atoi(e) != 0 : ITX_FUSE_DEFAULT != 0) && compute_lanes() == 1;
#else
        v = 0;
#endif
    }
    return v != 0;
}

// a push in flight: its compressed bytes, block list and status, so that the Huffman pass of one chunk runs beside the replay of the last
struct itxi_slot {
    hipEvent_t copied;                 // the compressed bytes have left the caller's buffer
    int copy_live;                     // a copy of this slot was recorded and not yet ended: written by the producer (push_begin behind the
                                       // record, push_end), read by the reader's io thread (push_copied) — release / acquire, nothing else of
                                       // the slot is read there
    uint8_t *win_buf;                  // where its blocks' bytes go: the window's buffer
    uint8_t *d_comp, *d_status, *h_status;
    itx_bgzf_block *d_blk, *h_blk;     // h_blk (page-locked): the block list shifted to the window's offsets
    size_t comp_cap, status_cap, blk_cap, h_cap;
    size_t n_blk, total;
};
// what a group of the schedule (itx_pushsched.h) owns on the device side
struct itxi_group {
    bool timed;
    hipEvent_t ev[3];                  // ITX_TIMING: before pass 1, between the passes, after pass 2 (fused: before and after the
                                       // launch that carries its pass 1)
    hipEvent_t done;                   // both passes and the status copies of every member through
};
// a compute lane: the stream the two passes of its groups run on, one group after the other, and their scratch
struct itxi_lane {
    hipStream_t cst;                   // (created when the first group is launched on it)
    uint8_t *d_lit[2];                 // fused launches: the lane's q-th group writes buffer q & 1, the launch after it reads it
    uint32_t *d_meta[2];               // (the two-kernel path uses buffer 0 alone)
    size_t lit_cap[2], meta_cap[2];
    uint32_t pend_span;                // fused: the span and arguments of the schedule's pending group
    GroupArgs pend_args;
};

struct itx_inflater {
    int device;
    hipStream_t st[2];                     // st[1]: carry-over, locate and parse of every window; st[0]: itx_inflate_bgzf's calls alone
    // the decoder (itx_inflate.hip)
    struct {
        int n_cu;
        uint8_t *d_comp, *d_out, *d_status, *d_lit;      // the stand-alone path (itx_inflate_bgzf). d_lit: the blocks' scratch regions
        uint32_t *d_meta;
        itx_bgzf_block *d_blk;
        size_t comp_cap, out_cap, status_cap, blk_cap, lit_cap, meta_cap;
        hipEvent_t ev[4];
        float ms_tokens, ms_resolve, ms_resolve_all;
        hipEvent_t ev_res_end[2];
        hipStream_t copy_st;               // every push's bytes cross PCIe on it, in push order
        itxp_sched sched;                  // which push is in which group, what is launched, resolved, pending: itx_pushsched.h
        itxi_slot lane[ITX_BAMWIN_LANES];
        itxi_group grp[ITX_BAMWIN_LANES];
        itxi_lane clane[ITX_BAMWIN_LANES];
    } dec;
    // windows of inflated bytes that stay on the device (itx_bamwin_*)
    struct {
        struct {
            uint8_t *buf;
            size_t cap;
            uint32_t start, len, consumed;     // unconsumed bytes are buf[start, len); consumed: end of the last parsed record
        } win[ITX_BAMWIN_WINDOWS];
        uint8_t *arena;                    // itx_inflater_reserve: the one allocation the lanes' and the first n_reserved_win windows' buffers are cut from
        int n_reserved_win;
    } wins;
    // the last parsed window's records (itx_bamwin.hip)
    struct {
        void *d_sum, *h_sum;               // PieceSum per piece, and its host copy
        uint32_t *d_spec, *d_pb, *h_pb, *d_recoff, *d_flags;
        uint8_t *d_seen;
        size_t seen_cap;
        size_t sum_cap, spec_cap, pb_cap, recoff_cap, soa_cap;
        int32_t *d_tid, *d_pos, *d_end, *d_mpos, *d_isize;
        uint8_t *d_mapq, *d_f5, *d_xa;
        int parsed_w;
        size_t n_rec;
    } parse;
};

#define ITXI_LOCAL __attribute__((visibility("hidden")))        /* shared by the library's files, no symbol of the library */
ITXI_LOCAL void bamwin_free(itx_inflater *h);         // itx_bamwin.hip: the parse buffers, for itx_inflater_destroy

// ITX_TIMING: device allocations made while the pipeline runs, and the time they took (itx_inflate.hip reports them)
ITXI_LOCAL extern double g_alloc_s;
ITXI_LOCAL extern unsigned long g_allocs;

template <typename T> static int grow(T **p, size_t *cap, size_t need, bool exact = false)
{
    if (need <= *cap) return ITX_OK;
    const double t_alloc0 = itx_wall_now();
    struct Acc {
        double t0;
        ~Acc()
        {
            g_alloc_s += itx_wall_now() - t0;
            g_allocs++;
        }
    } acc{t_alloc0};
    if (*p) ITX_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    const size_t want = exact ? need : need + need / 4;
    const double tm0 = itx_wall_now();
    ITX_HIP(hipMalloc((void **)p, want * sizeof(T)));
    if (getenv("ITX_TIMING_ALLOC")) fprintf(stderr, "[itx alloc] hipMalloc %.1f MB: %.2f ms\n", (double)(want * sizeof(T)) / 1e6, 1e3 * (itx_wall_now() - tm0));
    *cap = want;
    return ITX_OK;
}
