// itx_bamout_priv.h — internal: what the files of the BAM writer of `filter -b` share. itx_bamout.hip has the object and the
// batch path (and says what a batch goes through), itx_bamout_members.hip makes a stream's payloads BGZF members (-l),
// itx_bamout_sort.hip holds, sorts and replays the stream (-s), itx_bamout_annotate.hip takes the table for the tags (-a),
// itx_bamout_mates.hip holds the candidates and joins the mates of the counted pairs to the held stream (-m).
// itx_bamwin.hip includes this file for itx_bamout_start alone.
// One object, one kernel stream: every step below runs on bo->st, and "bo->st is idle" means the caller has waited for it.
#pragma once
#include "itx_bamidx.h"
#include "itx_deflate_device.h"
#include "itx_bgzfmember.h"
#include "itx_reptag.h"

typedef unsigned long long ull;

#define BO_TILE 256u                 // records per workgroup (measure, gather)
#define BO_LDS 32768u                // bytes staged at a time: a tile of short reads (256 x ~120 bytes) in one window
#define BO_P ITX_BAMOUT_PAYLOAD
#define BO_STRIDE ITX_BGZF_MEMBER_CAP(BO_P)      // bytes between two members' slots (a multiple of 4)
#define BO_MAX_RECORD 0x40000000u    // a record of a gibibyte is nobody's: the decoder's windows hold less
#define BO_TOT_BYTES 64u             // a batch's totals: bytes, records, records too long; -a: rows outside the table, tag bytes

static_assert(BO_P % 16u == 0 && BO_P <= ITXD_MAX_IN, "the payload: at most one DEFLATE window, whole 16-byte vectors");
static_assert(BO_TILE == ITX_BAMIDX_TILE && BO_P == ITX_BAMIDX_PAYLOAD, "the index (itx_bamidx.hip) places records by the gather's tiles and payloads");

// ---- filter -b -a: the table's rows and names as the kernels read them (one allocation, itx_bamout_annotate_enable)
struct BoAnn {
    const uint32_t *rows;            // per row: start, end, rep, cla, fam
    const ull *rep_off, *cla_off, *fam_off;
    const uint8_t *rep, *cla, *fam;  // the name pools: name i of a pool is bytes [off[i], off[i + 1])
    uint32_t n_rows;
};
#define BO_ROW_WORDS 5u

__device__ __forceinline__ ItxRepTag bo_row_tag(const BoAnn &a, uint32_t row)
{
    const uint32_t *r = a.rows + (size_t)BO_ROW_WORDS * row;
    ItxRepTag t;
    t.start = r[0];
    t.end = r[1];
    const ull r0 = a.rep_off[r[2]], c0 = a.cla_off[r[3]], f0 = a.fam_off[r[4]];
    t.rep = a.rep + r0;
    t.rep_len = (uint32_t)(a.rep_off[r[2] + 1u] - r0);
    t.cla = a.cla + c0;
    t.cla_len = (uint32_t)(a.cla_off[r[3] + 1u] - c0);
    t.fam = a.fam + f0;
    t.fam_len = (uint32_t)(a.fam_off[r[4] + 1u] - f0);
    return t;
}

// ---- filter -b -s: what is collected during the pass and the order of the replay
struct BoSortEnt {
    uint32_t tid, low;               // the high and the low sort key (itx_bamsortrule.h)
    ull off;                         // the record's first byte in the held stream
    uint32_t len, pad;               // 4 + block_size; pad: in mates mode the row the record was counted for (BO_NO_ROW: none given)
};
#define BO_NO_ROW 0xffffffffu
static_assert(sizeof(BoSortEnt) == 24, "BoSortEnt");

struct bo_slot {                     // one batch's members on their way out
    uint8_t *d_packed, *h_pin;
    size_t cap;                      // bytes of both
    ull *h_total;                    // page-locked: the packed size
    hipEvent_t e0, e1;               // around member + scan + pack; e1 is the batch's "done"
    uint32_t n_mem;
    int busy;
};

struct itx_bamout {
    int device;
    size_t cap;                      // records per batch
    hipStream_t st, cst;             // kernels; the copies to the host
    hipEvent_t ev[5];                // measure: 0 .. 1, gather: 2 .. 3 (3: the batch's records are read); 4: the caller's stream
    int gather_timed;
    int32_t *d_hits;
    uint32_t *d_len;
    ull *d_tile_sum, *d_tile_base, *d_tot, *h_tot;
    uint8_t *d_pay;                  // the payload stream: carry bytes, then the batch's
    size_t pay_cap, carry;
    uint8_t *d_mem;                  // member slots of BO_STRIDE bytes
    uint32_t *d_msize;
    uint64_t *d_moff;
    size_t mem_cap;                  // members
    bo_slot slot[2];
    int head, pending;               // the oldest batch not yet collected; batches not yet collected
    int finished;
    int level, level_set;            // the members' level (itx_bgzflevels.h): 6 unless itx_bamout_set_level chose another
    itx_bamout_stats stats;
    int annotate;                    // filter -b -a (itx_bamout_annotate_enable): d_ann holds the rows and names, ann points into it
    void *d_ann;
    BoAnn ann;
    ull tag_bytes;                   // tag bytes the device batches appended
    itx_bamidx *ix;                  // filter -b -i (itx_bamout_index_enable): the .bai index in the making, else null
    ull stream_base;                 // bytes of the record stream that are members already: d_pay[0] is this byte of the stream
    // filter -b -s (itx_bamout_sort_enable)
    int sort;                        // 0: off; 1: the stream is held (d_pay is the held stream, carry its bytes); 2: it is replayed
    int32_t n_ref;                   // from index_enable, else -1: the highest tid seen says how many passes tid takes
    BoSortEnt *d_sent;               // the pool: an entry per held record, in stream order
    ull n_sent, sent_cap, sent_grows;
    uint32_t *d_sflag, *h_sflag;     // [0] records that cannot be sorted, [1] the highest tid (device batches; h_sflag page-locked)
    ull host_bad;                    // the same of the host route's records
    uint32_t host_maxtid;
    uint8_t *d_held;                 // the replay: the held stream, the pairs in both buffers and where the sorted ones are,
    uint2 *d_k0, *d_k1, *sorted;     // the digit counts, the round's offsets into the held stream
    uint32_t *d_hist;
    ull *d_soff;
    ull sort_done, rounds;           // records replayed; rounds
    hipEvent_t sev[2];               // around the sort
    int sort_timed;
    double sort_ms, replay_ms;
    // filter -b -s -m (itx_bamout_mates_enable, itx_bamout_mates.hip)
    int mates;                       // 0: off; 1: candidates are collected; 2: the join is done and the candidate store gone
    uint32_t *d_mlen;                // the candidate pass's own lengths, tile sums, tile bases and totals (the counted pass's are
    ull *d_mtile_sum, *d_mtile_base, *d_mtot, *h_mtot;   // read by the host's totals step and by k_bs_entries); h_mtot page-locked
    ull *d_moff64;                   // the join's rounds: where a round's candidates lie in the candidate stream, and their rows
    int32_t *d_mrow;
    uint8_t *d_cand;                 // the candidate stream: the candidates' bytes one behind the other, in stream order
    size_t cand_cap, cand_len;
    struct BmCand *d_cent;           // the candidate pool: an entry per candidate, in stream order
    ull n_cent, cent_cap;
    uint32_t cand_maxtid;            // the highest tid among the candidates: it counts the tid passes as n_ref does
    int32_t *host_rows;              // itx_bamout_mates_host_rows: the rows of the next append_host's records (malloc)
    size_t n_host_rows;
    hipEvent_t mev[2];               // around a batch's candidate gather and entries (mev[1]: the window has been read), and the join
    int mates_timed;
    itx_bamout_mates_stats mstats;
};

// ---- the steps the files call across. All are the writer's own: nothing outside it calls them, but for itx_bamout_start.

// itx_bamout.hip. A batch of device records: measure + scan (waited for: the totals size every buffer), then gather, members and
// pack are enqueued. Called by itx_bamout_run and by itx_bamwin_bamout (itx_bamwin.hip), while the stream is collected: refused
// once it is finished or being replayed (sort == 2).
int itx_bamout_start(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, const int32_t *d_hit_row, size_t n, void *stream);

// itx_bamout.hip. The enable calls (set_level, annotate_enable, sort_enable, index_enable) before they change anything: ITX_OK
// while nothing has entered the stream and `already` is 0, else ITX_E_STATE with "<fn>: called twice" (already != 0) or
// "<fn>: the stream has begun".
int bo_not_begun(const itx_bamout *bo, const char *fn, int already);

// itx_bamout.hip. Room for a stream of `total` bytes and for the n_mem members made of it next; bo->st is idle. Every limit is
// checked and every buffer allocated here, before anything is written: what does not fit leaves the object as it was.
// Called in front of every bo_emit: by start, append_host and finish, and by sort_next for a round of the replay.
int bo_reserve(itx_bamout *bo, ull total, ull n_mem);

// itx_bamout.hip. The scan of nt tiles' sums in d_tile_sum (k_tile_scan2) and the wait for its totals: ev[1] is recorded behind
// the scan, tot_bytes of d_tot are copied to h_tot, the stream is waited for (wait_ms counts it), the gather before is timed
// (bo_read_gather_time), and ev[0] .. ev[1] is added to *acc_ms. The caller has recorded ev[0] and enqueued what fills
// d_tile_sum: start (any state but finished or sort == 2) and sort_next (sort == 2).
int bo_totals(itx_bamout *bo, uint32_t nt, size_t tot_bytes, double *acc_ms);

// itx_bamout.hip. k_bo_gather enqueued over n records of lengths d_len, behind bo->carry bytes of d_pay; bo_totals has filled
// d_tile_base and bo_reserve has made room. While the stream is collected (start) rec_off are uint32_t offsets into u and, under
// -a, hit_row chooses the tags laid behind a record; during the replay (sort_next, sort == 2) rec_off are 64-bit offsets into the
// held stream u and hit_row is not read.
int bo_launch_gather(itx_bamout *bo, const uint8_t *u, const void *rec_off, uint32_t n, const int32_t *hit_row);

// itx_bamout.hip. The same kernel with every array named: n records at rec_off (wide: 64-bit offsets, else uint32_t) of u, of
// lengths len_in, laid behind `base` bytes of pay by the tile bases of a scan over those lengths; ann: len_in are annotated lengths
// and hit_row chooses each record's tags. bo_launch_gather is this over the counted pass's arrays; the mates' passes
// (itx_bamout_mates.hip) gather a window's candidates into the candidate stream and the chosen ones behind the held stream.
int bo_launch_gather_at(itx_bamout *bo, int wide, int ann, const uint8_t *u, const void *rec_off, uint32_t n, const uint32_t *len_in, const ull *tile_base, ull base,
                        uint8_t *pay, const int32_t *hit_row);

// itx_bamout.hip. The device time of the last gather (and of the index's entry kernels) is read and added to gather_ms, or to
// replay_ms during the replay; ev[3] is through, which every caller has waited for. Nothing happens when it was read already.
void bo_read_gather_time(itx_bamout *bo);

// itx_bamout_members.hip. d_pay holds `total` bytes: its whole payloads (with_tail: and the short rest) become members in the
// next slot, the rest moves to the front. bo_reserve(total, that many members) has succeeded, and with an index
// itx_bamidx_reserve for as many. Called by start and append_host (sort == 0), finish (with_tail) and sort_next (sort == 2).
int bo_emit(itx_bamout *bo, ull total, int with_tail);

// itx_bamout_sort.hip. filter -b -s: room for n_more more entries in the pool; bo->st is idle. What does not fit leaves the
// object as it was. Called by start and append_host while the stream is held (sort == 1).
int bs_reserve(itx_bamout *bo, ull n_more);

// itx_bamout_sort.hip. k_bs_entries enqueued behind a batch's gather (the kernel lives with the sort, start launches it through
// here): one entry per counted record of the batch, n_counted of them, behind those of the pool; bs_reserve(n_counted) has
// succeeded and bo->carry is still the held stream's length before the batch. Called by start while the stream is held (sort == 1).
// In mates mode hit_row is the batch's chosen rows and every entry keeps its record's; else it is null.
int bs_entries(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, uint32_t n, ull n_counted, const int32_t *hit_row);

// itx_bamout_mates.hip. filter -b -s -m: the candidates among a batch's n records (itx_materule.h) go behind those of the candidate
// store, bytes and entries; the host waits for their totals in between. Called by start behind the counted gather and bs_entries
// (mates == 1). On return mev[1] is behind the last kernel that reads the window (itx_bamout_wait_kernels waits for it).
int bm_batch(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, uint32_t n);

// itx_bamout_mates.hip. The join, at the first sort_next before the sort (mates == 1, sort == 1, bo->st idle): the candidates the
// held counted records want are laid behind the held stream and their entries behind the pool; the candidate store goes.
int bm_join(itx_bamout *bo);

// itx_bamout_mates.hip. Everything the mates own is freed (destroy).
void bm_destroy(itx_bamout *bo);
