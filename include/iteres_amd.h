/* iteres_amd.h — C ABI of the MI355X (gfx950) engine for iteres' one hot path:
 *
 *     BAM record -> RepeatMasker-interval overlap classification -> per-repName / repFamily /
 *     repClass read counters, per-base consensus coverage (iteres stat) and per-locus read
 *     counts (iteres filter).
 *
 * The reference (lidaof/iteres, /root/reference) has no library or FFI surface: the path is
 * two static loops inside the program. This header is therefore the seam a maintainer would cut
 * INSIDE the reference: every entry point names the reference code it stands in for (paths
 * relative to /root/reference). INTEGRATION.md shows the calls a patched generic.c / stat.c /
 * filter.c would make.
 *
 * Conventions: plain C, no global state, every function returns ITX_OK (0) or a negative ITX_E_*
 * code; itx_last_error() gives a thread-local message. One submitting thread per engine.
 * All "host" pointers are ordinary host memory; "device" pointers are HIP device memory on the
 * engine's GPU. There is no CPU fallback: every call that needs the GPU fails with
 * ITX_E_NO_DEVICE when none is usable.
 */
#ifndef ITERES_AMD_H
#define ITERES_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITX_OK 0
#define ITX_E_ARG (-1)        /* bad argument */
#define ITX_E_RANGE (-2)      /* a table row is outside its chromosome: what binKeeperAdd errAborts on (cuskent/binRange.c:176-178) */
#define ITX_E_NO_DEVICE (-3)  /* no usable gfx950 device / HIP runtime error */
#define ITX_E_NOMEM (-4)
#define ITX_E_STATE (-5)      /* call order violated (e.g. submit before set_tidmap) */
#define ITX_E_LIMIT (-6)      /* a size exceeds what the device layout encodes */

const char *itx_last_error(void);
/* ABI version of this header: major*1000 + minor. */
int itx_abi_version(void);
/* Number of visible HIP devices, or a negative ITX_E_* code. Does not create a context. */
int itx_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * The repeat table: replaces `struct hash *hashRmsk` (per-chromosome binKeeper of struct rmsk,
 * generic.h:7-15, built by rmsk2binKeeperHash generic.c:1578-1626) together with the per-row
 * links to hashRep / hashFam / hashCla entries (generic.c:1631-1693) and the repeat-size lookup
 * (generic.c:1647).
 * ------------------------------------------------------------------------------------------- */
typedef struct itx_table itx_table;

/* One rmsk.txt row as generic.c:1594-1607 parses it. `chrom` indexes chrom_size[]; rep/fam/cla
 * are dense ids of the row's OWN repName / repFamily / repClass strings (repName -> family is
 * not functional in rmsk, so the ids come from the row). Rows are given in FILE order: the
 * order decides ties exactly as binKeeper's insertion order does (cuskent/binRange.c:185,209-225). */
typedef struct itx_row {
    int32_t  chrom;
    uint32_t start, end;            /* genoStart, genoEnd                        (generic.c:1602-1603) */
    uint32_t cons_start, cons_end;  /* consensus_start / consensus_end           (generic.c:1596-1601) */
    uint32_t rep, fam, cla;
} itx_row;

/* chrom_size[c] = value from the chrom-size file; rep_len[r] = consensus length from the
 * repeat-size file or 0 (generic.c:1647). Fails with ITX_E_RANGE on a row binKeeperAdd would
 * abort on; *bad_row (optional) receives its index. device = HIP device ordinal. */
int itx_table_create(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom,
                     const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla,
                     int device, itx_table **out, size_t *bad_row);
void itx_table_destroy(itx_table *t);

typedef struct itx_table_info {
    uint64_t n_rows, n_rep, n_fam, n_cla;
    uint64_t cov_len;      /* sum of rep_len: length of the concatenated coverage vectors          */
    uint64_t n_units;      /* distinct (repName, repFamily, repClass) triples among the rows       */
    uint64_t n_slots;      /* consensus slots the device accumulates over: sum over units of (rep_len + 1) */
    uint64_t table_bytes;  /* device bytes the table occupies                                      */
    int32_t  n_chrom, bin_shift, device, reserved;
} itx_table_info;
int itx_table_get_info(const itx_table *t, itx_table_info *out);
/* TEST ONLY: one array of a built table copied to the host, so that the device build and the host build (ITX_TABLE_HOST=1) can be
 * compared array by array. *bytes receives the array's size; dst NULL: nothing else happens; otherwise cap_bytes must hold it.
 * The layouts are internal (csrc/itx_tablebuild.h, csrc/itx_common.h) and may change with any release. */
enum { ITX_TABLE_IV = 0, ITX_TABLE_ORIG = 1, ITX_TABLE_BL = 2, ITX_TABLE_ROW_UNIT = 3, ITX_TABLE_PART_UNIT = 4, ITX_TABLE_UNIT_SLOT = 5,
       ITX_TABLE_UNIT_IDS = 6, ITX_TABLE_UNIT_COVOFF = 7, ITX_TABLE_CHROM_OFF = 8, ITX_TABLE_BIN_OFF = 9 };
int itx_table_debug_copy(const itx_table *t, int which, void *dst, size_t cap_bytes, size_t *bytes);
/* off[r] = start of repName r inside cov/cov_uniq; off[n_rep] = cov_len. */
int itx_table_cov_offsets(const itx_table *t, uint64_t *off);

/* ---------------------------------------------------------------------------------------------
 * The engine: replaces the body of the record loop, generic.c:748-1036 (stat copy) ==
 * generic.c:385-697 (filter copy): read-end / mapped / used counters, coordinate derivation,
 * binKeeperFind + best-hit rule (generic.c:945-970), and the accumulate step
 * (generic.c:983-1032). The order-dependent features around it reach the engine as one flag bit per
 * record (ITX_F5_NOLOOKUP) and have device implementations of their own further down: -R dedup
 * (generic.c:907-919, itx_dedup_*), the XA/NM veto (972-982, itx_xaveto_*), bed emission (925-936,
 * itx_bed_*), the qname lists of filter -r (662-666, itx_names_*).
 * ------------------------------------------------------------------------------------------- */
typedef struct itx_engine itx_engine;

typedef struct itx_params {
    uint32_t mapq_min;             /* -Q  unique-read MAPQ threshold           (stat.c:49)  */
    float    min_cov;              /* -c / -g coverage threshold               (stat.c:50)  */
    uint32_t extension;            /* -E  0 = none                             (stat.c:61)  */
    uint32_t isize_max;            /* -I                                       (stat.c:62)  */
    int32_t  treat_pe_as_se;       /* -T                                       (stat.c:55)  */
    int32_t  discard_half_mapped;  /* -D                                       (stat.c:56)  */
    int32_t  mode;                 /* ITX_MODE_STAT: counters + coverage; ITX_MODE_FILTER: per-locus counts */
    int32_t  accum;                /* ITX_ACCUM_*: how the device accumulates (same results)            */
} itx_params;
#define ITX_MODE_STAT 0
#define ITX_MODE_FILTER 1
#define ITX_ACCUM_DEFAULT 0
#define ITX_ACCUM_ATOMIC 1        /* global atomics straight from the classify kernel                  */
#define ITX_ACCUM_PARTITION 2     /* key emit -> radix partition -> LDS histograms (no scattered atomics) */

/* Record batch, structure of arrays. One element per BAM record, in file order:
 *   tid, pos            bam1_core_t.tid / .pos                       (cussamtools/bam.h:169-177)
 *   tmpend              n_cigar ? bam_calend(core, cigar) : pos + l_qseq          (generic.c:820)
 *   mapq                bam1_core_t.qual
 *   flag5               bit0 PAIRED(0x1) bit1 UNMAP(0x4) bit2 MUNMAP(0x8) bit3 REVERSE(0x10) bit4 READ1(0x40);
 *                       bit5 ITX_F5_NOLOOKUP, set by the caller: the record is counted like any other up to
 *                       reads_mapped / reads_mapped_unique (cnt[0..7], cnt[11]) but is not looked up — how a caller
 *                       applies the reference's two `continue`s that sit between those counters and the
 *                       accumulation: -R duplicates (generic.c:907-919) and the XA veto (generic.c:972-982)
 *   mpos, isize         bam1_core_t.mpos / .isize; both may be NULL when no record of the batch
 *                       has PAIRED set (then they are never read). */
typedef struct itx_batch {
    const int32_t *tid, *pos, *tmpend;
    const uint8_t *mapq, *flag5;
    const int32_t *mpos, *isize;
} itx_batch;
#define ITX_F5_NOLOOKUP 0x20
#define ITX_FLAG5(bamflag) ((uint8_t)((((bamflag) & 0x1) ? 1 : 0) | (((bamflag) & 0x4) ? 2 : 0) | (((bamflag) & 0x8) ? 4 : 0) | \
                                      (((bamflag) & 0x10) ? 8 : 0) | (((bamflag) & 0x40) ? 16 : 0)))

/* batch_capacity = largest n a single submit may carry. */
int itx_engine_create(const itx_table *t, const itx_params *p, size_t batch_capacity, itx_engine **out);
void itx_engine_destroy(itx_engine *e);

/* tid2chrom[tid] for the BAM header in use: index into chrom_size[], or -1 when the (possibly
 * -C renamed) reference name is not in the chrom-size file or its size is 2 (generic.c:793-801),
 * or -2 when -C drops it (generic.c:783-784). Call again when the next BAM of a list starts. */
int itx_engine_set_tidmap(itx_engine *e, const int32_t *tid2chrom, int n_tid);

/* Pinned double buffers (2 slots): the host decoder fills slot s while slot 1-s is in flight. */
typedef struct itx_staging {
    int32_t *tid, *pos, *tmpend;
    uint8_t *mapq, *flag5;
    int32_t *mpos, *isize;
    int32_t *hit_row;              /* filled by the device when submit_slot(want_hits != 0) */
    size_t capacity;
} itx_staging;
int itx_engine_staging(itx_engine *e, int slot, itx_staging *out);
/* Asynchronous: H2D copies + kernels on the slot's stream. has_paired = 0 promises that no record
 * has PAIRED set (mpos/isize are then not copied). want_hits: write back per record the index of
 * the chosen table row (as passed to itx_table_create) or -1 into staging.hit_row. */
int itx_engine_submit_slot(itx_engine *e, int slot, size_t n, int has_paired, int want_hits);
/* Same copies, classification only: nothing is accumulated, staging.hit_row receives the chosen rows. For
 * callers that must look at the chosen row before the record counts (the XA veto): classify, wait, set
 * ITX_F5_NOLOOKUP on the vetoed records, then submit the slot. */
int itx_engine_classify_slot(itx_engine *e, int slot, size_t n, int has_paired);
int itx_engine_wait_slot(itx_engine *e, int slot);

/* Same work on a batch that is ALREADY in device memory (pointers in `b` are device pointers, each
 * 16-byte aligned), enqueued on `stream` (a hipStream_t, NULL = the null stream). d_hit_row: optional
 * device int32[n] (16-byte aligned) for the chosen rows. Returns after enqueueing. Submissions of one
 * engine must be stream-ordered with respect to each other. */
int itx_engine_submit_device(itx_engine *e, const itx_batch *b, size_t n, int32_t *d_hit_row, void *stream);
/* The same on the engine's own compute stream (the one the slot submits run on: device batches and slot batches of one
 * record stream stay ordered). itx_engine_wait_own returns when everything submitted there is through — the arrays of
 * `b` may then be reused — without waiting for other work on the device. */
int itx_engine_submit_device_own(itx_engine *e, const itx_batch *b, size_t n, int32_t *d_hit_row);
int itx_engine_wait_own(itx_engine *e);
/* Classification only (no accumulation): cuskent/binRange.c:196-227 + generic.c:950-970 per record. */
int itx_engine_classify_device(itx_engine *e, const itx_batch *b, size_t n, int32_t *d_hit_row, void *stream);
/* The lookup alone, on plain intervals: for record i the FIRST row binKeeperFind(chrom of tid[i], pos[i], tmpend[i])
 * would return (cuskent/binRange.c:196-227, clipping included) — what cpgBedGraphOverlapRepeat takes for a CpG site
 * (generic.c:1082-1088) — or -1. mapq / flag5 are not looked at (the arrays must exist); no filter, no best-hit rule,
 * no -c, nothing is accumulated. Chosen rows come back like with classify (slot: staging.hit_row). */
int itx_engine_first_hit_slot(itx_engine *e, int slot, size_t n);
int itx_engine_first_hit_device(itx_engine *e, const itx_batch *b, size_t n, int32_t *d_hit_row, void *stream);
int itx_engine_sync(itx_engine *e);
/* Zero every accumulator. */
int itx_engine_reset(itx_engine *e);

/* What the loop leaves behind for the writers (generic.c:53-113, 1709-1746). Any pointer may be
 * NULL. cnt[13] as generic.c:1048-1060 (cnt[8] and cnt[12] stay 0 here: -R and the XA veto are
 * the caller's); rep/fam/cla_cnt: [0,n) all reads, [n,2n) reads with MAPQ >= mapq_min;
 * cov/cov_uniq: bp_total / bp_total_unique of every repName, concatenated per
 * itx_table_cov_offsets; locus_cnt[row]: slCount(ss->sl) per table row (filter mode). */
typedef struct itx_result {
    uint64_t *cnt;
    uint64_t *rep_cnt, *fam_cnt, *cla_cnt;
    uint32_t *cov, *cov_uniq;
    uint32_t *locus_cnt;
} itx_result;
/* Drains all streams, turns the raw accumulators into the result arrays on the device and copies
 * them to the host pointers of `out`. The raw accumulators are left untouched, so more batches may
 * follow and finish may be called again. */
int itx_engine_finish(itx_engine *e, const itx_result *out);

/* Multi-GPU: every output is a commutative integer sum over records, so ranks process disjoint
 * parts of the stream against replicated tables and exchange ONE compact partial at the end:
 *   itx_engine_partial_size   -> element counts of the partial: n_u64 x uint64 and n_u32 x uint32
 *   itx_engine_export_partial -> writes this engine's partial into caller-owned DEVICE buffers
 *                                (what the driver all-reduces with RCCL, sum, over xGMI)
 *   itx_engine_finish_partial -> like itx_engine_finish, but from (reduced) partial buffers
 * The partial is [cnt[16] | per-unit read counts] as u64 and [coverage difference arrays] (stat) or
 * [per-locus counts] (filter) as u32; sums are mod 2^64 / 2^32 like the reference's counters. */
int itx_engine_partial_size(const itx_engine *e, uint64_t *n_u64, uint64_t *n_u32);
int itx_engine_export_partial(itx_engine *e, void *d_u64, void *d_u32, void *stream);
int itx_engine_finish_partial(itx_engine *e, const void *d_u64, const void *d_u32, const itx_result *out);
/* The engine's own pair of partial buffers (device memory of the sizes above, owned by the engine): for a caller without
 * a device allocator of its own — export into them, reduce them across ranks (itx_comm_reduce_sum), finish from them. */
int itx_engine_partial_buffers(itx_engine *e, void **d_u64, void **d_u32);

/* The exchange itself, for a host that runs one process per GPU (iteres_amd/host: `iteres stat|filter` with ITX_GPUS /
 * ITX_RANK + ITX_WORLD): replaces nothing in the reference, which has one thread and one set of counters
 * (generic.c:705-722) — it is what makes N replicas of that loop one job. itx_comm_create: rank 0 publishes the
 * communicator id as the file `id_path`, the others wait for it. itx_comm_reduce_sum: sum over ranks of the two device
 * buffers of a partial (and of a small host vector `meta`, n_meta <= 64: the host's own counters) onto rank 0, in place,
 * behind `stream`'s work; returns when the result is there (other ranks: when their part is handed over).
 *   ITX_COMM_RCCL  ncclReduce over xGMI (librccl is loaded on first use)
 *   ITX_COMM_FILE  through files next to id_path, added on the host — for ranks that share a device (rehearsals on a
 *                  one-GPU box: RCCL refuses two ranks on one GPU)
 * Waiting is bounded (ITX_COMM_TIMEOUT seconds, default 900). */
typedef struct itx_comm itx_comm;
#define ITX_COMM_RCCL 0
#define ITX_COMM_FILE 1
int itx_comm_create(int rank, int world, int device, const char *id_path, int mode, itx_comm **out);
void itx_comm_destroy(itx_comm *c);
int itx_comm_reduce_sum(itx_comm *c, void *d_u64, size_t n64, void *d_u32, size_t n32, uint64_t *meta, size_t n_meta, void *stream);

/* Device time spent in the engine's kernels since the last reset, from HIP events recorded on the
 * submitting stream around each submit_device/submit_slot (milliseconds), and the number of
 * records classified. */
typedef struct itx_stats {
    double kernel_ms;             /* all kernels of all submits                                        */
    uint64_t records, hits;
    double stage_ms[5];           /* partition path, summed over submits: [0] stream (derive + classify + */
                                  /* key emit + partition count), [1] plan, [2] scatter, [3] hist, [4] 0  */
                                  /* — HIP events recorded between the launches on the submitting stream  */
    uint64_t submits, keys;       /* number of submits; keys emitted (partition path)                   */
} itx_stats;
int itx_engine_get_stats(itx_engine *e, itx_stats *out);

/* ---- BGZF inflate on the device --------------------------------------------------------------------------------
 * Replaces the reference's per-block zlib inflate (cussamtools/bgzf.c:367-397 inflate_block, reached from
 * bgzf_read -> bgzf_read_block, bgzf.c:425-521). The caller indexes the blocks of a chunk of the file (header
 * check bgzf.c:401-411, BSIZE, ISIZE trailer) and hands over the compressed chunk; every block is decoded by one
 * wavefront into its place in `out`. Offsets are relative to `comp` / `out`; uoff must be the running sum of the
 * usize's (the inflated bytes are contiguous). `comp` needs 16 readable bytes past comp_len. status[i] = 0 when block
 * i inflated to exactly usize bytes, else a small positive code (the data is damaged or the decoder declined it —
 * the caller's zlib has the last word, as in the reference). Synchronous; one calling thread per inflater. */
typedef struct itx_inflater itx_inflater;
#define ITX_BAMWIN_LANES 12       /* pushes that may be in flight at once (push_begin's s); ITX_PUSHES (environment) says how many an inflater sets up */
#define ITX_BAMWIN_LANES_DEFAULT 12 /* their kernels run in groups of ITX_GROUP (default 4) pushes a launch on ITX_LANES (default 1) compute lanes. A launch
                                   * covers pass 1 of its group and pass 2 of the group before it on the lane (ITX_FUSE=0: both passes of its own group, two
                                   * kernels): three groups are alive at once, one whose bytes cross PCIe, one in pass 1, one waiting for pass 2. With
                                   * itx_inflater_reserve the 12 slots, two scratch buffers and 16 windows of the command's 384 MB chunks are 26 597 153 792 bytes of HBM, 17.3 GB before */
#define ITX_BAMWIN_WINDOWS 48     /* windows of inflated bytes (w): the decode may run this far ahead of the consumer (a window's
                                   * buffer is allocated when it is first pushed into: 288 GB of HBM is room for a long lead) */
typedef struct itx_bgzf_block {
    uint32_t coff, csize;         /* the whole gzip member: 18-byte header, deflate data, CRC32, ISIZE */
    uint32_t uoff, usize;
} itx_bgzf_block;
int itx_inflater_create(int device, itx_inflater **out);
void itx_inflater_destroy(itx_inflater *h);
int itx_inflate_bgzf(itx_inflater *h, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk, void *out, size_t out_len,
                     uint8_t *status);
/* Device time of the two passes of the last call (Huffman -> tokens; first group of tokens -> bytes), milliseconds. */
int itx_inflater_last_ms(const itx_inflater *h, float *tokens_ms, float *resolve_ms);
/* ... and of pass 2 over ALL groups of that call; kernels only when the call was given out == NULL (the inflated bytes then
 * stay on the device: timing runs) */
int itx_inflater_last_resolve_all_ms(const itx_inflater *h, float *ms);

/* ---- BAM records located and parsed on the device ---------------------------------------------------------------
 * Replaces bam_read1 (cussamtools/bam.c:179-210) and the field reads of the scan loop (generic.c:745-905 off
 * bam1_core_t, bam.h:169-177; bam_calend bam.c:17-27) for whole chunks: the inflated bytes never leave the device,
 * only the per-record SoA (the itx_staging arrays) comes back. An inflater holds ITX_BAMWIN_WINDOWS WINDOWS of inflated bytes
 * (w) so that some can be filled while the records of another are still being fetched:
 *   push      inflate the blocks of a chunk into window w (offsets as for itx_inflate_bgzf; *n_new = bytes added)
 *   patch     overwrite part of what push produced (a block the caller inflated itself); truncate: drop the end
 *   carry     move the unconsumed tail of window `from` (a partial record) in front of window `to`'s fresh bytes
 *   peek/skip the unconsumed bytes from the front (the BAM header is parsed by the caller)
 *   parse     locate every complete record of window w and parse it: *n_rec records; *malformed = a record length
 *             below 32 ended the stream (bam.c:186-190); *flags bit 0: some record has PAIRED set, bit 1: some
 *             record carries an XA tag; *rewalked: pieces whose guessed start had to be corrected (may be NULL)
 *   fetch     records [first, first + n) of the last parse into dst's HOST arrays at index dst_at (hit_row untouched),
 *             optionally their byte offsets in the window and per-record XA marks
 *   bytes     raw window bytes at such offsets (read names, XA / NM strings: the caller's side channels)
 *   tids      which references (tid < n_targets) have a mapped record in the last parsed window (one byte each)
 *   device_batch  records [first, ..) of the last parse as DEVICE arrays for itx_engine_submit_device* (first % 16 == 0;
 *             valid until the next parse)
 * Records are located by guess-and-verify (csrc/itx_bamwin.hip): exact whatever the bytes look like. A record of
 * more than 4 MiB that straddles two chunks makes carry move the fresh bytes back (ITX_E_LIMIT only when the window's buffer
 * cannot hold both). One thread may push while another
 * parses / fetches the OTHER window. */
/* Before a stream of pushes, while the device is idle: every buffer the pushes will need, sized for chunks of at most
 * comp_bytes compressed bytes / max_blocks blocks / max_bytes inflated bytes, so that nothing is allocated (and, worse,
 * freed: hipFree waits for every kernel in flight) inside the pipeline — ONE device allocation for all of it. *n_windows,
 * in: the most the caller can use (< 1: no preference); out: how many windows were set up (w < *n_windows; between 4 and
 * ITX_BAMWIN_WINDOWS, by what the device has free). Optional: without it the buffers grow on demand. */
int itx_inflater_reserve(itx_inflater *h, size_t comp_bytes, size_t max_blocks, size_t max_bytes, int *n_windows);
int itx_bamwin_push(itx_inflater *h, int w, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk, uint8_t *status, size_t *n_new);
/* push in two halves, for a caller that keeps several pushes going (s < ITX_BAMWIN_LANES: each has its own stream and scratch,
 * so the latency-bound Huffman pass of one chunk runs beside the replay of the previous ones): begin enqueues and returns;
 * copied waits until `comp` may be reused; end waits for the push and delivers status / n_new. */
int itx_bamwin_push_begin(itx_inflater *h, int w, int s, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk);
int itx_bamwin_push_copied(itx_inflater *h, int s);
int itx_bamwin_push_end(itx_inflater *h, int s, uint8_t *status, size_t *n_new);
int itx_bamwin_patch(itx_inflater *h, int w, size_t uoff, const void *bytes, size_t len);
int itx_bamwin_truncate(itx_inflater *h, int w, size_t n_new);
int itx_bamwin_carry(itx_inflater *h, int from, int to);
int itx_bamwin_avail(const itx_inflater *h, int w, size_t *bytes);
int itx_bamwin_peek(itx_inflater *h, int w, size_t off, void *dst, size_t len);
int itx_bamwin_skip(itx_inflater *h, int w, size_t n);
int itx_bamwin_parse(itx_inflater *h, int w, int n_targets, size_t *n_rec, int *malformed, int *flags, size_t *rewalked);
int itx_bamwin_fetch(itx_inflater *h, size_t first, size_t n, const itx_staging *dst, size_t dst_at, uint32_t *rec_off, uint8_t *xa);
int itx_bamwin_bytes(itx_inflater *h, size_t off, void *dst, size_t len);
int itx_bamwin_tids(itx_inflater *h, uint8_t *seen, int n_targets);
int itx_bamwin_device_batch(itx_inflater *h, size_t first, int with_mates, itx_batch *out);

/* ---- the XA / NM multi-mapping veto on the device --------------------------------------------------------------------
 * Replaces mapped2diffSubfam (generic.c:303-341) and its gate (generic.c:972-982) for the records of a window the device
 * decoder has parsed: the XA:Z / NM tags are read where the inflated record lies, the alternatives with NM' <= NM are looked
 * up in the table ("any overlapping row of another subfamily name", names compared without case), and the records the
 * reference would drop get ITX_F5_NOLOOKUP in the window's flag5 array — before the window is handed to the engine.
 *   create       row_rep[n_rows]: repName id of the caller's row i; rep_word[n_rep]: equal for names that sameWord() calls
 *                equal; chrom_name[n_chrom]: the chromosome names in chrom_size[] order (hashRmsk's keys); p: the run's
 *                parameters (the record's interval is re-derived for qlen, generic.c:764-905)
 *   set_tidmap   per BAM header, as itx_engine_set_tidmap
 *   hits/stream  where itx_engine_classify_device must leave the chosen rows of the batch, and on which stream
 *   itx_bamwin_xa_veto  judges records [first, first + n) of the inflater's last parsed window (n <= batch_capacity):
 *                *n_hard > 0: some record needs the host's reading (a number strtol(.., 0, 0) reads differently from plain
 *                decimal, an alternative without four fields — where the reference asserts): NOTHING was marked, the caller
 *                takes the host route for these records; else *n_vetoed records were marked. */
typedef struct itx_xaveto itx_xaveto;
int itx_xaveto_create(const itx_table *t, const itx_params *p, const uint32_t *row_rep, const uint32_t *rep_word, const char *const *chrom_name, int n_chrom,
                      size_t batch_capacity, itx_xaveto **out);
void itx_xaveto_destroy(itx_xaveto *x);
int itx_xaveto_set_tidmap(itx_xaveto *x, const int32_t *tid2chrom, int n_tid);
int32_t *itx_xaveto_hits(itx_xaveto *x);
void *itx_xaveto_stream(itx_xaveto *x);
int itx_bamwin_xa_veto(itx_inflater *h, itx_xaveto *x, size_t first, size_t n, uint64_t *n_vetoed, uint64_t *n_hard);

/* ---- a backlog of parsed records in HBM -----------------------------------------------------------------------------
 * What a caller keeps of windows it parses BEFORE its table exists (the engine cannot take them yet): the per-record arrays
 * only — 14 B per record, 22 with mates, a ninth of the inflated bytes — so that the windows can be pushed into again and the
 * decode goes on while the rmsk file is parsed and the table built (host/stream.c: the helper thread). append copies n records
 * (device arrays) and says where they lie (a multiple of 16); batch gives that place back as an itx_batch. */
typedef struct itx_backlog itx_backlog;
int itx_backlog_create(int device, size_t max_records, itx_backlog **out);
void itx_backlog_destroy(itx_backlog *b);
size_t itx_backlog_room(const itx_backlog *b);
int itx_backlog_append(itx_backlog *b, const itx_batch *src, size_t n, size_t *at);
int itx_backlog_batch(const itx_backlog *b, size_t at, int with_mates, itx_batch *out);

/* ---- -R (remove redundant reads) on the device --------------------------------------------------------------------
 * Replaces generic.c:907-919 (filter copy 544-556): the `dup` hash of "chr:start:end:strand" keys and the `continue` behind
 * it. As a rule per record, records numbered in file order: one with MAPQ >= -Q is dropped iff an earlier one with MAPQ >= -Q
 * has the same (chromosome name, start, end, strand); one with MAPQ < -Q looks up the key of the last MAPQ >= -Q record before
 * it and is always dropped — except the very first record to reach that point of the loop when it comes before any MAPQ >= -Q
 * record (the reference's key buffer then holds no record's key: modelled as a key no record has). Dropped records get
 * ITX_F5_NOLOOKUP in their flag5 (the engine counts them up to reads_mapped(_unique) and does not look them up); the caller
 * corrects cnt[11] by *dup_unique. csrc/itx_dedup.hip: a hash table in HBM that only ever compares FULL keys (hashes pick
 * cells), grown by rehashing; at most 2^32 - 1 records per run.
 *   create     chrom_size[n_chrom] as for itx_table_create; p: mapq_min, extension, isize_max, treat_pe_as_se,
 *              discard_half_mapped; first_cells: a first size for the table (it grows)
 *   set_tidmap the BAM header in use: tid2chrom as for itx_engine_set_tidmap, tid2name[t] an id of the (renamed) reference
 *              name that is equal for equal strings over all files of the run (< 2^31)
 *   run        the next n records of the stream as DEVICE arrays (mpos / isize NULL: no record is paired), in file order,
 *              window after window; synchronous
 *   itx_bamwin_dedup   run over all records of the inflater's last parsed window */
typedef struct itx_dedup itx_dedup;
int itx_dedup_create(int device, const int64_t *chrom_size, int n_chrom, const itx_params *p, size_t first_cells, itx_dedup **out);
void itx_dedup_destroy(itx_dedup *d);
int itx_dedup_set_tidmap(itx_dedup *d, const int32_t *tid2chrom, const uint32_t *tid2name, int n_tid);
int itx_dedup_run(itx_dedup *d, const int32_t *tid, const int32_t *pos, const int32_t *tmpend, const uint8_t *mapq, uint8_t *flag5, const int32_t *mpos,
                  const int32_t *isize, size_t n);
int itx_dedup_counts(itx_dedup *d, uint64_t *dup_unique, uint64_t *dropped, uint64_t *keys);
int itx_bamwin_dedup(itx_inflater *h, itx_dedup *d);

/* ---- the bed files of stat -B / -V on the device ------------------------------------------------------------------------
 * Replaces generic.c:925-936 for the records of a window the device decoder has parsed: the text of both files is built where
 * the records lie (csrc/itx_bed.hip; the line itself: csrc/itx_bedline.h) and comes back as finished bytes, one line per
 * record that reaches the bed stage, in file order:
 *     -B  chr \t start \t end \t qname \t mapq \t strand [ \t NM \t XA ] \n        (ITX_BED_ALL; NM / XA iff the record has an XA tag)
 *     -V  chr \t start \t end \t qname \t mapq \t strand \n                        (ITX_BED_UNIQ; only records with MAPQ >= mapq_min)
 * A record with ITX_F5_NOLOOKUP set has no line (-R comes before the bed stage, generic.c:907-919), so a caller runs this AFTER
 * the -R pass and BEFORE the XA veto (generic.c:972 comes after 925).
 *   create      chrom_size[n_chrom] as for itx_table_create; p: mapq_min, extension, isize_max, treat_pe_as_se,
 *               discard_half_mapped; want: ITX_BED_ALL | ITX_BED_UNIQ; batch_capacity: the most records a batch may carry
 *   set_tidmap  per BAM header: tid2chrom as for itx_engine_set_tidmap, tid2name[t] the reference name as it is printed (after
 *               the -C rule; NULL for a reference -C drops). Not while a batch is waiting to be collected.
 *   itx_bamwin_bed  starts the build over records [first, first + n) of the inflater's last parsed window: measures the lines,
 *               waits for the sizes, enqueues the formatting and the copy to page-locked host memory, and returns. *n_hard > 0:
 *               some record needs the host's reading (a read name without a NUL inside its record): NOTHING was started, the
 *               caller takes the host route for these records. At most two batches may be started and not yet collected.
 *   run         the same over plain DEVICE arrays: the records' bytes, rec_off[i] = where record i (its block_len field)
 *               starts in them, and the per-record arrays of an itx_batch (mpos / isize NULL: no record is paired)
 *   collect     waits for the OLDEST started batch and hands out its two texts (host pointers, owned by the object, valid until
 *               the next-but-one start; a text that was not asked for has 0 bytes). Two calls instead of one so that the copy
 *               and the caller's fwrite of batch k overlap the kernels of batch k + 1.
 *   wait_kernels  returns when the kernels of every started batch are through (their copies may still run): the window's bytes
 *               and arrays may then be overwritten by the decoder
 *   get_stats   batches collected, their bytes, device time of the kernels, and how long the calls waited for the device */
typedef struct itx_bed itx_bed;
#define ITX_BED_ALL 1
#define ITX_BED_UNIQ 2
typedef struct itx_bed_text {
    const char *all, *uniq;
    uint64_t all_bytes, uniq_bytes;
} itx_bed_text;
typedef struct itx_bed_stats {
    uint64_t batches, hard_batches, bytes;
    double kernel_ms, wait_s;
} itx_bed_stats;
int itx_bed_create(int device, const int64_t *chrom_size, int n_chrom, const itx_params *p, int want, size_t batch_capacity, itx_bed **out);
void itx_bed_destroy(itx_bed *b);
int itx_bed_set_tidmap(itx_bed *b, const int32_t *tid2chrom, const char *const *tid2name, int n_tid);
int itx_bamwin_bed(itx_inflater *h, itx_bed *b, size_t first, size_t n, uint64_t *n_hard);
int itx_bed_run(itx_bed *b, const void *d_bytes, const uint32_t *d_rec_off, const itx_batch *d_batch, size_t n, uint64_t *n_hard);
int itx_bed_wait_kernels(itx_bed *b);
int itx_bed_collect(itx_bed *b, itx_bed_text *out);
int itx_bed_get_stats(const itx_bed *b, itx_bed_stats *out);

/* ---- the read lists of filter -r on the device ----------------------------------------------------------------------------
 * Replaces generic.c:662-666 (a classified record's name is head-inserted into its row's list) and the list part of
 * writeFilterOut (generic.c:1729-1731: the list reversed back to file order and joined with ','): batches leave (row, name)
 * entries in a pool in device memory, in record order; the end of the stream sorts them by row, stable, and lays the lists down
 * as one text (csrc/itx_names.hip). -R duplicates carry ITX_F5_NOLOOKUP and never choose a row; filter has no XA veto.
 *   create      batch_capacity: the most records a batch may carry; pool_bytes: a first size for the pool of name bytes
 *               (0: ITX_NAMES_POOL_BYTES from the environment, else 64 MiB). The pool and the entry list grow.
 *   hits/stream a device int32[batch_capacity] and a stream of the object's own, for itx_engine_classify_device to leave the
 *               chosen rows in (any other buffer / stream will do: `stream` below names it)
 *   itx_bamwin_names  records [first, first + n) of the inflater's last parsed window: every record with d_hit_row[i] >= 0 appends
 *               (d_hit_row[i], its name). `stream`: where d_hit_row was written (the object waits behind it). Waits for the
 *               batch's two totals, enqueues the gather, returns. *n_hard > 0: some record needs the host's reading (a read name
 *               without a NUL inside its record): NOTHING was appended, the caller takes the host route for these records.
 *   run         the same over plain DEVICE arrays: the records' bytes and rec_off[i] = where record i (its block_len field) starts
 *   wait_kernels  returns when every gather is through: the window's bytes may then be overwritten by the decoder
 *   append_host n hits the caller read itself, in stream order between the device batches: rows[i], and name i =
 *               name_bytes[name_off[i] .. name_off[i + 1]) (no NUL; name_off has n + 1 elements)
 *   finish      once: the lists of rows [0, n_rows). text: the names of a row in append order, each followed by ',' and the last
 *               by NUL, the rows one after the other; row_off[r]: where row r's list starts in text, UINT64_MAX when it has none;
 *               row_cnt[r]: its number of names. Host memory owned by the object, valid until destroy.
 * More than 2^32 - 2 names, or a pool the device cannot hold: ITX_E_NOMEM, nothing appended (ITX_HOST_NAMES=1 keeps the
 * command's lists on the host; ITX_HOST_NAMES=0 asks for this route). */
typedef struct itx_names itx_names;
typedef struct itx_names_result {
    const char *text;
    uint64_t text_bytes;
    const uint64_t *row_off;
    const uint32_t *row_cnt;
    uint64_t n_entries;
} itx_names_result;
typedef struct itx_names_stats {
    uint64_t batches, hard_batches, host_batches, entries, bytes, grows;   /* device batches appended; ...; pool reallocations */
    double gather_ms, finish_ms;                                           /* device time: measure + gather kernels; sort + text */
} itx_names_stats;
int itx_names_create(int device, size_t batch_capacity, size_t pool_bytes, itx_names **out);
void itx_names_destroy(itx_names *nm);
int32_t *itx_names_hits(itx_names *nm);
void *itx_names_stream(itx_names *nm);
int itx_bamwin_names(itx_inflater *h, itx_names *nm, size_t first, size_t n, const int32_t *d_hit_row, void *stream, uint64_t *n_hard);
int itx_names_run(itx_names *nm, const void *d_bytes, const uint32_t *d_rec_off, const int32_t *d_hit_row, size_t n, void *stream, uint64_t *n_hard);
int itx_names_wait_kernels(itx_names *nm);
int itx_names_append_host(itx_names *nm, const uint32_t *rows, const char *name_bytes, const uint64_t *name_off, size_t n);
int itx_names_finish(itx_names *nm, size_t n_rows, itx_names_result *out);
int itx_names_get_stats(const itx_names *nm, itx_names_stats *out);

/* ---- the BAM of filter -b on the device (an extension: the reference writes no such file) -------------------------------------
 * Every record that chose a row, block_size and bytes unchanged and in file order, becomes part of one stream of bytes in device
 * memory; every ITX_BAMOUT_PAYLOAD bytes of it (csrc/itx_bgzfmember.h: 8192) are made one BGZF member there, and the members
 * are handed out packed one behind the other (csrc/itx_bamout.hip; the members: csrc/itx_bamout_members.hip). The header's members
 * and the EOF marker are the caller's.
 *   create      batch_capacity: the most records a batch may carry; stream_bytes: a first size for the stream's buffer
 *               (at least four payloads are taken). Every buffer grows on demand.
 *   hits/stream as for itx_names_*
 *   itx_bamwin_bamout  records [first, first + n) of the inflater's last parsed window; `stream`: where d_hit_row was written.
 *               Waits for the batch's totals, enqueues gather, members and pack, returns.
 *   run         the same over plain DEVICE arrays: the records' bytes and rec_off[i] = where record i (its block_size field) starts
 *   wait_kernels  returns when every gather is through: the window's bytes may then be overwritten by the decoder
 *   append_host whole records (block_size field and bytes, one behind the other) the caller counted itself, in stream order
 *               between the device batches; bytes that are not whole records: ITX_E_ARG, nothing appended
 *   finish      once: what is left of the stream, less than one payload, becomes the last member (none when nothing is left)
 *   collect     the members of the oldest batch (run, append_host or finish) not yet handed out: waits for that batch's kernels,
 *               copies the packed members into one of two page-locked buffers of the object; `bytes` stays valid until the
 *               next-but-one collect. len 0: that batch completed no payload, or nothing is pending. At most two batches may
 *               wait to be collected: a third that completes a payload is refused with ITX_E_STATE, nothing appended.
 *   pending     batches that wait to be collected
 * A record of 1 GiB or more, or more than 2^31 members in a batch: ITX_E_LIMIT; no memory: ITX_E_NOMEM; both before anything
 * is written, the object stays as it was. */
typedef struct itx_bamout itx_bamout;
typedef struct itx_bamout_members {
    const void *bytes;
    uint64_t len, room;                      /* packed bytes; the size of the buffer they lie in */
    uint64_t n_members;
} itx_bamout_members;
typedef struct itx_bamout_stats {
    uint64_t batches, host_batches, records, payload_bytes, members, out_bytes, grows, carry;   /* carry: stream bytes not yet in a member */
    double gather_ms, member_ms, wait_ms;    /* device time: measure + gather; member + scan + pack. Host time spent waiting in these calls */
} itx_bamout_stats;
int itx_bamout_create(int device, size_t batch_capacity, size_t stream_bytes, itx_bamout **out);
void itx_bamout_destroy(itx_bamout *bo);
int32_t *itx_bamout_hits(itx_bamout *bo);
void *itx_bamout_stream(itx_bamout *bo);
int itx_bamwin_bamout(itx_inflater *h, itx_bamout *bo, size_t first, size_t n, const int32_t *d_hit_row, void *stream);
int itx_bamout_run(itx_bamout *bo, const void *d_bytes, const uint32_t *d_rec_off, const int32_t *d_hit_row, size_t n, void *stream);
int itx_bamout_wait_kernels(itx_bamout *bo);
int itx_bamout_append_host(itx_bamout *bo, const void *bytes, size_t len);
int itx_bamout_finish(itx_bamout *bo);
int itx_bamout_collect(itx_bamout *bo, itx_bamout_members *out);
int itx_bamout_pending(const itx_bamout *bo);
int itx_bamout_get_stats(const itx_bamout *bo, itx_bamout_stats *out);
/* The .bai index (SAM v1 section 5.2) of that BAM, built on the device in the same pass (csrc/itx_bamidx.hip; the rule a record
 * follows is csrc/itx_bairule.h). Its bytes are a function of the BAM: a run of consecutive records with one (tid, bin) is one chunk,
 * a bin's chunks stay in file order and a chunk is merged into its predecessor when prev.end >> 16 >= beg >> 16; bins ascend,
 * pseudo-bin 37450 follows them for every reference that has records; an untouched window of the linear index takes the value of
 * the nearest touched one below (0 when there is none); n_no_coor = 0 ends the file.
 *   index_enable  before the first batch (ITX_E_STATE after it, or when called twice). l_ref[0 .. n_ref): the reference lengths
 *               of the BAM's header; they size the linear index. Without this call nothing of the index exists.
 *   index_finish  after itx_bamout_finish (ITX_E_STATE before it, without index_enable, or when called twice).
 *               first_member_offset: where the first record member starts in the file (the bytes of the header's members).
 *               status ITX_BAI_OK (0): bytes / len are the file, in a page-locked buffer that lives as long as the object.
 *               Otherwise no index can be made, bytes is NULL, and status says why: 1 the records are not in coordinate order,
 *               2 a record ends beyond 2^29, 3 a record ends beyond its reference's l_ref (or names no reference),
 *               4 n_ref >= 2^16. The members are the same whether or not an index is made. */
typedef struct itx_bamout_index_result {
    const void *bytes;
    uint64_t len;
    int32_t status, pad;
    uint64_t entries, chunks, grows;         /* records indexed; chunks written (pseudo-bins apart); times the entry pool grew */
    double batch_ms, finish_ms;              /* device time: the per-batch entry kernels; everything index_finish enqueued */
} itx_bamout_index_result;
int itx_bamout_index_enable(itx_bamout *bo, int32_t n_ref, const int32_t *l_ref);
int itx_bamout_index_finish(itx_bamout *bo, uint64_t first_member_offset, itx_bamout_index_result *out);
/* The same stream in coordinate order (filter -b -s, csrc/itx_bamout_sort.hip; the order is csrc/itx_bamsortrule.h: tid, pos, reverse
 * strand, equal keys in stream order). The counted records are held in device memory until the stream ends, sorted there and replayed through the
 * member path, so the members are those a plain run over the sorted stream would make.
 *   sort_enable  before the first batch (ITX_E_STATE after it, or when called twice). From then on run / itx_bamwin_bamout /
 *               append_host make no member (nothing is pending, the two-batch limit does not apply), stats.carry counts the held
 *               bytes, and itx_bamout_finish is refused with ITX_E_STATE.
 *   sort_next   after the last batch, in place of finish, until *more is 0 (ITX_E_STATE without sort_enable, and once *more was
 *               0). The first call sorts; every call replays one round of at most batch_capacity records, which is one batch
 *               for collect: collect between the calls as between batches. The last round ends with the short last member. A
 *               counted record with tid < 0 or pos < 0: ITX_E_LIMIT before any member is made. No record: no member. After the
 *               first call run / append_host are refused with ITX_E_STATE. With index_enable the index is that of the sorted
 *               stream; index_finish follows the last round.
 * 2^32 - 2 records or more: ITX_E_LIMIT. The held stream and the sort need device memory for about twice the counted bytes:
 * ITX_E_NOMEM says to run without the sort; the object stays as it was. */
typedef struct itx_bamout_sort_stats {
    uint64_t records, rounds, pool_grows;    /* records held; rounds replayed so far; times the entry pool grew */
    double sort_ms, replay_ms;               /* device time: the radix sort; the rounds' lengths, scans and gathers */
} itx_bamout_sort_stats;
int itx_bamout_sort_enable(itx_bamout *bo);
int itx_bamout_sort_next(itx_bamout *bo, int *more);
int itx_bamout_sort_get_stats(const itx_bamout *bo, itx_bamout_sort_stats *out);
/* The level of the members (filter -b -l; csrc/itx_bamout_members.hip over csrc/itx_bgzflevels.h). Every level frames the same payloads of ITX_BAMOUT_PAYLOAD bytes,
 * so the records, the index's rule and the sort are untouched; the members' sizes, and with them every virtual offset, differ.
 *   6  the default: csrc/itx_bgzfmember.h, the only level an object has without this call
 *   0  a stored DEFLATE block per member: payload + 31 bytes
 *   1  a dynamic-Huffman block whose parse runs in slices of 128 positions on all lanes of the wave (csrc/itx_deflate_fast.h):
 *      larger members than level 6, made faster; never more than payload + 31 bytes
 *   set_level   before the first batch (ITX_E_STATE after it, or when called twice); a level other than 0, 1 or 6: ITX_E_ARG.
 *               A refused call changes nothing.
 *   get_level   the level in use (ITX_E_ARG for a null object) */
int itx_bamout_set_level(itx_bamout *bo, int level);
int itx_bamout_get_level(const itx_bamout *bo);
/* Every counted record tagged with the row it was counted for (filter -b -a, csrc/itx_bamout_annotate.hip; the rule is csrc/itx_reptag.h). Behind the record's own
 * bytes go ZN:Z:repName, ZC:Z:repClass, ZF:Z:repFamily, ZS:I:genoStart and ZE:I:genoEnd of the row in d_hit_row, 26 bytes and the
 * three names, and block_size grows by as much; nothing else of the record changes. Aux bytes the record has are not looked at: a
 * record that carries one of these tags already gets a second one behind it. The members, the index and the sort take the longer
 * records as they come; with sort_enable the records are annotated when they are first gathered and the replay copies them.
 *   annotate_enable  before the first batch (ITX_E_STATE after it, or when called twice). rows[n_rows]: start, end, rep, cla and
 *               fam are read; the name tables are in the form itx_loci_create takes (name i = bytes[off[i] .. off[i + 1]), off has
 *               n + 1 elements). Checked before anything is allocated: a null pointer, offsets that do not ascend, a row whose rep,
 *               cla or fam lies outside its table: ITX_E_ARG; a name of 2^16 bytes or more: ITX_E_LIMIT. No device memory:
 *               ITX_E_NOMEM. A refused call changes nothing. The rows and names are copied: the caller's arrays are its own again
 *               on return. From then on a batch whose d_hit_row names a row >= n_rows is refused with ITX_E_ARG, and one whose
 *               record reaches 1 GiB with its tags with ITX_E_LIMIT, nothing appended.
 *   append_host stays a taker of whole records: the caller annotates what it counted itself by the same rule (itx_reptag.h builds as C).
 *   annotate_get_stats  the tag bytes the device batches appended so far (they are part of stats.payload_bytes) */
int itx_bamout_annotate_enable(itx_bamout *bo, const itx_row *rows, size_t n_rows, const char *rep_bytes, const uint64_t *rep_off, uint32_t n_rep,
                               const char *cla_bytes, const uint64_t *cla_off, uint32_t n_cla, const char *fam_bytes, const uint64_t *fam_off, uint32_t n_fam);
int itx_bamout_annotate_get_stats(const itx_bamout *bo, uint64_t *tag_bytes);
/* The mates of the counted pairs in the sorted stream (filter -b -s -m, csrc/itx_bamout_mates.hip; the rule is csrc/itx_materule.h).
 * Without -T a proper pair is counted through its READ1 alone, so the stream holds half of every counted fragment. In mates mode every
 * record of a batch that could be such a mate (a candidate: paired, not READ1, mapped with a mapped mate, primary) is kept in a candidate
 * store in device memory beside the held stream. The first sort_next joins: a held counted record that is paired with a mapped mate
 * (wanted) looks up (mtid, mpos, name) among the candidates, the first candidate in stream order that matches byte for byte is chosen,
 * and every chosen candidate is appended once to the held stream before it is sorted; the candidate store is freed. Equal sort keys:
 * counted records first, mates behind, each in input order. With annotate_enable a mate carries the tags of the row its (earliest)
 * READ1 was counted for.
 *   mates_enable  after sort_enable, before the first batch (ITX_E_STATE without sort_enable, after the first batch, or when called twice).
 *   mates_append_host  whole records of a window the caller counted itself, all of them, in stream order between the device batches
 *               (beside append_host, which takes the counted ones): the candidates among them join the store. Bytes that are not
 *               whole records: ITX_E_ARG, nothing appended. ITX_E_STATE without mates_enable or once sort_next was called.
 *   mates_host_rows  with annotate_enable: the chosen rows of the records of the NEXT append_host, one per record (the host-route READ1s'
 *               mates need them for their tags); append_host is refused with ITX_E_STATE without them and with ITX_E_ARG when their
 *               number differs. Without annotate_enable the call is not needed.
 *   mates_get_stats  candidates held and their bytes, times the store grew, wanted and found (after the first sort_next), device time.
 * 2^32 - 2 candidates or more: ITX_E_LIMIT. The candidates of a paired file are about half its inflated bytes, held beside the -s
 * stream until the join: ITX_E_NOMEM says to run without -m. */
typedef struct itx_bamout_mates_stats {
    uint64_t candidates, candidate_bytes, grows, wanted, found;
    double gather_ms, join_ms;               /* device time: the batches' candidate measure, gather and entries; the sort, join and append */
} itx_bamout_mates_stats;
int itx_bamout_mates_enable(itx_bamout *bo);
int itx_bamout_mates_append_host(itx_bamout *bo, const void *bytes, size_t len);
int itx_bamout_mates_host_rows(itx_bamout *bo, const int32_t *rows, size_t n);
int itx_bamout_mates_get_stats(const itx_bamout *bo, itx_bamout_mates_stats *out);

/* ---- the genome coverage of filter -G on the device (an extension: the reference writes no such file) ------------------------------
 * The depth of the counted reads over the chromosomes of the size file, as two bedGraph texts: all counted reads, and those with
 * MAPQ >= mapq_min (csrc/itx_gcov.hip). A record counts when it chose a row (d_hit_row >= 0) and does not carry ITX_F5_NOLOOKUP; it
 * covers the [start, end) of csrc/itx_derive.h, the interval the lookup ran on. 0 <= start < end <= size - 1 is checked: a record
 * outside adds nothing and is counted in stats.out_of_range. Depth is u32 and wraps. Sums commute: run and add_host in any order.
 *   create      chrom_size[n_chrom] as for itx_table_create (a size <= 2 has no slots, generic.c:796-797; a size of 2^31 and above:
 *               ITX_E_LIMIT); p: mapq_min, extension, isize_max, treat_pe_as_se, discard_half_mapped. Two u32 arrays of one slot per
 *               base are allocated before anything else and zeroed: ITX_E_NOMEM when the device cannot hold them.
 *   set_tidmap  per input header, as itx_engine_set_tidmap
 *   hits/stream a device int32[batch_capacity] and a stream of the object's own, for itx_engine_classify_device to leave the chosen
 *               rows in (any other buffer / stream will do)
 *   run         n records as DEVICE arrays (mpos / isize NULL: no record is paired) and their chosen rows; enqueued on `stream`, where
 *               d_hit_row was written, and returns
 *   wait_kernels  returns when the newest run is through (each run waits for the one before): the arrays may then be overwritten
 *   add_host    n intervals the caller derived itself (the host route's counted records): chromosome (index into chrom_size), start,
 *               end, uniq != 0 for MAPQ >= mapq_min. Checked like the records of run. The arrays are the caller's again on return.
 *   finish      once (ITX_E_STATE the second time, and for run / add_host / set_tidmap after it). order[n_order]: the chromosomes in
 *               the order the files list them, each at most once (ITX_E_ARG otherwise; one that is left out is not written);
 *               chromosome c's name = name_bytes[name_off[c] .. name_off[c + 1]) (n_chrom + 1 offsets, a name below 2^16 bytes).
 *               Finds the change points of both arrays and gives the arrays back. round_bytes (0: 32 MiB, at most 1 GiB): a round
 *               of text takes max(1, round_bytes / (longest name + 34)) change points, so its text fits round_bytes or is one line.
 *               ITX_E_NOMEM / ITX_E_ARG leave the object as it was.
 *   next        the next round of file `which` (0: all counted reads, 1: MAPQ >= mapq_min): waits for it, starts the round after it
 *               into the other of two page-locked buffers, and hands it out: `bytes` (whole lines "chrom\tstart\tend\tdepth\n", one per
 *               maximal run of equal depth > 0, 0-based half open, chromosomes in finish's order, starts ascending) stays valid until
 *               the next call; more == 0: that was the last round (a file without lines: len 0, more 0). One file after the other:
 *               ITX_E_STATE for the other file while one has rounds left, and for a file that has been handed out.
 *   get_stats   records added and refused, change points, lines, bytes and rounds per file, device time of the add kernels, of the
 *               two dense passes and of the text kernels, time the host waited in these calls, and what create's allocation and
 *               zeroing cost; and what itx_gcov_bigwig_build (below) made of each file: items, sections, levels, summaries, device time */
typedef struct itx_gcov itx_gcov;
typedef struct itx_gcov_text {
    const char *bytes;
    uint64_t len;
    int32_t more, pad;
} itx_gcov_text;
typedef struct itx_gcov_stats {
    uint64_t batches, host_batches, records, out_of_range, records_uniq;
    uint64_t points[2], lines[2], bytes[2], rounds[2];
    uint64_t slots, device_bytes;              /* bases with a slot; bytes of the two arrays */
    double add_ms, points_ms, text_ms, zero_ms, wait_s, alloc_s;
    uint64_t bw_items[2], bw_sections[2], bw_levels[2], bw_summaries[2];   /* itx_gcov_bigwig_build, per file */
    double bw_ms;                              /* device time of those builds */
} itx_gcov_stats;
int itx_gcov_create(int device, const int64_t *chrom_size, int n_chrom, const itx_params *p, size_t batch_capacity, itx_gcov **out);
void itx_gcov_destroy(itx_gcov *g);
int itx_gcov_set_tidmap(itx_gcov *g, const int32_t *tid2chrom, int n_tid);
int32_t *itx_gcov_hits(itx_gcov *g);
void *itx_gcov_stream(itx_gcov *g);
int itx_gcov_run(itx_gcov *g, const itx_batch *d_batch, const int32_t *d_hit_row, size_t n, void *stream);
int itx_gcov_wait_kernels(itx_gcov *g);
int itx_gcov_add_host(itx_gcov *g, const int32_t *chrom, const uint32_t *start, const uint32_t *end, const uint8_t *uniq, size_t n);
int itx_gcov_finish(itx_gcov *g, const uint32_t *order, int n_order, const char *name_bytes, const uint64_t *name_off, size_t round_bytes);
int itx_gcov_next(itx_gcov *g, int which, itx_gcov_text *out);
int itx_gcov_get_stats(itx_gcov *g, itx_gcov_stats *out);

/* ---- the .loci file of filter / cpgfilter on the device ----------------------------------------------------------------------
 * Replaces the row walk and the fprintf of writeFilterOut (generic.c:1709-1746) and writeFilterOutMRE (generic.c:1748-1772): the
 * order of the lines is a function of the table alone — hashRmsk's chromosomes in hash order, a chromosome's rows by bin
 * ascending, newest insertion first (cuskent/binRange.c:365-392) — so it is sorted when the table is known, beside the scan of
 * the alignments; the lines are formatted where the sorted table lies and come back as one text (csrc/itx_loci.hip, the line
 * rule: csrc/itx_lociline.h).
 *   create      kind: ITX_LOCI_FILTER / ITX_LOCI_CPG. rows[n_rows] in file order with row_chrom[i] = row i's index into the
 *               chromosome names (itx_row.chrom is not read); chrom_rank[c] = chromosome c's place in the file's chromosome order;
 *               four name tables, name i = bytes[off[i] .. off[i + 1]) (off has n + 1 elements): chromosomes, then what
 *               itx_row.rep / .cla / .fam index. Uploads (the caller's arrays are its own again on return), starts the sort on a
 *               stream of its own and returns without waiting for it. n_chrom >= 2^19, n_rows >= 2^32 - 1, or a row whose bin does
 *               not fit 13 bits (a coordinate of 460 M and above): ITX_E_RANGE, before anything is allocated. ITX_E_NOMEM: the
 *               device cannot hold the table.
 *   order       waits for the sort; order[k] = the row at place k of the file (n_rows elements); *sort_ms (optional): its device time
 *   filter_text the lines of writeFilterOut without the read lists (generic.c:1719-1728): locus_cnt[n_rows], the -t threshold, the
 *               normalising read number. cpg_text: those of writeFilterOutMRE (generic.c:1760-1766): cpg_count[n_rows],
 *               cpg_total[n_rows], the -t threshold. out->lines: lines printed; out->hard: printed lines with a double the device
 *               does not model (not finite: a read number of 0, a row of length 0; 2^63 and above) — then text is NULL and the
 *               caller writes the whole file itself. Else text[0 .. bytes) is the file behind its header line, host memory owned by
 *               the object (capacity bytes, the ones behind the text filled with 0xA5 on the device), valid until the next call.
 *               The text call of the other kind: ITX_E_ARG. ITX_E_NOMEM: no room for the text. */
typedef struct itx_loci itx_loci;
#define ITX_LOCI_FILTER 0
#define ITX_LOCI_CPG 1
typedef struct itx_loci_text {
    const char *text;
    uint64_t bytes, capacity, lines, hard;
    double sort_ms, text_ms;                   /* device time: key + sort kernels; measure + scan + write kernels of this call */
} itx_loci_text;
int itx_loci_create(int device, int kind, const itx_row *rows, const uint32_t *row_chrom, size_t n_rows, const uint32_t *chrom_rank, uint32_t n_chrom,
                    const char *chrom_bytes, const uint64_t *chrom_off, const char *rep_bytes, const uint64_t *rep_off, uint32_t n_rep,
                    const char *cla_bytes, const uint64_t *cla_off, uint32_t n_cla, const char *fam_bytes, const uint64_t *fam_off, uint32_t n_fam,
                    itx_loci **out);
void itx_loci_destroy(itx_loci *lo);
int itx_loci_order(itx_loci *lo, uint32_t *order, double *sort_ms);
int itx_loci_filter_text(itx_loci *lo, const uint32_t *locus_cnt, int threshold, unsigned long long reads_num, itx_loci_text *out);
int itx_loci_cpg_text(itx_loci *lo, const int *cpg_count, const double *cpg_total, double threshold, itx_loci_text *out);

/* ---- SAM text split and parsed on the device (iteres stat|filter -S) --------------------------------------------------------
 * A chunk of SAM body text, cut by the caller behind a newline, becomes the per-record arrays the host reader fills otherwise
 * (itx_batch's layout) plus, per record, byte offsets into the text: the caller cuts a read name or an XA value out of its own
 * copy of the text only when it wants one (csrc/itx_samtext.hip; the line rule, stated once: csrc/itx_samline.h). The device
 * models the plain spelling of every field; a line spelt otherwise is HARD: the chunk's records are then not handed out
 * (n_rec = 0) and the caller parses the chunk itself, whole and in order.
 *   create       the @SQ names, name t = name_bytes[name_off[t] .. name_off[t + 1]) (the first of equal names wins a lookup);
 *                max_chunk_bytes: the largest text one parse may carry (at most 256 MiB: ITX_E_LIMIT), which sizes the buffers of
 *                both slots. ITX_E_NO_DEVICE when there is no such device.
 *   parse_begin  slot 0 or 1: copies text[0 .. len) to the device on the object's copy stream and enqueues the kernels; returns
 *                without waiting (the text must stay as it is until parse_end). final: the input ends with this text, a last line
 *                without a newline is a line; otherwise the bytes behind the last newline are not consumed. len > max_chunk_bytes:
 *                ITX_E_LIMIT. Two slots, so that one chunk crosses the link and is parsed while the other's records are fetched;
 *                the two slots may be driven from two threads.
 *   parse_end    waits for the slot's parse. n_lines: lines in the consumed bytes; consumed: through the last '\n', all of len
 *                when final; n_hard: lines the device does not model, first_hard_line: the 0-based index of the first of them
 *                (more lines than len / 20 + 2 prove a line too short for 11 fields: counted as one more hard line);
 *                n_rec: n_lines, or 0 when n_hard > 0; flags: ITX_SAMTEXT_PAIRED / _XA some record has the PAIRED flag / an XA
 *                field, ITX_SAMTEXT_NUL the text holds a NUL byte; kernel_ms: device time of the four kernels.
 *   fetch        records [first, first + n) of the slot's parsed chunk into the staging arrays at dst_at, and their side values
 *                into whichever of the other arrays is not NULL: line_off (the line's first byte in the text), qname_len (the
 *                read name is the line's first bytes), xa_off / xa_len (the XA value; xa_mark[i] != 0: the record carries XA),
 *                nm. Waits for the copies. */
typedef struct itx_samtext itx_samtext;
#define ITX_SAMTEXT_PAIRED 1
#define ITX_SAMTEXT_XA 2
#define ITX_SAMTEXT_NUL 4
typedef struct itx_samtext_result {
    uint64_t n_lines, n_rec, consumed, n_hard, first_hard_line;
    int flags;
    double kernel_ms;
} itx_samtext_result;
int itx_samtext_create(int device, const char *name_bytes, const uint64_t *name_off, int n_targets, size_t max_chunk_bytes, itx_samtext **out);
int itx_samtext_parse_begin(itx_samtext *x, int slot, const void *text, size_t len, int final);
int itx_samtext_parse_end(itx_samtext *x, int slot, itx_samtext_result *res);
int itx_samtext_fetch(itx_samtext *x, int slot, size_t first, size_t n, const itx_staging *dst_staging, size_t dst_at, uint32_t *line_off,
                      uint32_t *qname_len, uint32_t *xa_off, uint32_t *xa_len, int32_t *nm, uint8_t *xa_mark);
void itx_samtext_destroy(itx_samtext *x);
/* The same for a SAM text that arrives as BGZF (bgzip's output: a chain of gzip members of at most 64 KiB each): the members are
 * inflated on the device by the decoder of itx_inflate_bgzf and parsed where they land, so only the compressed bytes cross the link.
 * The chunks of a file form a STREAM: the bytes behind the last newline of a chunk begun with final = 0 (its tail) are the first
 * bytes (the carry) of the next chunk's text, copied on the device.
 *   parse_begin_bgzf  the members blk[0 .. n_blk) of comp (offsets as for itx_inflate_bgzf, checked the same way: ITX_E_ARG for a
 *                list that does not fit) are copied and inflated into a buffer of the slot; the slot's text is the carry, then the
 *                inflated bytes from offset `skip` on (the file's header, which the caller has read itself; skip beyond the
 *                inflated bytes leaves none); the four kernels of parse_begin run over that text. Waits for the parse of the
 *                stream's previous chunk (its tail length is needed), for nothing of this one; comp and blk are the caller's again
 *                when parse_end returns. The previous chunk must lie in the OTHER slot (ITX_E_STATE). A chunk begun with final != 0,
 *                a chunk with a member the decoder did not take, and itx_samtext_parse_begin into the previous chunk's slot end
 *                the stream: the next chunk has no carry. ITX_E_LIMIT, nothing begun, when the members inflate to more than
 *                max_chunk_bytes + 64 KiB or the text would exceed max_chunk_bytes.
 *   parse_end    as above, over the slot's text; n_rec = 0 also when a member's status is not 0 (bgzf_info: n_bad).
 *   bgzf_info    after parse_end of a chunk begun by parse_begin_bgzf: text_len, carry_len (the text's first bytes, from the chunk
 *                before), tail_len (text_len - consumed), n_bad / first_bad: members whose status is not 0 (itx_inflate_bgzf) and
 *                the index of the first; inflate_ms: device time of the decoder's two passes.
 *   text         bytes [off, off + len) of the text of a slot whose parse has ended (begun either way), to the host.
 *   strings      the read names (want & 1) of records [first, first + n) of the slot's parsed chunk and the XA values (want & 2) of
 *                those with xa_mark != 0, gathered on the device: each followed by a NUL, packed in record order (name, then XA)
 *                into a page-locked buffer the object owns (valid until the next strings call or destroy); qname_at[i] / xa_at[i]:
 *                where record first + i's string starts in it, UINT32_MAX for none. */
typedef struct itx_samtext_bgzf_info_t {
    uint64_t text_len, carry_len, tail_len, n_bad, first_bad;
    double inflate_ms;
} itx_samtext_bgzf_info_t;
typedef struct itx_samtext_strings_out {
    const char *text;
    uint64_t text_len;
    const uint32_t *qname_at, *xa_at;
    double kernel_ms;
} itx_samtext_strings_out;
int itx_samtext_parse_begin_bgzf(itx_samtext *x, int slot, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk, size_t skip, int final);
int itx_samtext_bgzf_info(itx_samtext *x, int slot, itx_samtext_bgzf_info_t *out);
int itx_samtext_text(itx_samtext *x, int slot, size_t off, void *dst, size_t len);
int itx_samtext_strings(itx_samtext *x, int slot, size_t first, size_t n, int want, itx_samtext_strings_out *out);

/* ITX_TIMING: what the device decoder measured about itself (pushes, mean duration of the two passes, device allocations),
 * one line on stderr; also printed when the process exits normally. */
void itx_timing_report(void);

/* bigWig files of `iteres stat` built on the device from the engine's coverage (csrc/itx_bigwig.hip): every section's
 * payload and every zoom level's summaries (the arithmetic of host/bw_sum.c, one step of it in csrc/itx_bwfold.h), each block deflated into a zlib stream by
 * csrc/itx_deflate_core.h. The host lays the files down around what comes back (host/bw_dense.c write_bigwig_device).
 *   start    after itx_engine_finish / itx_engine_finish_partial; uniq: the unique-read coverage instead of all reads;
 *            the chromosomes in bigWig id order as (offset into the coverage, length > 0), the zoom reductions (each a
 *            power-of-4 multiple of the one before). Launches on a stream of its own and returns.
 *   collect  waits, then hands out the results (owned by the build until destroy): the compressed blocks packed one after
 *            the other (sections in file order, then each level's zoom blocks of 1024 summaries), block i at
 *            bytes [block_off[i], block_off[i+1]), and each level's summaries.
 * Device memory that does not fit is ITX_E_NOMEM ("itx_bigwig_start: no device memory for N bytes"); collect answers ITX_E_LIMIT
 * if the packed blocks were to exceed the room laid out for them. */
typedef struct itx_bigwig itx_bigwig;
typedef struct {
    uint32_t chrom_id, start, end, valid_count;
    float min_val, max_val, sum_data, sum_squares;
} itx_bw_summary;
typedef struct {
    uint64_t n_sec, n_blocks;
    uint32_t n_levels;
    uint64_t n_sum[10], slot_first[10];       /* summaries per level; index of the level's first zoom block */
    const itx_bw_summary *sum[10];
    const uint64_t *block_off;                /* n_blocks + 1 */
    const uint8_t *blocks;
    double device_ms;                         /* from the first kernel to the end of the last */
} itx_bw_result;
int itx_bigwig_start(itx_engine *e, int uniq, const uint64_t *cov_off, const uint32_t *len, uint32_t n_chrom, const uint32_t *reduction,
                     uint32_t n_levels, itx_bigwig **out);
int itx_bigwig_collect(itx_bigwig *b, itx_bw_result *out);
void itx_bigwig_destroy(itx_bigwig *b);

/* ---- the bigWig content of filter -W: the genome coverage of filter -G as sparse (bedGraph) data, built on the device ---------------
 * What the reference's converter, bigWigFileCreate(bedGraph, chromSizes, blockSize 256, itemsPerSlot 1024, clip 0, compress 1), makes of
 * the text that itx_gcov_next hands out for file `which` (csrc/itx_gcovbw.hip; the host lays the file down, host/bw_sparse.c
 * write_bigwig_sparse_device). An item is a line of that text: [start, end) with (float)(double)depth. Only chromosomes with an item
 * get a bigWig id; ids ascend in finish's order (the command gives strcmp order of the names, which the file's B+ tree needs).
 *   bigwig_build   after itx_gcov_finish (ITX_E_STATE before it, or when the file was built already), before, between or after the
 *                  text rounds: they do not touch each other. Sections of up to 1024 items (24-byte header, type bedGraph, 12 bytes an
 *                  item), the first reduction found by the reference's loop (only counts cross the bus), every further level, the
 *                  zoom blocks of 1024 summaries, all deflated and packed. ITX_E_NOMEM leaves the object as it was: the text can
 *                  still be taken, and the build tried again.
 *   bigwig_result  what was built (owned by the object until destroy; ITX_E_STATE when nothing was built): n_items == 0 means the file
 *                  has no data (the reference's converter refuses such an input) and nothing else is filled in. chrom[id]: index into
 *                  create's chrom_size; sec_key: (chrom id, first start, last end) per section, sec_count its items; blocks as in
 *                  itx_bw_result: the sections, then each level's zoom blocks.
 *   copy_points    the change points of file `which` as they lie on the device, 4 words each: (position, depth from here on, place of
 *                  the chromosome in finish's order, 0); out holds 4 * stats.points[which] words. For a host-side build. */
typedef struct itx_gcov_bw_result {
    uint64_t n_items, n_sec, n_blocks;
    uint32_t n_chrom, n_levels;
    const uint32_t *chrom;                    /* n_chrom */
    const uint32_t *sec_key;                  /* 3 * n_sec */
    const uint32_t *sec_count;                /* n_sec */
    uint32_t reduction[10];
    uint64_t n_sum[10], slot_first[10];
    const itx_bw_summary *sum[10];
    const uint64_t *block_off;                /* n_blocks + 1 */
    const uint8_t *blocks;
    uint32_t reduce_rounds, pad;              /* times the first reduction was counted */
    double items_ms, chain_ms, fold_ms, deflate_ms;
} itx_gcov_bw_result;
int itx_gcov_bigwig_build(itx_gcov *g, int which);
int itx_gcov_bigwig_result(itx_gcov *g, int which, itx_gcov_bw_result *out);
int itx_gcov_copy_points(itx_gcov *g, int which, uint32_t *out);

/* Page-locked host memory for the buffers that cross PCIe on every call (NULL when it cannot be had). */
void *itx_pinned_alloc(size_t bytes);
void itx_pinned_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
