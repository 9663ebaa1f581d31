/* itx_host.h — the C host side of the drop-in: `iteres stat` / `iteres filter` with the reference's command
 * line, stderr banners, exit codes and output file formats (stat.c, filter.c, generic.c:53-113,1709-1746 of
 * /root/reference), driving the MI355X engine through include/iteres_amd.h. Everything here is host logic:
 * parsing, name bookkeeping in the reference's hash iteration order, BAM/SAM decoding into the pinned record
 * SoA, and the writers. There is no CPU implementation of the hot path in this program. */
#ifndef ITX_HOST_H
#define ITX_HOST_H
#include <stdint.h>
#include <stdio.h>
#include <stddef.h>
#include <time.h>

#include "../../include/iteres_amd.h"

#define ITERES_VERSION "0.3.3-r123"      /* generic.h:4 of the reference: same version string in the usage text */

/* ---- errors: cuskent/errabort.c:166-199 — message + newline to stderr, exit(-1) */
void die(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));
void warnf(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
extern FILE *itx_err_stream;             /* where die / warnf write when not stderr (ranks > 0 of a multi-GPU job) */
extern const char *itx_err_prefix;
extern void (*itx_die_hook)(void);        /* run by die() before it leaves (rank 0 ends the ranks it started) */
static inline double now_s(void)           /* seconds on the monotonic clock */
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static inline void chk(int rc, const char *what)   /* an ABI call that must not fail */
{
    if (rc != ITX_OK) die("%s: %s", what, itx_last_error());
}
void *xmalloc(size_t n);
void *xcalloc(size_t n, size_t sz);
void *xrealloc(void *p, size_t n);
char *xstrdup(const char *s);

/* ---- string -> dense id table that remembers insertion order and can list its names in the iteration
 * order of a kent hash (cuskent/hash.c:41-53,115-142,374-410,511-552) built by the same insertions. */
typedef struct {
    char **name;
    uint32_t n, cap;
    uint32_t *bucket;      /* open hashing for lookups */
    uint32_t *next;
    uint32_t nbucket;
} names_t;
void names_init(names_t *t);
void names_free(names_t *t);
int64_t names_find(const names_t *t, const char *s);
uint32_t names_intern(names_t *t, const char *s);             /* id of s, adding it when new */
uint32_t kent_hash_string(const char *s);                     /* cuskent/hash.c:41-53 */
/* order[i] = id of the i-th name hashFirst/hashNext would visit (hash started with 2^start_pow2 buckets). */
void names_kent_order(const names_t *t, int start_pow2, uint32_t *order);

/* ---- two-column "name value" files (cuskent/obscure.c:139-150 hashNameIntFile): later duplicates win */
typedef struct {
    names_t names;
    int64_t *value;
} sizes_t;
void sizes_load(const char *path, sizes_t *out);
void sizes_free(sizes_t *s);
/* value of name or dflt (hashIntValDefault, cuskent/hash.c:250-258) */
int64_t sizes_get(const sizes_t *s, const char *name, int64_t dflt);

/* ---- rmsk.txt -> rows + name tables (generic.c:1578-1707 without the binKeeper) */
typedef struct {
    names_t chroms;            /* chromosomes that got a binKeeper, in first-seen order: key order of hashRmsk   */
    names_t reps, fams, clas;  /* hashRep / hashFam / hashCla insertion order                                     */
    itx_row *rows;             /* kept rows, file order; .chrom indexes chrom_size                                */
    uint32_t *row_chrom_name;  /* [n_rows] index into chroms                                                      */
    size_t n_rows;
    int64_t *chrom_size;       /* [chroms.n] size from the chrom-size file                                        */
    uint32_t *rep_len;         /* [reps.n]  repeat-size file value or 0 (generic.c:1647)                          */
    uint32_t *rep_fam, *rep_cla;   /* family / class string ids of the FIRST row of each name (generic.c:1638-1640) */
    uint32_t *fam_cla;         /* class of the first row of each family (generic.c:1667-1668)                     */
    uint64_t *rep_genome, *rep_total, *fam_genome, *fam_total, *cla_genome, *cla_total;   /* genome_count, total_length */
    int repeat_num;            /* rows counted by the banner (generic.c:1593,1697)                                */
} rmsk_t;
void rmsk_load(const char *path, const sizes_t *chr_sizes, const sizes_t *rep_sizes, int filter_field, const char *filter_name,
               rmsk_t *out);
void rmsk_free(rmsk_t *r);

/* ---- alignment input: BAM (BGZF) or SAM text, decoded into the engine's record SoA */
typedef struct aln_reader aln_reader;
/* BAM decoding on the device (include/iteres_amd.h: itx_bamwin_*): BGZF blocks inflated, records located and parsed there;
 * the reader only moves compressed bytes in and the per-record arrays out. The reader stays free of any link-time
 * dependency on the HIP library: the driver hands it the entry points before it opens a file. `alloc` / `release`:
 * page-locked memory for the compressed chunks. NULL restores the host decoder. */
typedef struct aln_device_ops {
    itx_inflater *ctx;
    int (*push_begin)(itx_inflater *, int, int, const void *, size_t, const itx_bgzf_block *, size_t);
    int (*push_end)(itx_inflater *, int, uint8_t *, size_t *);
    int (*patch)(itx_inflater *, int, size_t, const void *, size_t);
    int (*truncate)(itx_inflater *, int, size_t);
    int (*carry)(itx_inflater *, int, int);
    int (*avail)(const itx_inflater *, int, size_t *);
    int (*peek)(itx_inflater *, int, size_t, void *, size_t);
    int (*skip)(itx_inflater *, int, size_t);
    int (*parse)(itx_inflater *, int, int, size_t *, int *, int *, size_t *);
    int (*fetch)(itx_inflater *, size_t, size_t, const itx_staging *, size_t, uint32_t *, uint8_t *);
    int (*bytes)(itx_inflater *, size_t, void *, size_t);
    int (*tids)(itx_inflater *, uint8_t *, int);
    int (*device_batch)(itx_inflater *, size_t, int, itx_batch *);
    void *(*alloc)(size_t bytes);
    void (*release)(void *p);
    const char *(*last_error)(void);
    /* what the driver reserved on the device (itx_inflater_reserve): windows to rotate through, blocks / inflated bytes per push;
     * zeros: the defaults (ITX_BAMWIN_WINDOWS, 16384 blocks, 1 GiB) with buffers that grow on demand */
    int n_windows;
    size_t max_blocks, max_bytes;
    int (*xa_veto)(itx_inflater *, itx_xaveto *, size_t, size_t, uint64_t *, uint64_t *);      /* itx_bamwin_xa_veto */
    int (*push_copied)(itx_inflater *, int);       /* itx_bamwin_push_copied: lane s's compressed bytes have left the caller's buffer */
    int (*bed)(itx_inflater *, itx_bed *, size_t, size_t, uint64_t *);                         /* itx_bamwin_bed */
    int (*names)(itx_inflater *, itx_names *, size_t, size_t, const int32_t *, void *, uint64_t *);   /* itx_bamwin_names */
    int (*bamout)(itx_inflater *, itx_bamout *, size_t, size_t, const int32_t *, void *);             /* itx_bamwin_bamout */
} aln_device_ops;
void aln_use_device(const aln_device_ops *ops);
size_t aln_raw_step(size_t left);           /* bytes per read step of a regular file with `left` bytes to go (after aln_use_device) */
/* compressed bytes per chunk handed to the device decoder (ITX_BGZF_CHUNK overrides). Pass 1 of the decoder is a lane per
 * block and bound by the latency of one block's symbol chain (~29 ms for a block of literal-heavy content, whatever the number
 * of blocks, until every SIMD holds a wave: 65 k blocks): its throughput is the blocks in flight. Blocks of real BAM content
 * take ~33 KB compressed, so 384 MB = 12 k blocks per push, four pushes in flight = 48 k blocks (round 2: 128 MB, written for
 * blocks of 15 KB). Measured, 200 M reads of 40-value-quality content: record loop 1.35 s -> 0.64 s. */
#define ALN_DEVICE_CHUNK (384u << 20)
#define ALN_DEVICE_RAW_BUFFERS 5             /* page-locked chunk buffers the reader of a regular file rotates through (bamio.c) */
/* Device decoder only. aln_device_window: 1 when the next records can be taken as DEVICE arrays — the reader stands at
 * the start of a decoded window (decoding the next one if need be); *flags: bit 0 some record of the window is paired,
 * bit 1 some record carries an XA tag; *tid_seen[n_targets]: references with a mapped record in the window. 0: host
 * decoder, end of input, or in the middle of a window: use aln_read_batch (which then stops at the window's end).
 * aln_read_batch_device: the next <= cap records of that window as device arrays, valid until the next reader call. */
int aln_device_window(aln_reader *r, int *flags, const uint8_t **tid_seen);
/* Device decoder only: fn(ctx, n_rec) is called once for every window right after its records have been located and parsed, in
 * file order, before any of them is handed out (-R on the device marks its duplicates there: stream.c dedup_window) */
void aln_set_window_hook(aln_reader *r, void (*fn)(void *ctx, size_t n_rec), void *ctx);
size_t aln_read_batch_device(aln_reader *r, size_t cap, itx_batch *b);
/* the XA veto over the batch aln_read_batch_device has just handed out (its chosen rows are in the veto object's buffer);
 * aln_device_rewind: hand the current window's records out again from its first one (the host route after all) */
int aln_device_xa_veto(aln_reader *r, itx_xaveto *x, size_t n, uint64_t *n_vetoed, uint64_t *n_hard);
/* the bed text of the batch aln_read_batch_device has just handed out, started on the device (itx_bed_collect delivers it) */
int aln_device_bed(aln_reader *r, itx_bed *b, size_t n, uint64_t *n_hard);
/* the names of the batch aln_read_batch_device has just handed out, appended to the read lists on the device: d_hit_row holds the
 * batch's chosen rows, written on `stream` */
int aln_device_names(aln_reader *r, itx_names *nm, size_t n, const int32_t *d_hit_row, void *stream, uint64_t *n_hard);
/* the records of that batch that chose a row, appended to the BAM of filter -b on the device (same arguments) */
int aln_device_bamout(aln_reader *r, itx_bamout *bo, size_t n, const int32_t *d_hit_row, void *stream);
void aln_device_rewind(aln_reader *r, size_t n);       /* the last n records handed out by aln_read_batch_device are handed out again (by whichever route reads next) */
size_t aln_device_left(const aln_reader *r);  /* device decoder: records of the current window not yet taken */
int aln_device_exhausted(aln_reader *r);
void aln_readahead(aln_reader *r);            /* BAM: start decoding ahead of the first aln_read_batch */     /* device decoder: 1 when no record is left */
aln_reader *aln_open(const char *path, int is_sam);          /* NULL when the file cannot be opened / has no header */
/* SAM text split and parsed on the device (include/iteres_amd.h: itx_samtext_*). aln_open never touches the GPU: the driver,
 * which knows the device, makes the object from the reader's reference names and attaches it before the first batch is read;
 * entry points instead of a link-time dependency, as for aln_device_ops. The body of the file is then read in chunks of
 * ITX_SAM_CHUNK bytes (default ALN_SAM_CHUNK) cut behind a newline, by a read-ahead thread into two buffers from `alloc`; a
 * chunk's records come from the device's arrays, its read names and XA strings from the host's copy of the text by offset. A
 * chunk with a line the device does not model (csrc/itx_samline.h) is parsed by the host, whole and in order. Without an
 * attached object the reader takes line after line with getline, or — ITX_SAM_CHUNK set — the same chunks all by the host.
 * -S input is read through zlib, as the reference reads it: gzip, BGZF and a mix of both are SAM text too. With an object attached
 * and its BGZF entries set, a file whose first member is BGZF is inflated on the device as well (ITX_HOST_SAM_INFLATE=1: by the
 * host): the read-ahead thread reads whole members from the file's own descriptor until they inflate to ITX_SAM_CHUNK bytes, the
 * device inflates them, carries the unconsumed tail from chunk to chunk and gathers the strings a side channel wants. A chunk the
 * decoder cannot take whole (a member that does not inflate, a member that is not BGZF, a member the file's end cuts short) hands
 * the rest of the file over to the host's zlib reader, from that chunk's first member on and for good. */
typedef struct aln_sam_device {
    itx_samtext *obj;
    int (*parse_begin)(itx_samtext *, int, const void *, size_t, int);
    int (*parse_end)(itx_samtext *, int, itx_samtext_result *);
    int (*fetch)(itx_samtext *, int, size_t, size_t, const itx_staging *, size_t, uint32_t *, uint32_t *, uint32_t *, uint32_t *, int32_t *, uint8_t *);
    void *(*alloc)(size_t bytes);
    void (*release)(void *p);
    const char *(*last_error)(void);
    /* BGZF inflated on the device (all four, or none) */
    int (*parse_begin_bgzf)(itx_samtext *, int, const void *, size_t, const itx_bgzf_block *, size_t, size_t, int);
    int (*bgzf_info)(itx_samtext *, int, itx_samtext_bgzf_info_t *);
    int (*text)(itx_samtext *, int, size_t, void *, size_t);
    int (*strings)(itx_samtext *, int, size_t, size_t, int, itx_samtext_strings_out *);
} aln_sam_device;
#define ALN_SAM_CARRY ((size_t)1 << 20)     /* room the device object gets for the tail one chunk leaves to the next */
#define ALN_SAM_CHUNK ((size_t)64 << 20)
size_t aln_sam_chunk_bytes(void);           /* ITX_SAM_CHUNK, or the default */
void aln_set_sam_device(aln_reader *r, const aln_sam_device *d);
/* One rank's share of a BAM file (multi-GPU; device decoder): the records that start between the split points of the
 * compressed byte offsets lo and hi (hi = SIZE_MAX: to the end; (0, SIZE_MAX) is aln_open). aln_range_verified, after the
 * last batch: 1 when the share's end boundary proved to be a true record start (or the share runs to the end of the file). */
aln_reader *aln_open_range(const char *path, size_t lo, size_t hi);
int aln_range_verified(const aln_reader *r);
/* the split point at or after compressed byte `at` (1 found: BGZF block at file offset *block, *off inflated bytes into it,
 * the block takes *csize bytes; 0 none before the end of the file; -1 the file cannot be read) */
int aln_find_split(const char *path, size_t at, size_t *block, size_t *off, size_t *csize);
void aln_close(aln_reader *r);
/* filter -b: readers opened after aln_keep_header(1) keep the bytes of the BAM header as they read them (magic, text, reference
 * list: what a BAM that carries the same records starts with); aln_header_bytes hands them out (NULL: not kept, or SAM) */
void aln_keep_header(int on);
const uint8_t *aln_header_bytes(const aln_reader *r, size_t *len);
/* bgzf.c: the bytes as BGZF members of at most 0xff00 bytes each, made with zlib; the 28-byte EOF marker. 0, or -1 when writing fails */
int bgzf_write_members(FILE *f, const uint8_t *bytes, size_t len);
int bgzf_write_eof(FILE *f);
int aln_n_targets(const aln_reader *r);
const char *aln_target_name(const aln_reader *r, int tid);
/* What the decoder keeps per record beside the SoA, when the caller wants it (arrays of the batch capacity). */
typedef struct {
    int want_qnames, want_aux;
    int has_strings;           /* set by the reader when the batch left any string behind (else every entry is still NULL)       */
    char **qname;              /* malloc'd copies of the read names (filter -r, stat -B/-V)                              */
    char **xa;                 /* malloc'd value of the XA:Z tag, NULL when the record has none (bam_aux2Z, bam_aux.c:193) */
    int32_t *nm;               /* NM:i, 0 when absent (bam_aux2i, bam_aux.c:159-170)                                      */
    /* filter -b, batches of a device-decoded window that take the host route: the records' bytes as they lie in the window
     * (record i: raw + raw_off[i], 4 + its block_size bytes), valid until the slot is filled again */
    int want_raw;
    uint8_t *raw;
    size_t raw_len, raw_cap;
    size_t *raw_off;
} aln_side;
/* Fills up to cap records of the staging slot; returns the number read (0 at end of input).
 * side may be NULL. *any_paired is set when a record with the PAIRED flag was seen; *aux_xa when one carries an XA tag. */
size_t aln_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa);

/* ---- shared by the two drivers */
typedef struct {
    int is_sam, add_chr, treat, discard, keep_wig, xa_veto, dedup;
    unsigned mapq, isize, extension;
    float min_cov;
    const char *chr_size_file, *rep_size_file, *rmsk_file, *aln_arg;
    const char *bed_path, *bed_uniq_path;      /* stat -B / -V (generic.c:925-936), NULL = off */
    const char *bam_out_path;                  /* filter -b (an extension): the counted records as a BAM, NULL = off */
    int bam_sort;                              /* filter -b -s: the counted records leave sorted by coordinate (held and sorted on the device) */
    int bam_level;                             /* filter -b -l: the members' level (0, 1 or 6), read only when bam_level_given: without -l the */
    int bam_level_given;                       /* writer is not told a level and ITX_TIMING's line is the one it always was */
    int bam_index;                             /* filter -b -i: <bam_out_path>.bai beside it, built on the device in the same pass */
    int bam_annotate;                          /* filter -b -a: every emitted record carries the tags of its row (csrc/itx_reptag.h) */
    int bam_mates;                             /* filter -b -s -m: the mates of the counted pairs are emitted too (csrc/itx_materule.h) */
    int gcov;                                  /* filter -G (an extension): the counted reads' genome coverage as bedGraph (csrc/itx_gcov.hip) */
} run_opts;
/* counters of the record loop that only the host sees (generic.c:1048-1060) */
typedef struct {
    unsigned long long diff_subfam;            /* cnt[12]: records the XA veto dropped                                  */
    unsigned long long dup_unique;             /* MAPQ >= -Q records -R dropped: cnt[11] = cnt[7] - dup_unique         */
} host_counts;

/* ---- side.c: the string / file-order parts of the record loop */
typedef struct {
    uint32_t start, end;
    char strand;
} host_iv;
/* generic.c:764-905 (itx_derive of ../csrc/itx_derive.h): 1 when the record reaches reads_mapped++ (then *d is its interval), chrom as in the tid map */
int host_derive(const run_opts *o, int32_t chrom, int64_t chrom_size, unsigned flag5, int32_t pos, int32_t tmpend, int32_t mpos, int32_t isize,
                host_iv *d);
typedef struct dup_set dup_set;
dup_set *dup_set_new(void);
void dup_set_free(dup_set *s);
int dup_set_seen(dup_set *s, uint32_t chr_name_id, const host_iv *d, int uniq);      /* generic.c:907-919: 1 = drop */
typedef struct xa_index xa_index;
xa_index *xa_index_new(const rmsk_t *rm);
uint32_t *xa_rep_words(const rmsk_t *rm);            /* [reps.n] equal for names that differ only in case (sameWord); caller frees */
void xa_index_free(xa_index *x);
/* generic.c:303-341: 1 = veto. chosen_rep: repName id of the chosen row; xa is chopped in place. */
int xa_veto(const xa_index *x, uint32_t chosen_rep, int nm, char *xa, int qlen);
/* generic.c:7-15 */
char *filename_without_ext(const char *path);
/* Runs the record loop (generic.c:700-1062 / 343-697) over one or more files through the engine.
 * progress_every: 100000 (stat, generic.c:760) or 10000 (filter, generic.c:397). want_qnames: per-locus read
 * names (filter -r): *locus_names[row] receives a comma-joined list in BAM order (NULL: no read chose the row). */
/* records parsed ahead of the table by the helper thread (warmup.c): allowed when nothing per record is the host's business;
 * the size file's table has to be announced once it is loaded */
void stream_prefetch_allow(const run_opts *o, int filter_mode, int allowed);
void stream_sizes_ready(const sizes_t *chr_sizes);
void gpu_warmup_start(int bam_input, const char *aln_arg, int multi_file, int splittable);  /* warmup.c: starts the HIP runtime on a helper thread (and, for BAM input, the device inflater
                                        * with its page-locked buffers); run_stream joins it */
void run_stream(const run_opts *o, const rmsk_t *rm, const sizes_t *chr_sizes, int filter_mode, int multi_file,
                unsigned progress_every, int want_qnames, itx_engine **eng_out, itx_table **tab_out, char ***locus_names,
                host_counts *hc);

/* writers (generic.c:35-41,53-113,1709-1746) */
double cal_rpkm(unsigned long long reads, unsigned long long total_length, unsigned long long mapped);
double cal_rpm(unsigned long long reads, unsigned long long mapped);
void write_report(const char *path, const uint64_t *cnt, unsigned mapq, const char *subfam);
void write_wig_and_stat(const rmsk_t *rm, const itx_result *res, const uint64_t *cov_off, const char *f_stat, const char *f_wig,
                        const char *f_fam, const char *f_cla, const char *f_wig_uniq, unsigned long long reads_num,
                        unsigned long long reads_num_unique);
/* The .loci file's order sorted and its lines formatted on the device (include/iteres_amd.h: itx_loci_*). loci_dev_begin, right
 * after the table is loaded: decides the route (ITX_HOST_LOCI; filter -r stays with the host) and starts the device's sort, which
 * runs beside whatever the command does next; the writer takes the device's text, or writes the file itself when the route is the
 * host's, the device cannot hold the table, or a line holds a number the device does not print. ITX_TIMING: one line says which.
 * kind: ITX_LOCI_FILTER / ITX_LOCI_CPG; device: the HIP device. dev may be NULL: the host writes, no timing line. */
typedef struct loci_dev loci_dev;
loci_dev *loci_dev_begin(const rmsk_t *rm, int kind, int readlist, int device);
void loci_dev_free(loci_dev *d);
/* a name table in the form itx_loci_create and itx_bamout_annotate_enable take: name i = bytes[off[i] .. off[i + 1]); the caller frees both */
void loci_name_table(const names_t *t, char **bytes, uint64_t **off);
void write_filter_out(const rmsk_t *rm, const uint32_t *locus_cnt, char **locus_names, const char *path, int readlist, int threshold,
                      const char *subfam, unsigned long long reads_num, loci_dev *dev);

/* bw_dense.c (with bigwig.c, bw_sum.c; bw_priv.h): the bigWig of one set of wig blocks (stat.c:156-158); only names with a consensus
 * length belong here */
void write_bigwig(const char *path, const char *wig_name, const char *const *names, const uint32_t *len, const float *const *val,
                  size_t n_names);
/* The same file in two steps, with the blocks from the device (include/iteres_amd.h: itx_bigwig_*): the plan is the layout,
 * made from names and lengths alone — chromosome i of the file is names[src[i]] with size[i], and the zoom reductions —
 * and write_bigwig_device lays the file down around what the device built for that plan. */
typedef struct bw_plan bw_plan;
bw_plan *bw_plan_make(const char *wig_name, const char *const *names, const uint32_t *len, size_t n_names);
size_t bw_plan_chroms(const bw_plan *p, const size_t **src, uint32_t *size);
int bw_plan_levels(const bw_plan *p, const uint32_t **reductions);
void write_bigwig_device(const bw_plan *p, const char *path, const itx_bw_result *dev);
void bw_plan_free(bw_plan *p);
/* bw_sparse.c: sparse data, the bigWig of a bedGraph (filter -W): what the reference's converter makes of the lines "name start end value".
 * names / sizes: the chromosomes; items: grouped by chromosome (chrom: index into names), the chromosomes that occur in strcmp order
 * of their names, starts ascending, no overlap. write_bigwig_sparse builds everything here with zlib (the reference's bytes),
 * write_bigwig_sparse_device lays the file down around what itx_gcov_bigwig_build left. Both return 0 and write nothing when there
 * is no item (the converter refuses such an input), 1 otherwise. */
typedef struct {
    uint32_t chrom, start, end;
    float val;
} bw_item;
int write_bigwig_sparse(const char *path, const char *const *names, const uint32_t *sizes, const bw_item *items, size_t n_items);
int write_bigwig_sparse_device(const char *path, const char *const *names, const uint32_t *sizes, const itx_gcov_bw_result *dev);
/* tables.c: a whole text file in memory, through the same openers as the rmsk file (plain, .gz/.Z, .bz2, .zip) */
char *slurp_text(const char *path, size_t *len);

/* ---- multi.c: one process per GPU. `iteres stat|filter` starts N - 1 more copies of itself (ranks 1..N-1, GPU r each;
 * N = ITX_GPUS, default: every GPU the process may use, as far as the input is worth sharing; ITX_GPU_MAP=a,b,.. names
 * other devices) before anything touches a GPU; a launcher that starts the ranks
 * itself (bench.py under torch.distributed.run) sets ITX_RANK / ITX_WORLD / ITX_DEVICE / ITX_COMM_ID / ITX_EXCHANGE instead.
 * Every rank parses the same inputs, holds a replica of the table and takes its share of the alignment files' compressed
 * bytes (stream.c list_files_and_shares; the first file's by the helper thread, warmup.c); ONE sum-reduce of the engines' partials onto rank 0 ends the stream (include/iteres_amd.h: itx_comm_*),
 * rank 0 writes the files, the others leave. */
void multi_early(int argc, char **argv);            /* from main(): picks up a launcher's rank, quiets ranks > 0 */
void multi_begin(int splittable, const char *aln_arg, int multi_file);   /* after the options are known, before the first GPU call: starts the other ranks */
/* shares.c: this rank's share of every alignment file (compressed byte ranges; aln_open_range turns them into record boundaries) */
typedef struct {
    size_t lo, hi;             /* hi = SIZE_MAX: to the end of the file; lo == hi: nothing of this file */
} share_t;
/* sh[fi] for `rank` of `world`; returns 0 when the job cannot be shared (then rank 0 has everything, the others nothing):
 * not splittable, a file that is no regular file, or less than min_share compressed bytes per rank */
int plan_shares(char **files, int n_files, int splittable, int rank, int world, size_t min_share, share_t *sh);
size_t multi_min_share(void);                       /* compressed bytes below which a share is not worth a rank (ITX_SPLIT_MIN) */
void multi_finish(void);                            /* rank 0, before it returns: the ranks it started have all left */
int multi_rank(void);
int multi_world(void);
int multi_device(void);
int multi_comm_mode(void);
int multi_selftest(void);
const char *multi_comm_id(void);
/* exchange.c: the ONE exchange of a multi-rank job. exchange_comm_early (helper thread, once the HIP runtime is up) starts the RCCL
 * communicator beside the scan; exchange_partials exports the engine's partial into its own buffers (*d_u64 / *d_u32), agrees
 * with the other ranks on RCCL or files, sums partials and meta[] onto rank 0 and ends the ranks above 0 */
void exchange_comm_early(void);
int exchange_comm_early_wanted(void);   /* this run will make its communicator beside the scan (asked before any thread is started) */
void exchange_partials(itx_engine *eng, uint64_t *meta, size_t n_meta, int timing, void **d_u64, void **d_u32);
/* stream.c: what the writers read — itx_engine_finish, or, after a multi-GPU stream, the same from the reduced partial */
int stream_finish(itx_engine *eng, const itx_result *res);
/* out_names.c: filter -r with the lists built on the device: after run_stream, the number of names per table row (NULL: the host built the
 * lists, every locus_names[row] is a string of its own); stream_names_free releases the lists (locus_names[] point into them) */
const uint32_t *stream_names_counts(void);
void stream_names_free(char **locus_names);
/* out_gcov.c: filter -G / -W: after run_stream, the files of the coverage the stream accumulated on the device (csrc/itx_gcov.hip). text[2]: the
 * two bedGraph files (NULL: -G was not given, no text round runs), chromosomes in byte-wise order of their names; round k is written
 * while round k + 1 is formatted. bigwig[2]: the two bigWig files of the same lines (NULL: no -W; csrc/itx_gcovbw.hip, or with
 * ITX_BW_HOST=1 zlib on the host); a file without a line is not written, one of that name is removed. Releases the object. */
void stream_gcov_write(const sizes_t *chr_sizes, const char *const *text, const char *const *bigwig);

int main_cpgstat(int argc, char **argv);
int main_cpgfilter(int argc, char **argv);

void write_cpg_loci(const rmsk_t *rm, const int *cpg_count, const double *cpg_total, const char *path, const char *subfam, double threshold, loci_dev *dev);

int main_stat(int argc, char **argv);
int main_filter(int argc, char **argv);
/* numa.c */
void numa_place(void);              /* at program start, before any thread: ITX_CPUS, else the processors of the GPU's memory node (ITX_NUMA=0: no) */
void numa_spawn_begin(void);        /* around the start of another rank: it inherits the affinity the process was started with */
void numa_spawn_end(void);

#endif
