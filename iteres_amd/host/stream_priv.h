/* stream_priv.h — what stream.c (the record loop), warmup.c (the helper thread) and out_names.c / out_bam.c / out_gcov.c (the three
 * consumers of the chosen rows) share: one run's state, one file's, what the helper thread hands over, the batch's rows, and the
 * same steps of every consumer. Private to those five files; itx_host.h has the public entries. */
#ifndef ITX_STREAM_PRIV_H
#define ITX_STREAM_PRIV_H
#include "itx_host.h"

#define BATCH_RECORDS (4u << 20)

/* ---- warmup.c: what the helper thread leaves. gpu_warmup_start fills first, input_bytes and splittable before the thread
 * exists. From then on the helper thread writes these fields and nobody else does until it has been joined; the main thread reads
 * them only through the pointer gpu_warmup_join returned, and owns them from there (it hands the reader to the loop, releases the
 * backlog after the first file and the decoder after the stream). While the thread runs, the only words both sides touch are the two
 * atomics behind stream_sizes_ready and the stop flag gpu_warmup_join sets. */
typedef struct {
    itx_inflater *inflater;                       /* the device decoder (NULL: it did not come up, the host decodes) */
    int dev_windows;                              /* ... and what was reserved for it on the device (itx_inflater_reserve) */
    size_t dev_max_blocks, dev_max_bytes;
    char *first;                                  /* the first alignment file, opened (and decoded ahead) by the helper thread */
    aln_reader *reader;
    size_t lo, hi;                                /* the share it was opened with */
    itx_backlog *backlog;                         /* the records parsed ahead of the table: entry k is n records at `at` */
    struct backlog_ent { size_t at, n; int paired; } *ent;
    size_t n_ent, cap_ent;
    double seconds;
    char err[400];                                /* the helper thread's last error (itx_last_error is per thread) */
    size_t input_bytes;                           /* size of all alignment files together (0: unknown) */
    int splittable;                               /* the shares of a multi-GPU job: shares.c (share_t, plan_shares) */
} helper_out;
/* the table and the engine are there: the helper thread finishes the window it is at and is joined */
helper_out *gpu_warmup_join(void);
void use_device_reader(void);                     /* the reader decodes BAM through the helper thread's decoder and chunk buffers */

typedef struct {
    uint32_t row;
    char *name;
} hit_name;

/* ---- one run of run_stream */
typedef struct {
    const run_opts *o;
    const rmsk_t *rm;
    const sizes_t *chr_sizes;
    int filter_mode, multi_file, timing;
    int want_bed, want_qnames;
    int veto_on;                                  /* filter.c:134 passes diffSubfam = 0 */
    int dev_veto;                                 /* the veto may run on the device (not ITX_HOST_VETO) */
    helper_out *h;                                /* what the helper thread left (join_helper_thread) */
    itx_table *tab;
    itx_engine *eng;
    itx_params p;
    /* the four side objects, each with its host twin. -R: one set over all files */
    itx_dedup *dd;
    dup_set *dups;
    names_t chr_names;                            /* identities of the chromosome strings inside -R keys */
    double t_dedup;
    itx_xaveto *xv;                               /* the veto on the device (windows that stay in HBM) */
    xa_index *xi;
    /* -B / -V on the device (csrc/itx_bed.hip): the text of a batch is started right after the batch is taken and written to
     * the files one batch later, so that the copy and the fwrite run beside the next batch's kernels. Both routes write to the
     * same FILE: whatever is pending is written before the host route prints a line. */
    itx_bed *bd;
    int bed_pending;
    FILE *bed_f, *bed_uniq_f;
    itx_names *nm;                                /* the read lists gathered on the device (filter -r) */
    struct { hit_name *v; size_t n, cap; } hn;    /* ... and by the host */
    struct { uint32_t *rows; uint64_t *off; char *bytes; size_t cap_n, cap_b; } nbuf;
    /* filter -b (csrc/itx_bamout.hip): the counted records become BGZF members on the device; a batch's members are written to
     * the file while the next batch's kernels run. What the host route counted goes to the same stream, in stream order. */
    itx_bamout *bo;
    FILE *bam_f;
    int bam_header_done;
    uint64_t bam_first;                            /* -b -i: where the first record member starts in the file */
    struct { uint8_t *bytes; size_t cap; } bbuf;
    unsigned long long bam_dev_batches, bam_host_batches;
    unsigned long long bam_host_tag_bytes;         /* -b -a: tag bytes the host route appended */
    int32_t *brows;                                /* -b -s -m -a: the chosen rows of a host batch's counted records */
    size_t brows_cap;
    /* filter -G (csrc/itx_gcov.hip): every counted record adds its interval to the coverage on the device, whatever route it took;
     * the host route derives the intervals of its own records (gcov_host_batch). The files are written after the stream
     * (stream_gcov_write). */
    itx_gcov *gc;
    const struct stream_file_s *cur;               /* the file being scanned: its tid map, for the host route's intervals */
    struct { int32_t *chrom; uint32_t *start, *end; uint8_t *uniq; size_t cap; } gbuf;
    /* the host route: two pinned slots, taken when a batch first goes that way; s is filled next, pend[] are in flight */
    itx_staging st[2];
    aln_side side[2];                             /* what the host keeps per record beside the SoA */
    size_t pend[2];
    int have_slots, any_side, s;
    host_iv *iv;
    uint8_t *live;                                /* the record reached the bed / veto stage */
    names_t warned;
    unsigned long long ends;
    unsigned progress_every;
    host_counts *hc;
    unsigned long long veto_dev_batches, veto_host_batches, bed_host_batches, names_host_batches, boundary_missed;
    /* the list of files and this rank's share of each (one rank: all of it) */
    char *arg, *files[100];
    int n_files, shared;
    share_t share[100];
} stream_run;

/* ---- one file of it */
typedef struct stream_file_s {
    aln_reader *rd;
    int nt;                                       /* the header's references: chromosome, -R identity, (renamed) name of each */
    int32_t *t2c;
    uint32_t *t2id;
    char **t2name;
    int dev_bed, dev_names, handoff_ok, any_paired;
    double t_wait, t_read, t_host, t_submit;
    double t_open0, t_opened, t_loop_done;
} stream_file;

/* ---- stream.c: rules both threads apply */
int32_t chrom_of_target(const char *target, const run_opts *o, const sizes_t *chr_sizes);
int window_goes_direct(int wfl, const uint8_t *seen, const int32_t *t2c, int nt, int veto_on, int dev_veto);

/* ---- the chosen rows of one batch of the device route: ONE classification for all takers. The first consumer that is on asks
 * for them (batch_rows), every later one reads what it left. The owner of the buffer and the stream is the first that exists of
 * lists, BAM, coverage. When that is the lists or the BAM, what the host route still holds of earlier batches is collected first
 * (their files are in stream order); the coverage alone does not wait for it: sums commute. */
typedef struct {
    const int32_t *hits;                          /* on the device: the row every record of the batch chose, or < 0 */
    void *stream;                                 /* ... written on this stream: a gather queued there follows it */
    int done;
} chosen_rows;
void batch_rows(stream_run *r, const itx_batch *db, size_t n, chosen_rows *rows);

/* ---- out_names.c (filter -r), out_bam.c (filter -b with -i, -s, -a, -l), out_gcov.c (filter -G / -W): the same steps in each, called by
 * stream.c in the fixed order lists, BAM, coverage. Each does nothing when its output is off.
 *   _open          the device object and what it needs set up (map_targets; the coverage, which has no header to wait for: run_stream)
 *   _rows          1 and the object's own rows buffer and stream when the object exists (batch_rows picks the owner)
 *   _device_batch  the gather over the batch the device route has just taken, on the batch's rows
 *   _host_batch    the same for the records of host slot k, whose rows are back
 *   _window_done   the object's kernels are through with the window's arrays (or, before a host batch, with everything)
 *   _finish        the end of the stream, with the ITX_TIMING line (the coverage's is stream_gcov_write, after run_stream)
 *   _free          the host route's buffers */
void lists_open(stream_run *r, stream_file *f);                  /* sets f->dev_names */
int lists_rows(stream_run *r, int32_t **hits, void **stream);
int lists_device_batch(stream_run *r, stream_file *f, const itx_batch *db, size_t n, chosen_rows *rows);   /* 0: a name only the host can read */
void lists_host_batch(stream_run *r, int k);
void lists_window_done(stream_run *r);
void lists_finish(stream_run *r, char ***locus_names);
void lists_free(stream_run *r, int lists_taken);

void bam_open(stream_run *r, stream_file *f);
int bam_rows(stream_run *r, int32_t **hits, void **stream);
void bam_device_batch(stream_run *r, stream_file *f, const itx_batch *db, size_t n, chosen_rows *rows);
void bam_host_batch(stream_run *r, int k);
void bam_window_done(stream_run *r);
void bam_finish(stream_run *r);
void bam_free(stream_run *r);

void gcov_open(stream_run *r);
void gcov_tidmap(stream_run *r, const stream_file *f);           /* a new file's header (attach_tidmaps) */
int gcov_rows(stream_run *r, int32_t **hits, void **stream);
void gcov_device_batch(stream_run *r, const itx_batch *db, size_t n, chosen_rows *rows);
void gcov_host_batch(stream_run *r, int k);
void gcov_window_done(stream_run *r);
void gcov_free(stream_run *r);

#endif
