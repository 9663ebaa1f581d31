/* stream.c — the record loop of the reference (generic.c:700-1062 stat copy, 343-697 filter copy) as a host pipeline around the
 * GPU engine. run_stream is the list of steps; record_loop is the dispatcher: a BAM window the device decoder parsed goes to the
 * engine where it lies (device_window: per batch bed text, names, veto, progress, submit — the reference's order) when the file
 * may hand off and window_goes_direct; everything else, and the rest of a window only the host can read (host_takes_over), goes
 * through host_batch: one pinned staging slot decoded while the other is in flight, then warnings with progress, -R and bed lines
 * in file order, the XA veto (side.c), submit. First in the file: the helper thread that starts the runtime and decodes ahead. */
#define _GNU_SOURCE
#include "itx_host.h"
#include "../csrc/itx_bamsortrule.h"
#include "../csrc/itx_reptag.h"

#include <errno.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string.h>
#include <strings.h>
#include <time.h>

#define BATCH_RECORDS (4u << 20)

/* The first HIP call costs a few hundred milliseconds of runtime start-up; a helper thread pays them while the main
 * thread parses the rmsk file. */
#include <pthread.h>
static pthread_t warm_thread;
static int warm_on, warm_bam;
static char *warm_first;                      /* the first alignment file, opened (and decoded ahead) by the helper thread */
static aln_reader *warm_reader;
static int warm_single;                       /* the argument names one file */
static size_t warm_lo, warm_hi = SIZE_MAX;    /* the share the helper thread opened it with */

/* BAM input is decoded on the device (include/iteres_amd.h: itx_bamwin_*: blocks inflated, records located and parsed
 * there) unless ITX_HOST_INFLATE is set. The reader's compressed-chunk buffers then have to be page-locked, which takes
 * its time: the helper thread gets them ready while the main thread parses the rmsk file, and hands them out from this
 * little pool. */
static itx_inflater *g_inflater;
#define POOL_N (ITX_BAMWIN_LANES + 2)
static struct { void *p; size_t cap; int used; } pool[POOL_N];
static pthread_mutex_t pool_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t pool_cv = PTHREAD_COND_INITIALIZER;
static int pool_pinning;                       /* buffers the pinning thread (pin_main) has yet to deliver */
static void *pool_alloc(size_t n)
{
    pthread_mutex_lock(&pool_mu);
    int best = -1;
    for (;;) {
        for (int i = 0; i < POOL_N; i++)
            if (pool[i].p && !pool[i].used && pool[i].cap >= n && (best < 0 || pool[i].cap < pool[best].cap)) best = i;
        if (best >= 0 || pool_pinning <= 0) break;
        pthread_cond_wait(&pool_cv, &pool_mu);                       /* one is being locked right now: it will be here sooner than one of our own */
    }
    if (best >= 0) pool[best].used = 1;
    pthread_mutex_unlock(&pool_mu);
    if (best >= 0) return pool[best].p;
    /* a fresh one joins the pool when there is a place: released, it stays locked (for the next file; unlocking 384 MB takes
     * 30 ms, and at the end of the run the process leaves without) */
    void *p = itx_pinned_alloc(n);
    if (p) {
        pthread_mutex_lock(&pool_mu);
        for (int i = 0; i < POOL_N; i++)
            if (!pool[i].p) {
                pool[i].p = p;
                pool[i].cap = n;
                pool[i].used = 1;
                break;
            }
        pthread_mutex_unlock(&pool_mu);
    }
    return p;
}
static void pool_release(void *p)
{
    pthread_mutex_lock(&pool_mu);
    for (int i = 0; i < POOL_N; i++)
        if (pool[i].p == p) {
            pool[i].used = 0;                                        /* stays locked for the next file */
            pthread_mutex_unlock(&pool_mu);
            return;
        }
    pthread_mutex_unlock(&pool_mu);
    itx_pinned_free(p);
}

/* what the helper thread reserved on the device for the decoder (itx_inflater_reserve) */
static int g_dev_windows;
static size_t g_dev_max_blocks, g_dev_max_bytes;

static void use_device_reader(void)
{
    const aln_device_ops ops = {g_inflater,       itx_bamwin_push_begin, itx_bamwin_push_end, itx_bamwin_patch, itx_bamwin_truncate, itx_bamwin_carry, itx_bamwin_avail, itx_bamwin_peek,
                                itx_bamwin_skip, itx_bamwin_parse, itx_bamwin_fetch, itx_bamwin_bytes,    itx_bamwin_tids,  itx_bamwin_device_batch,
                                pool_alloc,      pool_release,     itx_last_error,   g_dev_windows,       g_dev_max_blocks, g_dev_max_bytes, itx_bamwin_xa_veto, itx_bamwin_push_copied,
                                itx_bamwin_bed,  itx_bamwin_names, itx_bamwin_bamout};
    aln_use_device(&ops);
}

/* the shares of a multi-GPU job: shares.c (share_t, plan_shares) */
static int warm_splittable;
static size_t warm_input_bytes;               /* size of all alignment files together (0: unknown) */

static char warm_err[400];                    /* the helper thread's last error (itx_last_error is per thread) */

/* generic.c:781-791 (-C): NULL when the record is skipped ("GL*"), else the (possibly renamed) chromosome */
static const char *rename_chr(const char *name, int add_chr, char *buf, size_t bufsz)
{
    if (!add_chr) return name;
    if (strncmp(name, "GL", 2) == 0) return NULL;
    if (strcasecmp(name, "MT") == 0) return "chrM";
    if (strncmp(name, "chr", 3) != 0) {
        snprintf(buf, bufsz, "chr%s", name);
        return buf;
    }
    return name;
}

/* generic.c:781-801 for one reference name of a BAM header: its chromosome in the size file, -1 when it is not there (or its
 * size reads as "not found": generic.c:796-797), -2 when -C drops it */
static int32_t chrom_of_target(const char *target, const run_opts *o, const sizes_t *chr_sizes)
{
    char buf[4096];
    const char *nm = rename_chr(target, o->add_chr, buf, sizeof buf);
    if (!nm) return -2;
    const int64_t id = names_find(&chr_sizes->names, nm);
    return (id >= 0 && (int)chr_sizes->value[id] != 2) ? (int32_t)id : -1;
}

/* ---- records parsed AHEAD of the table -------------------------------------------------------------------------------
 * The engine cannot take records before the table is on the device, and the ring of windows holds 0.1 s of decode: the decoder
 * used to sit idle for the rest of the rmsk parse and the table build. Now the helper thread goes on after it has opened the
 * first file: it parses the windows as they come, keeps their records in a backlog in HBM (include/iteres_amd.h itx_backlog_*:
 * 14 bytes per record instead of the 220 of the inflated stream) and lets the windows go back to the decoder. run_stream
 * submits the backlog first, in order. Only when nothing per record is the host's business (no -R, no bed files, no name
 * lists), one rank, and only whole windows without XA tags (the veto reads the window's bytes) and without mapped records on
 * chromosomes the size file lacks (their warnings are per record): the first window that does not qualify ends it and is
 * left, untouched, to the loop. ITX_NO_PREFETCH=1 turns it off. */
static const run_opts *pre_opts;
static int pre_filter_mode, pre_allowed;
static const sizes_t *pre_sizes;              /* set when the size file is loaded (stream_sizes_ready) */
static int pre_stop;                           /* run_stream: table and engine are there */
static itx_backlog *pre_bl;
static struct pre_ent { size_t at, n; int paired; } *pre_v;
static size_t pre_n, pre_cap;
static double pre_seconds;
void stream_prefetch_allow(const run_opts *o, int filter_mode, int allowed)
{
    pre_opts = o;
    pre_filter_mode = filter_mode;
    pre_allowed = allowed;
}
void stream_sizes_ready(const sizes_t *chr_sizes) { __atomic_store_n(&pre_sizes, chr_sizes, __ATOMIC_RELEASE); }

/* May this window go to the engine where it lies? Not with XA tags while the veto is on, unless the veto may run on the device
 * too (itx_xaveto_*); not with a mapped record on a chromosome the size file lacks (the warning is per record, in file order). */
static int window_goes_direct(int wfl, const uint8_t *seen, const int32_t *t2c, int nt, int veto_on, int dev_veto)
{
    if (veto_on && (wfl & 2) && !dev_veto) return 0;
    for (int t = 0; t < nt; t++)
        if (seen[t] && t2c[t] == -1) return 0;
    return 1;
}

static void prefetch_records(aln_reader *rd)
{
    const double t0 = now_s();
    const sizes_t *cs = NULL;
    while (!(cs = __atomic_load_n(&pre_sizes, __ATOMIC_ACQUIRE))) {            /* (loaded milliseconds after this thread started) */
        if (__atomic_load_n(&pre_stop, __ATOMIC_ACQUIRE) || now_s() - t0 > 10) return;
        usleep(200);
    }
    const run_opts *o = pre_opts;
    const int nt = aln_n_targets(rd);
    if (nt <= 0) return;
    int32_t *t2c = xmalloc(sizeof(int32_t) * (size_t)nt);
    for (int t = 0; t < nt; t++) t2c[t] = chrom_of_target(aln_target_name(rd, t), o, cs);
    size_t cap = warm_input_bytes / 60 + ((size_t)1 << 20);                     /* no BAM record takes less than that compressed */
    if (cap > ((size_t)160 << 20)) cap = (size_t)160 << 20;
    if (itx_backlog_create(multi_device(), cap, &pre_bl) != ITX_OK) {
        pre_bl = NULL;
        free(t2c);
        return;
    }
    const int veto_on = o->xa_veto && !pre_filter_mode;
    while (!__atomic_load_n(&pre_stop, __ATOMIC_ACQUIRE)) {
        int wfl = 0;
        const uint8_t *seen = NULL;
        if (!aln_device_window(rd, &wfl, &seen)) break;                         /* end of input */
        if (!window_goes_direct(wfl, seen, t2c, nt, veto_on, 0) || aln_device_left(rd) > itx_backlog_room(pre_bl)) break;
        itx_batch db;
        const size_t n = aln_read_batch_device(rd, SIZE_MAX, &db);
        if (n == 0) break;
        size_t at = 0;
        if (itx_backlog_append(pre_bl, &db, n, &at) != ITX_OK) die("records parsed ahead: %s", itx_last_error());
        if (pre_n == pre_cap) {
            pre_cap = pre_cap ? pre_cap * 2 : 64;
            pre_v = xrealloc(pre_v, sizeof *pre_v * pre_cap);
        }
        pre_v[pre_n].at = at;
        pre_v[pre_n].n = n;
        pre_v[pre_n].paired = db.mpos != NULL;
        pre_n++;
    }
    free(t2c);
    pre_seconds = now_s() - t0;
}

/* Page-locks the reader's chunk buffers, one after the other, from the moment the HIP runtime is up (0.1 s each for 384 MB):
 * the reader thread used to lock the third to fifth itself when it first needed them — 0.3 s during which the pipeline of
 * pushes crawled (one window decoded in the first 0.34 s). */
static size_t pin_want;
static int pin_count;
static void *pin_main(void *arg)
{
    (void)arg;
    for (int i = 0; i < pin_count && i < POOL_N; i++) {
        void *p = itx_pinned_alloc(pin_want);
        pthread_mutex_lock(&pool_mu);
        pool[i].p = p;
        pool[i].cap = p ? pin_want : 0;
        pool[i].used = 0;
        pool_pinning--;
        pthread_cond_broadcast(&pool_cv);
        pthread_mutex_unlock(&pool_mu);
    }
    pthread_mutex_lock(&pool_mu);
    pool_pinning = 0;
    pthread_cond_broadcast(&pool_cv);
    pthread_mutex_unlock(&pool_mu);
    return NULL;
}

static void *warm_main(void *arg)
{
    (void)arg;
    const double a = now_s();
    const int ndev = itx_device_count();
    const double b = now_s();
    if (ndev > 0) exchange_comm_early();                                 /* a multi-rank job: the communicator is made beside the scan */
    double t_created = b, t_pinned = b;
    int inf_rc = ITX_OK;
    /* the compressed chunks the reader rotates through are page-locked, which takes its time (0.1 - 0.2 s for the first two): a
     * thread of its own locks them while this one makes the inflater's streams; the others are locked by the reader thread when
     * it first needs them, beside the device's work */
    const char *ce = getenv("ITX_BGZF_CHUNK");
    const size_t chunk = ce && atol(ce) >= 1 ? (size_t)atol(ce) : ALN_DEVICE_CHUNK;
    size_t step = chunk;
    pthread_t pin_th;
    int pin_on = 0;
    if (ndev > 0 && warm_bam && !getenv("ITX_HOST_INFLATE")) {
        use_device_reader();                                             /* (aln_raw_step asks which decoder is in use; the inflater itself follows) */
        /* what the reader will ask for: a step's bytes plus room for a carried-over block; a small input gets small buffers */
        const size_t mine_bytes = warm_input_bytes ? warm_input_bytes / (size_t)(multi_world() > 0 ? multi_world() : 1) : 0;
        step = mine_bytes && !ce ? aln_raw_step(mine_bytes + mine_bytes / 64) : chunk;
        pin_want = step + (1u << 17);
        /* as many as a file of this size makes the reader use */
        pin_count = warm_input_bytes ? (int)(mine_bytes / step + 1) : 2;
        if (pin_count > ALN_DEVICE_RAW_BUFFERS) pin_count = ALN_DEVICE_RAW_BUFFERS;
        if (getenv("ITX_PIN_EARLY") && atoi(getenv("ITX_PIN_EARLY")) >= 1 && atoi(getenv("ITX_PIN_EARLY")) < pin_count) pin_count = atoi(getenv("ITX_PIN_EARLY"));   /* (A/B) */
        pool_pinning = pin_count;
        pin_on = pthread_create(&pin_th, NULL, pin_main, NULL) == 0;
        if (!pin_on) pool_pinning = 0;
    }
    if (ndev > 0 && warm_bam && !getenv("ITX_HOST_INFLATE") && (inf_rc = itx_inflater_create(multi_device(), &g_inflater)) != ITX_OK)
        snprintf(warm_err, sizeof warm_err, "%s", itx_last_error());
    else if (ndev <= 0)
        snprintf(warm_err, sizeof warm_err, "no usable GPU (%s)", itx_last_error());
    t_created = now_s();
    if (!pin_on && g_inflater) {
        pin_count = 2;
        pool_pinning = 2;
        pin_main(NULL);
    }
    t_pinned = now_s();
    if (!g_inflater) aln_use_device(NULL);                              /* it did not come up: the host decodes (run_stream says why when that will not do) */
    if (g_inflater) {
        /* the device side of the decoder, all of it, now that nothing runs there yet: windows and per-push scratch sized for
         * the most a push may carry (the block indexer cuts a chunk that inflates to more into two pushes) */
        const char *be = getenv("ITX_DEV_WINDOW_BLOCKS");
        const char *me = getenv("ITX_RESERVE_BLOCKS");                   /* scratch experiments */
        size_t max_blocks = be && atol(be) >= 1 ? (size_t)atol(be) : me && atol(me) >= 64 ? (size_t)atol(me) : 12288;
        /* no more than this rank's share of the input can need: a small file gets small buffers (a block of a real BAM takes
         * kilobytes; a file of smaller ones is simply cut into more pushes by the indexer) */
        if (warm_input_bytes) {
            const size_t mine = warm_input_bytes / (size_t)(multi_world() > 0 ? multi_world() : 1);
            const size_t est = mine / 2048 + 64;
            if (!be && est < max_blocks) max_blocks = est;
            const size_t nchunks = mine / chunk + 3;
            if (nchunks < ITX_BAMWIN_WINDOWS) g_dev_windows = (int)nchunks;          /* in: the most this input can use */
        }
        /* The ring the pushes rotate through: the pushes in flight plus four windows for the consumer. A deeper ring
         * (round 2: up to 48 windows, 50 GB of HBM for a 23 GB file) only let the decoder run ahead while the table was still
         * being built, and paid for it in device allocation time — seconds on a box whose memory the driver had yet to clear;
         * measured on 200 M reads: 8 windows 2.27 - 2.35 s per run, 48 windows 2.37 - 2.58 s. ITX_RESERVE_WINDOWS overrides. */
        {
            const char *we = getenv("ITX_RESERVE_WINDOWS");
            const char *pe = getenv("ITX_PUSHES");
            const int lanes = pe && atoi(pe) >= 1 && atoi(pe) <= ITX_BAMWIN_LANES ? atoi(pe) : ITX_BAMWIN_LANES_DEFAULT;
            const int ring = we && atol(we) >= 2 && atol(we) <= ITX_BAMWIN_WINDOWS ? (int)atol(we) : lanes + 4;
            if (g_dev_windows < 1 || g_dev_windows > ring) g_dev_windows = ring;
        }
        const size_t max_bytes = max_blocks * 65280u < ((size_t)1 << 30) ? max_blocks * 65280u : (size_t)1 << 30;
        if (!getenv("ITX_NO_RESERVE") && itx_inflater_reserve(g_inflater, step + (1u << 17), max_blocks, max_bytes, &g_dev_windows) == ITX_OK) {
            g_dev_max_blocks = max_blocks;
            g_dev_max_bytes = max_bytes;
        } else {
            g_dev_windows = 0;
        }
    }
    const double c = now_s();
    if (g_inflater && warm_first) {
        /* the first file's header, and its first windows decoded while the main thread is still parsing the rmsk file; a
         * file that does not open is left to run_stream, which reports it where the reference does */
        use_device_reader();
        share_t sh0;
        char *one[1] = {warm_first};
        /* this rank's share of the FIRST file when the list has one file (the common case); longer lists are opened by the loop */
        if (multi_world() <= 1) {
            warm_reader = aln_open(warm_first, 0);
        } else if (warm_single && plan_shares(one, 1, warm_splittable, multi_rank(), multi_world(), multi_min_share(), &sh0) && sh0.lo != sh0.hi) {
            warm_reader = aln_open_range(warm_first, sh0.lo, sh0.hi);
            warm_lo = sh0.lo;
            warm_hi = sh0.hi;
        }
        if (warm_reader) aln_readahead(warm_reader);
    }
    const double t_opened = now_s();
    if (getenv("ITX_TIMING"))
        fprintf(stderr, "[itx timing] HIP runtime start-up %.3f s, device inflater + page-locked buffers %.3f s (streams %.3f, page-locked %.3f, device reserve %.3f), first file opened %.3f s (helper thread)\n", b - a,
                c - b, t_created - b, t_pinned - t_created, c - t_pinned, t_opened - c);
    {
        const char *me = getenv("ITX_PREFETCH_MIN");                       /* bytes of input below which it is not worth a backlog (tests: 0) */
        const size_t min_bytes = me ? (size_t)atoll(me) : (size_t)1 << 30;
        if (warm_reader && pre_allowed && pre_opts && multi_world() <= 1 && warm_input_bytes >= min_bytes && !getenv("ITX_NO_PREFETCH")) prefetch_records(warm_reader);
    }
    if (pin_on) pthread_join(pin_th, NULL);                              /* (long done: it started when the runtime came up) */
    return NULL;
}
void gpu_warmup_start(int bam_input, const char *aln_arg, int multi_file, int splittable)
{
    warm_bam = bam_input;
    warm_splittable = splittable;
    if (bam_input && aln_arg) {
        warm_first = xstrdup(aln_arg);
        char *c = multi_file ? strchr(warm_first, ',') : NULL;
        warm_single = c == NULL;
        if (c) *c = 0;
        char *all = xstrdup(aln_arg), *save = NULL;
        warm_input_bytes = 0;
        for (char *tok = multi_file ? strtok_r(all, ",", &save) : all; tok; tok = multi_file ? strtok_r(NULL, ",", &save) : NULL) {
            struct stat sb;
            if (stat(tok, &sb) == 0 && S_ISREG(sb.st_mode)) warm_input_bytes += (size_t)sb.st_size;
            else {
                warm_input_bytes = 0;                                   /* a pipe: no idea */
                break;
            }
        }
        free(all);
    }
    if (!warm_on && pthread_create(&warm_thread, NULL, warm_main, NULL) == 0) warm_on = 1;
}
static void gpu_warmup_join(void)
{
    if (warm_on) pthread_join(warm_thread, NULL);
    warm_on = 0;
}

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
    /* filter -G (csrc/itx_gcov.hip): every counted record adds its interval to the coverage on the device, whatever route it took;
     * the host route derives the intervals of its own records (collect_gcov). The files are written after the stream
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

/* -R on the device: every window, right after its records are parsed (aln_set_window_hook) */
static void dedup_window(void *ctx, size_t n_rec)
{
    (void)n_rec;
    stream_run *r = ctx;
    const double t0 = now_s();
    chk(itx_bamwin_dedup(g_inflater, r->dd), "itx_bamwin_dedup");
    r->t_dedup += now_s() - t0;
}

static void bed_write_out(stream_run *r, int discard)
{
    itx_bed_text tx;
    chk(itx_bed_collect(r->bd, &tx), "itx_bed_collect");
    r->bed_pending--;
    if (discard) return;
    if (r->bed_f && tx.all_bytes && fwrite(tx.all, 1, tx.all_bytes, r->bed_f) != tx.all_bytes) die("writing the bed file: %s", strerror(errno));
    if (r->bed_uniq_f && tx.uniq_bytes && fwrite(tx.uniq, 1, tx.uniq_bytes, r->bed_uniq_f) != tx.uniq_bytes)
        die("writing the unique bed file: %s", strerror(errno));
}

/* filter -r on the device (csrc/itx_names.hip): the lists are gathered where the records lie; what the host route reads goes to
 * the same pool, in stream order (itx_names_append_host), so the end of the stream has one list to sort whatever route a window
 * took. The host route (ITX_HOST_NAMES=1), SAM text and the host decoder keep the lists on the host as before. */
static itx_names *g_names;
/* Which route builds the lists when ITX_HOST_NAMES is not set. The device route becomes the default only on a measurement of the
 * whole command ("Read lists on the device"); until one exists the host builds them, as before. ITX_HOST_NAMES=0 asks
 * for the device route, ITX_HOST_NAMES=1 for the host's. */
#define NAMES_HOST_DEFAULT 1
static int names_by_host(void)
{
    const char *e = getenv("ITX_HOST_NAMES");
    return e && *e ? atoi(e) != 0 : NAMES_HOST_DEFAULT;
}
static const uint32_t *g_names_cnt;                                   /* after the stream: names per row (stream_names_counts) */

const uint32_t *stream_names_counts(void) { return g_names_cnt; }
void stream_names_free(char **locus_names)
{
    free(locus_names);                                                 /* (the strings are the names object's one text) */
    itx_names_destroy(g_names);
    g_names = NULL;
    g_names_cnt = NULL;
}

/* the batch's hits to the device pool: (row, name) in record order */
static void names_to_device(stream_run *r, int k)
{
    const itx_staging *st = &r->st[k];
    aln_side *side = &r->side[k];
    size_t m = 0, b = 0, n = r->pend[k];
    if (r->nbuf.cap_n < n + 1) {
        r->nbuf.cap_n = n + n / 4 + 1;
        r->nbuf.rows = xrealloc(r->nbuf.rows, sizeof(uint32_t) * r->nbuf.cap_n);
        r->nbuf.off = xrealloc(r->nbuf.off, sizeof(uint64_t) * (r->nbuf.cap_n + 1));
    }
    for (size_t i = 0; i < n; i++) {
        if (st->hit_row[i] >= 0) {
            const size_t len = strlen(side->qname[i]);
            if (r->nbuf.cap_b < b + len + 1) {
                r->nbuf.cap_b = (b + len + 1) * 2;
                r->nbuf.bytes = xrealloc(r->nbuf.bytes, r->nbuf.cap_b);
            }
            r->nbuf.rows[m] = (uint32_t)st->hit_row[i];
            r->nbuf.off[m++] = b;
            memcpy(r->nbuf.bytes + b, side->qname[i], len);
            b += len;
        }
        free(side->qname[i]);
        side->qname[i] = NULL;
    }
    r->nbuf.off[m] = b;
    chk(itx_names_append_host(r->nm, r->nbuf.rows, r->nbuf.bytes, r->nbuf.off, m), "itx_names_append_host");
}

/* filter -r: keep the names of the records of slot k that chose a row, free the others */
static void collect_names(stream_run *r, int k)
{
    const itx_staging *st = &r->st[k];
    aln_side *side = &r->side[k];
    r->names_host_batches++;
    if (r->nm) {
        names_to_device(r, k);
        return;
    }
    for (size_t i = 0; i < r->pend[k]; i++) {
        const int32_t row = st->hit_row[i];
        if (row >= 0) {
            if (r->hn.n == r->hn.cap) {
                r->hn.cap = r->hn.cap ? r->hn.cap * 2 : 1 << 16;
                r->hn.v = xrealloc(r->hn.v, sizeof *r->hn.v * r->hn.cap);
            }
            r->hn.v[r->hn.n].row = (uint32_t)row;
            r->hn.v[r->hn.n].name = side->qname[i];
            r->hn.n++;
        } else {
            free(side->qname[i]);
        }
        side->qname[i] = NULL;
    }
}

/* filter -b: the members of the batches that wait (all but the newest `keep`) are fetched and written, oldest first */
static void bam_write_out(stream_run *r, int keep)
{
    while (itx_bamout_pending(r->bo) > keep) {
        itx_bamout_members m;
        chk(itx_bamout_collect(r->bo, &m), "itx_bamout_collect");
        if (m.len && fwrite(m.bytes, 1, m.len, r->bam_f) != m.len) die("writing %s: %s", r->o->bam_out_path, strerror(errno));
    }
}

/* filter -b -i: the index is built beside the stream (csrc/itx_bamidx.hip). The reference lengths of the kept header size its linear
 * part; the first record member starts where the header's members end. */
static void bam_index_begin(stream_run *r, const uint8_t *hb, size_t hl)
{
    int32_t l_text = 0, n_ref = 0;
    size_t at = 8;
    if (hl >= 8) memcpy(&l_text, hb + 4, 4);
    if (hl < 12 || l_text < 0 || (size_t)l_text > hl - 12) die("%s: the kept BAM header is cut short", r->o->bam_out_path);
    at += (size_t)l_text;
    memcpy(&n_ref, hb + at, 4);
    at += 4;
    if (n_ref < 0) die("%s: the kept BAM header names %d references", r->o->bam_out_path, n_ref);
    int32_t *l_ref = xcalloc((size_t)n_ref + 1, sizeof(int32_t));
    for (int32_t k = 0; k < n_ref; k++) {
        int32_t l_name = 0;
        if (hl - at >= 4) memcpy(&l_name, hb + at, 4);
        if (hl - at < 4 || l_name < 0 || (size_t)l_name + 8 > hl - at) die("%s: the kept BAM header is cut short", r->o->bam_out_path);
        memcpy(&l_ref[k], hb + at + 4 + (size_t)l_name, 4);
        at += 8 + (size_t)l_name;
    }
    chk(itx_bamout_index_enable(r->bo, n_ref, l_ref), "itx_bamout_index_enable");
    free(l_ref);
    const long first = ftell(r->bam_f);
    if (first < 0) die("%s: %s", r->o->bam_out_path, strerror(errno));
    r->bam_first = (uint64_t)first;
}

/* filter -b -a: the device's gather gets the rows and the names the tags are made of (csrc/itx_reptag.h); names of 2^16 bytes and
 * more are refused there */
static void bam_annotate_begin(stream_run *r)
{
    const rmsk_t *rm = r->rm;
    const names_t *tabs[3] = {&rm->reps, &rm->clas, &rm->fams};
    char *nb[3];
    uint64_t *no[3];
    for (int t = 0; t < 3; t++) loci_name_table(tabs[t], &nb[t], &no[t]);
    chk(itx_bamout_annotate_enable(r->bo, rm->rows, rm->n_rows, nb[0], no[0], rm->reps.n, nb[1], no[1], rm->clas.n, nb[2], no[2], rm->fams.n), "itx_bamout_annotate_enable");
    for (int t = 0; t < 3; t++) {
        free(nb[t]);
        free(no[t]);
    }
}

/* filter -b -s: the kept header (magic, l_text, text, reference list) with the text the sorted file carries (csrc/itx_bamsortrule.h);
 * l_text follows the new length, the reference list is untouched. The caller frees the result. */
static uint8_t *bam_sorted_header(const stream_run *r, const uint8_t *hb, size_t hl, size_t *out_len)
{
    int32_t l_text = 0;
    if (hl >= 8) memcpy(&l_text, hb + 4, 4);
    if (hl < 12 || l_text < 0 || (size_t)l_text > hl - 12) die("%s: the kept BAM header is cut short", r->o->bam_out_path);
    uint8_t *nb = xcalloc(hl + ITX_BAMSORT_HEADER_GROWTH, 1);
    const size_t nl = itx_bamsort_header_text((const char *)hb + 8, (size_t)l_text, (char *)nb + 8);
    if (nl > INT32_MAX) die("%s: a header text of %zu bytes", r->o->bam_out_path, nl);
    const int32_t nl32 = (int32_t)nl;
    memcpy(nb, hb, 4);
    memcpy(nb + 4, &nl32, 4);
    memcpy(nb + 8 + nl, hb + 8 + (size_t)l_text, hl - 8 - (size_t)l_text);
    *out_len = hl - (size_t)l_text + nl;
    return nb;
}

/* filter -b -i, after the last members: the finished index is written, or one line says why there is none */
static void bam_index_end(stream_run *r, itx_bamout_index_result *ir)
{
    static const char *const why[] = {"", "the counted records are not in coordinate order", "a record ends beyond 2^29", "a record ends beyond its reference's length in the BAM header",
                                      "the BAM header names 65536 references or more"};
    chk(itx_bamout_index_finish(r->bo, r->bam_first, ir), "itx_bamout_index_finish");
    if (ir->status != 0) {
        fprintf(stderr, "[iteres] no index is written for %s: %s\n", r->o->bam_out_path, ir->status >= 1 && ir->status <= 4 ? why[ir->status] : "unknown reason");
        return;
    }
    char *path = NULL;
    if (asprintf(&path, "%s.bai", r->o->bam_out_path) < 0) die("Preparing output wrong");
    FILE *f = fopen(path, "wb");
    if (!f) die("mustOpen: Can't open %s to write: %s", path, strerror(errno));
    if (fwrite(ir->bytes, 1, ir->len, f) != ir->len || fclose(f) != 0) die("writing %s: %s", path, strerror(errno));
    free(path);
}

/* filter -b: the records of slot k that chose a row, as the reader kept their bytes, to the device's stream in record order.
 * -a: each with the tags of its row behind it, by the rule the device's gather follows (csrc/itx_reptag.h), from the host's own table */
static void collect_bam(stream_run *r, int k)
{
    const itx_staging *st = &r->st[k];
    const aln_side *side = &r->side[k];
    const rmsk_t *rm = r->rm;
    size_t b = 0;
    for (size_t i = 0; i < r->pend[k]; i++) {
        if (st->hit_row[i] < 0) continue;
        uint32_t bs;
        memcpy(&bs, side->raw + side->raw_off[i], 4);
        size_t len = 4 + (size_t)bs;
        ItxRepTag t;
        if (r->o->bam_annotate) {
            if ((size_t)st->hit_row[i] >= rm->n_rows) die("filter -b -a: a record chose row %d of %zu", st->hit_row[i], rm->n_rows);
            const itx_row *row = &rm->rows[st->hit_row[i]];
            const char *rep = rm->reps.name[row->rep], *cla = rm->clas.name[row->cla], *fam = rm->fams.name[row->fam];
            t.rep = (const uint8_t *)rep, t.cla = (const uint8_t *)cla, t.fam = (const uint8_t *)fam;
            t.rep_len = (uint32_t)strlen(rep), t.cla_len = (uint32_t)strlen(cla), t.fam_len = (uint32_t)strlen(fam);
            t.start = row->start, t.end = row->end;
            if (len + itx_reptag_len(&t) >= 0x40000000u) die("filter -b -a: a record of %zu bytes with its tags", len + itx_reptag_len(&t));
            len += itx_reptag_len(&t);
            r->bam_host_tag_bytes += itx_reptag_len(&t);
        }
        if (r->bbuf.cap < b + len) {
            r->bbuf.cap = (b + len) * 2;
            r->bbuf.bytes = xrealloc(r->bbuf.bytes, r->bbuf.cap);
        }
        if (r->o->bam_annotate) itx_reptag_write(side->raw + side->raw_off[i], 4u + bs, &t, 0u, (uint32_t)len, r->bbuf.bytes + b);
        else memcpy(r->bbuf.bytes + b, side->raw + side->raw_off[i], len);
        b += len;
    }
    r->bam_host_batches++;
    chk(itx_bamout_append_host(r->bo, r->bbuf.bytes, b), "itx_bamout_append_host");
    bam_write_out(r, 1);
}

/* filter -G: what the stream left on the device for stream_gcov_write, and the batches each route added (ITX_TIMING) */
static itx_gcov *g_gcov;
static unsigned long long g_gcov_dev_batches, g_gcov_host_batches;

/* filter -G: the records of slot k that chose a row add the interval the lookup ran on (host_derive: itx_derive of
 * ../csrc/itx_derive.h). One that has none, which no counted record is, goes up with no chromosome and is counted as out of range. */
static void collect_gcov(stream_run *r, int k)
{
    const itx_staging *st = &r->st[k];
    const stream_file *f = r->cur;
    const size_t n = r->pend[k];
    size_t m = 0;
    if (r->gbuf.cap < n) {
        r->gbuf.cap = n + n / 4 + 1;
        r->gbuf.chrom = xrealloc(r->gbuf.chrom, sizeof(int32_t) * r->gbuf.cap);
        r->gbuf.start = xrealloc(r->gbuf.start, sizeof(uint32_t) * r->gbuf.cap);
        r->gbuf.end = xrealloc(r->gbuf.end, sizeof(uint32_t) * r->gbuf.cap);
        r->gbuf.uniq = xrealloc(r->gbuf.uniq, r->gbuf.cap);
    }
    for (size_t i = 0; i < n; i++) {
        if (st->hit_row[i] < 0) continue;
        const int32_t t = st->tid[i];
        const int32_t chrom = (f && t >= 0 && t < f->nt) ? f->t2c[t] : -1;
        host_iv iv = {0, 0, '+'};
        const int ok = host_derive(r->o, chrom, chrom >= 0 ? r->chr_sizes->value[chrom] : 0, st->flag5[i], st->pos[i], st->tmpend[i], st->mpos[i], st->isize[i], &iv);
        r->gbuf.chrom[m] = ok ? chrom : -1;
        r->gbuf.start[m] = iv.start;
        r->gbuf.end[m] = iv.end;
        r->gbuf.uniq[m] = st->mapq[i] >= r->o->mapq;
        m++;
    }
    g_gcov_host_batches++;
    chk(itx_gcov_add_host(r->gc, r->gbuf.chrom, r->gbuf.start, r->gbuf.end, r->gbuf.uniq, m), "itx_gcov_add_host");
}

static void side_release(aln_side *side, size_t n, int keep_qnames)
{
    if (!side->has_strings) return;                /* nothing was stored: the arrays are all NULL as they were */
    side->has_strings = 0;
    for (size_t i = 0; i < n; i++) {
        if (side->want_qnames && !keep_qnames) {
            free(side->qname[i]);
            side->qname[i] = NULL;
        }
        if (side->want_aux) {
            free(side->xa[i]);
            side->xa[i] = NULL;
        }
    }
}

/* wait for host slot k and collect what its previous batch left behind; returns the seconds waited */
static double drain_slot(stream_run *r, int k)
{
    const double t0 = now_s();
    chk(itx_engine_wait_slot(r->eng, k), "itx_engine_wait_slot");
    const double waited = now_s() - t0;
    if (!r->pend[k]) return waited;
    if (r->want_qnames) collect_names(r, k);
    if (r->bo) collect_bam(r, k);
    if (r->gc) collect_gcov(r, k);
    side_release(&r->side[k], r->pend[k], r->want_qnames);
    r->pend[k] = 0;
    return waited;
}
/* both (idle_too: or only those with a batch in flight), the older batch first: the read lists are in file order */
static void drain_slots(stream_run *r, int idle_too)
{
    for (int kk = 0; kk < 2; kk++)
        if (idle_too || r->pend[r->s ^ kk]) drain_slot(r, r->s ^ kk);
}

/* generic.c:760-761 for n records at once */
static void progress_marks(stream_run *r, size_t n)
{
    for (unsigned long long m = (r->ends / r->progress_every + 1) * r->progress_every; m <= r->ends + n; m += r->progress_every)
        fprintf(stderr, "\r* Processed read ends: %llu", m);
    r->ends += n;
}

/* after a multi-GPU stream: the reduced partial (the engine's own buffers) the writers' arrays come from */
static void *g_reduced_u64, *g_reduced_u32;

int stream_finish(itx_engine *eng, const itx_result *res)
{
    if (g_reduced_u64) return itx_engine_finish_partial(eng, g_reduced_u64, g_reduced_u32, res);
    return itx_engine_finish(eng, res);
}

/* ---- the steps of run_stream, in its order ------------------------------------------------------------------------------ */

/* table: every chromosome of the size file is known to the engine (a read may land on one without repeats) */
static void make_table_and_engine(stream_run *r)
{
    const rmsk_t *rm = r->rm;
    const run_opts *o = r->o;
    struct timespec ts0, ts1;
    clock_gettime(CLOCK_MONOTONIC, &ts0);
    int ndev = itx_device_count();
    if (ndev <= 0) die("no usable MI355X (HIP) device: %s", ndev < 0 ? itx_last_error() : "none visible");
    size_t bad = 0;
    int rc = itx_table_create(rm->rows, rm->n_rows, r->chr_sizes->value, (int)r->chr_sizes->names.n, rm->rep_len, rm->reps.n, rm->fams.n, rm->clas.n,
                              multi_device(), &r->tab, &bad);
    if (rc == ITX_E_RANGE) {
        const itx_row *row = &rm->rows[bad];
        die("(%d %d) out of range (%d %d) in binKeeperAdd", (int)row->start, (int)row->end, 0, (int)r->chr_sizes->value[row->chrom]);
    }
    chk(rc, "itx_table_create");
    r->p.mapq_min = o->mapq;
    r->p.min_cov = o->min_cov;
    r->p.extension = o->extension;
    r->p.isize_max = o->isize;
    r->p.treat_pe_as_se = o->treat;
    r->p.discard_half_mapped = o->discard;
    r->p.mode = r->filter_mode ? ITX_MODE_FILTER : ITX_MODE_STAT;
    r->p.accum = ITX_ACCUM_DEFAULT;
    chk(itx_engine_create(r->tab, &r->p, BATCH_RECORDS, &r->eng), "itx_engine_create");
    clock_gettime(CLOCK_MONOTONIC, &ts1);
    if (r->timing) fprintf(stderr, "[itx timing] table build + engine %.3f s\n", (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec));
}

static void open_outputs_and_side_buffers(stream_run *r)
{
    const run_opts *o = r->o;
    for (int k = 0; k < 2; k++) {
        r->side[k].want_qnames = r->want_qnames || r->want_bed;
        r->side[k].want_aux = r->veto_on || o->bed_path != NULL;
        if (r->side[k].want_qnames) r->side[k].qname = xcalloc(BATCH_RECORDS, sizeof(char *));
        r->side[k].want_raw = o->bam_out_path != NULL;
        if (r->side[k].want_raw) r->side[k].raw_off = xcalloc(BATCH_RECORDS, sizeof(size_t));
        if (r->side[k].want_aux) {
            r->side[k].xa = xcalloc(BATCH_RECORDS, sizeof(char *));
            r->side[k].nm = xcalloc(BATCH_RECORDS, sizeof(int32_t));
        }
    }
    r->any_side = r->side[0].want_qnames || r->side[0].want_aux || r->side[0].want_raw;
    if (o->dedup || r->want_bed || r->veto_on) {
        r->iv = xcalloc(BATCH_RECORDS, sizeof *r->iv);
        r->live = xcalloc(BATCH_RECORDS, 1);
    }
    names_init(&r->chr_names);
    names_init(&r->warned);
    /* mustOpen, cuskent/common.c:2543-2568 */
    if (o->bed_path && !(r->bed_f = fopen(o->bed_path, "w"))) die("mustOpen: Can't open %s to write: %s", o->bed_path, strerror(errno));
    if (o->bed_uniq_path && !(r->bed_uniq_f = fopen(o->bed_uniq_path, "w")))
        die("mustOpen: Can't open %s to write: %s", o->bed_uniq_path, strerror(errno));
    if (o->bam_out_path && !(r->bam_f = fopen(o->bam_out_path, "wb"))) die("mustOpen: Can't open %s to write: %s", o->bam_out_path, strerror(errno));
}

/* the list of files (stat: comma separated, generic.c:725; filter: one file) and this rank's share of every one */
static void list_files_and_shares(stream_run *r)
{
    r->arg = xstrdup(r->o->aln_arg);
    if (r->multi_file) {
        for (char *s = r->arg; r->n_files < 100;) {
            r->files[r->n_files++] = s;
            char *c = strchr(s, ',');
            if (!c) break;
            *c = 0;
            s = c + 1;
        }
    } else {
        r->files[r->n_files++] = r->arg;
    }
    r->shared = plan_shares(r->files, r->n_files, warm_splittable && !getenv("ITX_HOST_INFLATE"), multi_rank(), multi_world(), multi_min_share(), r->share) &&
                multi_world() > 1;
}

/* the helper thread (HIP start-up, device decoder, first file opened and decoding ahead) has had the rmsk parse and the table
 * build to finish */
static void join_helper_thread(stream_run *r)
{
    const double t_join = now_s();
    if (getenv("ITX_PREFETCH_HOLD_MS")) usleep((useconds_t)atol(getenv("ITX_PREFETCH_HOLD_MS")) * 1000u);     /* tests: a table that takes its time */
    __atomic_store_n(&pre_stop, 1, __ATOMIC_RELEASE);                  /* table and engine are there: the helper thread finishes the window it is at */
    gpu_warmup_join();
    if (r->timing) fprintf(stderr, "[itx timing] waited %.3f s for the helper thread\n", now_s() - t_join);
    if (g_inflater) use_device_reader();
}

/* -R: one set over all files, like `dup` (generic.c:721). BAM decoded on the device: the set lives there too
 * (csrc/itx_dedup.hip) and marks a window's duplicates where the window lies, right after it is parsed; SAM text, the host
 * decoder and ITX_HOST_DEDUP=1: the host's hash set, record by record */
static void choose_dedup_set(stream_run *r)
{
    const run_opts *o = r->o;
    if (o->dedup && g_inflater && !o->is_sam && !getenv("ITX_HOST_DEDUP")) {
        size_t cells = warm_input_bytes / 24;                          /* a first guess at the keys to come; the table grows */
        if (cells < ((size_t)1 << 20)) cells = (size_t)1 << 20;
        if (cells > ((size_t)1 << 28)) cells = (size_t)1 << 28;
        chk(itx_dedup_create(multi_device(), r->chr_sizes->value, (int)r->chr_sizes->names.n, &r->p, cells, &r->dd), "itx_dedup_create");
    }
    r->dups = o->dedup && !r->dd ? dup_set_new() : NULL;
    if (r->shared && !g_inflater) die("rank %d: the device decoder did not come up: %s", multi_rank(), warm_err[0] ? warm_err : itx_last_error());
}

/* ---- per file: open, tid maps, backlog ------------------------------------------------------------------------------------ */

/* SAM text: the route. ITX_HOST_SAM=1 the host's line parser, =0 the device's kernels (csrc/itx_samtext.hip); unset: the host,
 * until a measurement at size says otherwise (DESIGN.md "SAM text on the device"). */
static int sam_by_device(void)
{
    const char *e = getenv("ITX_HOST_SAM");
    return e && atoi(e) == 0;
}

/* the device object for one SAM file, made from the reader's reference names and attached before the first batch is read */
static itx_samtext *sam_device_attach(aln_reader *rd)
{
    const int nt = aln_n_targets(rd);
    size_t bytes = 0;
    for (int t = 0; t < nt; t++) bytes += strlen(aln_target_name(rd, t));
    char *pool = xmalloc(bytes + 1);
    uint64_t *off = xmalloc(sizeof(uint64_t) * ((size_t)nt + 1));
    size_t at = 0;
    for (int t = 0; t < nt; t++) {
        const size_t k = strlen(aln_target_name(rd, t));
        off[t] = at;
        memcpy(pool + at, aln_target_name(rd, t), k);
        at += k;
    }
    off[nt] = at;
    itx_samtext *x = NULL;
    /* room for a chunk of text; for BGZF, whose chunks end with a whole member, 64 KiB more and the tail of the chunk before */
    size_t room = aln_sam_chunk_bytes() + 65536 + ALN_SAM_CARRY;
    if (room > (size_t)256 << 20) room = (size_t)256 << 20;              /* the most an object takes: a longer text is the host's */
    chk(itx_samtext_create(multi_device(), pool, off, nt, room, &x), "itx_samtext_create");
    free(pool);
    free(off);
    const aln_sam_device d = {x, itx_samtext_parse_begin, itx_samtext_parse_end, itx_samtext_fetch, itx_pinned_alloc, itx_pinned_free, itx_last_error,
                              itx_samtext_parse_begin_bgzf, itx_samtext_bgzf_info, itx_samtext_text, itx_samtext_strings};
    aln_set_sam_device(rd, &d);
    return x;
}

/* 1: the reader is the helper thread's, with records parsed ahead of the table to submit first */
static int open_file(stream_run *r, stream_file *f, int fi, int pass)
{
    const run_opts *o = r->o;
    const share_t *sh = &r->share[fi];
    int backlog = 0;
    f->t_open0 = now_s();
    if (fi == 0 && pass == 0 && warm_reader && warm_first && strcmp(r->files[0], warm_first) == 0 && warm_lo == sh->lo && warm_hi == sh->hi) {
        f->rd = warm_reader;                                             /* opened and decoding since the helper thread came up */
        warm_reader = NULL;
        backlog = pre_bl != NULL;
    } else {
        if (warm_reader && fi == 0 && pass == 0) {                       /* opened for another share than this plan's: not used */
            aln_close(warm_reader);
            warm_reader = NULL;
        }
        f->rd = (sh->lo == 0 && sh->hi == SIZE_MAX) ? aln_open(r->files[fi], o->is_sam) : aln_open_range(r->files[fi], sh->lo, sh->hi);
    }
    f->t_opened = now_s();
    if (!f->rd) {
        fprintf(stderr, "Fail to open %s file %s\n", o->is_sam ? "SAM" : "BAM", o->aln_arg);
        die("Error\n");
    }
    return backlog;
}

/* The engine and the side objects learn the current file's header: at the top of a file all that exist (only == NULL), after a
 * late creation the new one. */
static void attach_tidmaps(stream_run *r, stream_file *f, const void *only)
{
    const int nt = f->nt > 0 ? f->nt : 0;
    if (!only) chk(itx_engine_set_tidmap(r->eng, f->t2c, nt), "itx_engine_set_tidmap");
    if (r->xv && (!only || only == r->xv)) chk(itx_xaveto_set_tidmap(r->xv, f->t2c, nt), "itx_xaveto_set_tidmap");
    if (r->gc && !only) chk(itx_gcov_set_tidmap(r->gc, f->t2c, nt), "itx_gcov_set_tidmap");
    if (r->bd && (!only || only == r->bd)) chk(itx_bed_set_tidmap(r->bd, f->t2c, (const char *const *)f->t2name, nt), "itx_bed_set_tidmap");
    if (r->dd && !only) {
        chk(itx_dedup_set_tidmap(r->dd, f->t2c, f->t2id, nt), "itx_dedup_set_tidmap");
        aln_set_window_hook(f->rd, dedup_window, r);
    }
    if (!only && f->nt == 0) {
        /* no references: nothing can map; still count the read ends */
        int32_t none = -1;
        chk(itx_engine_set_tidmap(r->eng, &none, 1), "itx_engine_set_tidmap");
    }
}

/* The side objects of the device route are made when first needed: the veto object must not be built for inputs without XA tags. */
static void create_bed(stream_run *r, stream_file *f)
{
    chk(itx_bed_create(multi_device(), r->chr_sizes->value, (int)r->chr_sizes->names.n, &r->p, (r->bed_f ? ITX_BED_ALL : 0) | (r->bed_uniq_f ? ITX_BED_UNIQ : 0),
                       BATCH_RECORDS, &r->bd),
        "itx_bed_create");
    attach_tidmaps(r, f, r->bd);
}
static void create_xaveto(stream_run *r, stream_file *f)
{
    const rmsk_t *rm = r->rm;
    uint32_t *row_rep = xmalloc(sizeof(uint32_t) * (rm->n_rows + 1)), *words = xa_rep_words(rm);
    for (size_t i = 0; i < rm->n_rows; i++) row_rep[i] = rm->rows[i].rep;
    chk(itx_xaveto_create(r->tab, &r->p, row_rep, words, (const char *const *)r->chr_sizes->names.name, (int)r->chr_sizes->names.n, BATCH_RECORDS, &r->xv),
        "itx_xaveto_create");
    attach_tidmaps(r, f, r->xv);
    free(row_rep);
    free(words);
}

/* the header's references against the size file, and which routes this file may take */
static void map_targets(stream_run *r, stream_file *f)
{
    const run_opts *o = r->o;
    const int nt = f->nt = aln_n_targets(f->rd);
    f->t2c = xmalloc(sizeof(int32_t) * (size_t)(nt + 1));
    f->t2id = xcalloc((size_t)nt + 1, sizeof(uint32_t));
    f->t2name = xcalloc((size_t)nt + 1, sizeof(char *));
    for (int t = 0; t < nt; t++) {
        char buf[4096];
        const char *nm = rename_chr(aln_target_name(f->rd, t), o->add_chr, buf, sizeof buf);
        f->t2name[t] = nm ? xstrdup(nm) : NULL;
        if (!nm) {
            f->t2c[t] = -2;
        } else {
            /* generic.c:796-797: cend = size-1 with 2 as the "not found" default; a listed size of 2 reads the same */
            f->t2c[t] = chrom_of_target(aln_target_name(f->rd, t), o, r->chr_sizes);
            if (r->dups || r->dd) f->t2id[t] = names_intern(&r->chr_names, nm);
        }
    }
    attach_tidmaps(r, f, NULL);
    /* Nothing per record is the host's business when no option asks for names, -R or bed lines: a window of records the
     * device decoder parsed then goes to the engine where it lies, in HBM (window_goes_direct says which). The bed lines do
     * not keep a window on the host: the device decoder's windows get their text built where they lie (ITX_HOST_BED=1: by the
     * host). Nor do the read lists of filter -r on the device route (ITX_HOST_NAMES=0). */
    f->dev_bed = r->want_bed && g_inflater && !o->is_sam && !getenv("ITX_HOST_BED");
    f->dev_names = r->want_qnames && g_inflater && !o->is_sam && !names_by_host();
    f->handoff_ok = !r->dups && (!r->want_bed || f->dev_bed) && (!r->want_qnames || f->dev_names);
    if (f->dev_names && !r->nm) {
        chk(itx_names_create(multi_device(), BATCH_RECORDS, 0, &r->nm), "itx_names_create");
        g_names = r->nm;
    }
    if (f->dev_bed && !r->bd) create_bed(r, f);
    if (r->bam_f && !r->bam_header_done) {
        /* the emitted BAM starts with the input's header as it was read (magic, text, reference list), in members of the host's */
        size_t hl = 0;
        const uint8_t *hb = aln_header_bytes(f->rd, &hl);
        if (!g_inflater || o->is_sam || !hb) die("filter -b needs BAM input decoded on the device: %s", warm_err[0] ? warm_err : "the decoder is not in use");
        uint8_t *sorted_hb = o->bam_sort ? bam_sorted_header(r, hb, hl, &hl) : NULL;
        if (sorted_hb) hb = sorted_hb;
        if (bgzf_write_members(r->bam_f, hb, hl) != 0) die("writing %s: %s", o->bam_out_path, strerror(errno));
        r->bam_header_done = 1;
        chk(itx_bamout_create(multi_device(), BATCH_RECORDS, 0, &r->bo), "itx_bamout_create");
        if (o->bam_level_given) chk(itx_bamout_set_level(r->bo, o->bam_level), "itx_bamout_set_level");
        if (o->bam_sort) chk(itx_bamout_sort_enable(r->bo), "itx_bamout_sort_enable");
        if (o->bam_annotate) bam_annotate_begin(r);
        if (o->bam_index) bam_index_begin(r, hb, hl);
        free(sorted_hb);
    }
}

/* the records the helper thread parsed while the table was being built: first, in file order */
static void submit_backlog(stream_run *r)
{
    const double td = now_s();
    unsigned long long got = 0;
    for (size_t k = 0; k < pre_n; k++)
        for (size_t off = 0; off < pre_v[k].n; off += BATCH_RECORDS) {
            const size_t m = pre_v[k].n - off < BATCH_RECORDS ? pre_v[k].n - off : BATCH_RECORDS;
            itx_batch db;
            chk(itx_backlog_batch(pre_bl, pre_v[k].at + off, pre_v[k].paired, &db), "itx_backlog_batch");
            progress_marks(r, m);
            got += m;
            chk(itx_engine_submit_device_own(r->eng, &db, m, NULL), "itx_engine_submit_device_own");
        }
    chk(itx_engine_wait_own(r->eng), "itx_engine_wait_own");
    if (r->timing)
        fprintf(stderr, "\n[itx timing] parsed ahead of the table by the helper thread: %llu records of %zu windows (%.3f s there), submitted in %.3f s\n", got, pre_n,
                pre_seconds, now_s() - td);
}

/* ---- the record loop: the device route window by window, the host route batch by batch ----------------------------------- */

/* Only the host can read this batch: it and the rest of its window take the host route (the batches before are through).
 * drop_bed: the bed text this batch already started is the host's to print. */
static int host_takes_over(stream_run *r, stream_file *f, size_t n, int drop_bed, double since)
{
    if (drop_bed && r->bd) bed_write_out(r, 1);
    aln_device_rewind(f->rd, n);
    f->t_host += now_s() - since;
    return 0;
}

/* The device route for the window the reader stands at: its batches go to the engine where they lie. Per batch, in the
 * reference's order (generic.c:925 before 972): bed text, names, veto, progress, submit. 1: the window went through; 0: the
 * host route takes over from the current batch. */
static int device_window(stream_run *r, stream_file *f, int xa_window)
{
    int wfl;
    const uint8_t *seen;
    double tq = now_s();
    do {
        itx_batch db;
        const size_t n = aln_read_batch_device(f->rd, BATCH_RECORDS, &db);
        f->t_read += now_s() - tq;
        if (n == 0) break;
        tq = now_s();
        if (r->bd) {
            /* built from the window as -R left it. The batch before this one is written out while this one's kernels run. */
            uint64_t hard = 0;
            if (aln_device_bed(f->rd, r->bd, n, &hard) != 0) die("device bed: %s", itx_last_error());
            if (!hard) r->bed_pending++;
            while (r->bed_pending > (hard ? 0 : 1)) bed_write_out(r, 0);
            if (hard) return host_takes_over(r, f, n, 0, tq);        /* a record only the host can print */
        }
        if (r->nm) {
            /* Classify into the lists' buffer first, gather, and only then submit: a batch whose names only the host can read
             * has then not been counted yet, and the host route counts it once. (filter runs no veto: the rows are final.)
             * What the host route still holds of earlier batches goes to the pool first — the lists are in file order. */
            drain_slots(r, 0);
            uint64_t hard = 0;
            chk(itx_engine_classify_device(r->eng, &db, n, itx_names_hits(r->nm), itx_names_stream(r->nm)), "itx_engine_classify_device");
            if (aln_device_names(f->rd, r->nm, n, itx_names_hits(r->nm), itx_names_stream(r->nm), &hard) != 0) die("device read lists: %s", itx_last_error());
            if (hard) return host_takes_over(r, f, n, 0, tq);
        }
        if (r->bo) {
            /* filter -b, the same order: classify (once for both gatherers when the lists are built here too), gather, submit.
             * The members of the batch before this one are written to the file while this one's kernels run. */
            int32_t *hits = r->nm ? itx_names_hits(r->nm) : itx_bamout_hits(r->bo);
            void *hst = r->nm ? itx_names_stream(r->nm) : itx_bamout_stream(r->bo);
            if (!r->nm) {
                drain_slots(r, 0);
                chk(itx_engine_classify_device(r->eng, &db, n, hits, hst), "itx_engine_classify_device");
            }
            if (aln_device_bamout(f->rd, r->bo, n, hits, hst) != 0) die("device BAM output: %s", itx_last_error());
            r->bam_dev_batches++;
            bam_write_out(r, 1);
        }
        if (r->gc) {
            /* filter -G: the rows the lists or the BAM had classified, else classified into the coverage's own buffer; its kernel
             * follows on the stream they were written on. Sums commute: no order to keep with the host route's batches. */
            const int32_t *hits = r->nm ? itx_names_hits(r->nm) : r->bo ? itx_bamout_hits(r->bo) : itx_gcov_hits(r->gc);
            void *hst = r->nm ? itx_names_stream(r->nm) : r->bo ? itx_bamout_stream(r->bo) : itx_gcov_stream(r->gc);
            if (!r->nm && !r->bo) chk(itx_engine_classify_device(r->eng, &db, n, itx_gcov_hits(r->gc), hst), "itx_engine_classify_device");
            chk(itx_gcov_run(r->gc, &db, hits, n, hst), "itx_gcov_run");
            g_gcov_dev_batches++;
        }
        if (xa_window) {
            /* classify, let the device read the tags of the classified records, mark the vetoed ones */
            uint64_t vetoed = 0, hard = 0;
            chk(itx_engine_classify_device(r->eng, &db, n, itx_xaveto_hits(r->xv), itx_xaveto_stream(r->xv)), "itx_engine_classify_device");
            if (aln_device_xa_veto(f->rd, r->xv, n, &vetoed, &hard) != 0) die("device veto: %s", itx_last_error());
            if (hard) return host_takes_over(r, f, n, 1, tq);        /* an alternative only strtol / the reference's assert can judge */
            if (r->hc) r->hc->diff_subfam += vetoed;
            r->veto_dev_batches++;
        }
        f->t_host += now_s() - tq;
        progress_marks(r, n);
        tq = now_s();
        chk(itx_engine_submit_device_own(r->eng, &db, n, NULL), "itx_engine_submit_device_own");
        /* the window's arrays are the decoder's again once its last batch is through: the next parse overwrites them */
        if (aln_device_left(f->rd) == 0) {
            chk(itx_engine_wait_own(r->eng), "itx_engine_wait_own");
            if (r->bd) chk(itx_bed_wait_kernels(r->bd), "itx_bed_wait_kernels");
            if (r->nm) chk(itx_names_wait_kernels(r->nm), "itx_names_wait_kernels");
            if (r->bo) chk(itx_bamout_wait_kernels(r->bo), "itx_bamout_wait_kernels");
            if (r->gc) chk(itx_gcov_wait_kernels(r->gc), "itx_gcov_wait_kernels");
        }
        f->t_submit += now_s() - tq;
        tq = now_s();
    } while (!aln_device_window(f->rd, &wfl, &seen));                  /* until the next window's start (or the end) */
    return 1;
}

/* generic.c:760-761 progress; generic.c:793-801 one warning per unknown chromosome, in file order. Batches without a mapped
 * record on an unknown chromosome (all of them, for most files) only print the progress marks. */
static void warn_unknown_chromosomes(stream_run *r, const stream_file *f, size_t n)
{
    const int32_t *tidv = r->st[r->s].tid, *t2c = f->t2c;
    const uint8_t *f5 = r->st[r->s].flag5;
    const int nt = f->nt;
    int unknown = 0;
#pragma omp parallel for schedule(static) reduction(| : unknown)
    for (long i = 0; i < (long)n; i++) {
        const int32_t t = tidv[i];
        if (!(f5[i] & 2) && t >= 0 && t < nt && t2c[t] == -1) unknown |= 1;
    }
    if (!unknown) {
        progress_marks(r, n);
        return;
    }
    for (size_t i = 0; i < n; i++) {
        if (++r->ends % r->progress_every == 0) fprintf(stderr, "\r* Processed read ends: %llu", r->ends);
        const int32_t t = tidv[i];
        if (!(f5[i] & 2) && t >= 0 && t < nt && t2c[t] == -1 && names_find(&r->warned, f->t2name[t]) < 0) {
            names_intern(&r->warned, f->t2name[t]);
            warnf("* Warning: read ends mapped to chromosome %s will be discarded as %s not existed in the chromosome size file", f->t2name[t],
                  f->t2name[t]);
        }
    }
}

/* in file order: -R and the bed lines (generic.c:907-936). 1: a live record carries an XA tag */
static int ordered_pass(stream_run *r, const stream_file *f, size_t n)
{
    const run_opts *o = r->o;
    itx_staging *st = &r->st[r->s];
    const aln_side *side = &r->side[r->s];
    host_iv *iv = r->iv;
    int batch_xa = 0;
    if (r->want_bed) r->bed_host_batches++;
    for (size_t i = 0; i < n; i++) {
        const int32_t t = st->tid[i];
        const int32_t chrom = (t >= 0 && t < f->nt) ? f->t2c[t] : -1;
        r->live[i] = 0;
        if (!host_derive(o, chrom, chrom >= 0 ? r->chr_sizes->value[chrom] : 0, st->flag5[i], st->pos[i], st->tmpend[i], st->mpos[i], st->isize[i], &iv[i]))
            continue;
        const int uniq = st->mapq[i] >= o->mapq;
        if (r->dd && (st->flag5[i] & ITX_F5_NOLOOKUP)) continue;          /* a duplicate, marked on the device */
        if (r->dups && dup_set_seen(r->dups, f->t2id[t], &iv[i], uniq)) {
            st->flag5[i] |= ITX_F5_NOLOOKUP;
            if (uniq && r->hc) r->hc->dup_unique++;
            continue;
        }
        r->live[i] = 1;
        const char *xa = side->want_aux ? side->xa[i] : NULL;
        if (xa) batch_xa = 1;
        if (r->bed_f) {
            fprintf(r->bed_f, "%s\t%u\t%u\t%s\t%i\t%c", f->t2name[t], iv[i].start, iv[i].end, side->qname[i], (int)st->mapq[i], iv[i].strand);
            if (xa) fprintf(r->bed_f, "\t%i\t%s", (int)side->nm[i], xa);
            fprintf(r->bed_f, "\n");
        }
        if (r->bed_uniq_f && uniq)
            fprintf(r->bed_uniq_f, "%s\t%u\t%u\t%s\t%i\t%c\n", f->t2name[t], iv[i].start, iv[i].end, side->qname[i], (int)st->mapq[i], iv[i].strand);
    }
    return batch_xa;
}

/* the XA veto needs the chosen row first: classify the slot, look, mark, then count (generic.c:972-982) */
static void veto_pass(stream_run *r, const stream_file *f, size_t n)
{
    itx_staging *st = &r->st[r->s];
    const aln_side *side = &r->side[r->s];
    r->veto_host_batches++;
    if (!r->xi) r->xi = xa_index_new(r->rm);
    chk(itx_engine_classify_slot(r->eng, r->s, n, f->any_paired), "itx_engine_classify_slot");
    chk(itx_engine_wait_slot(r->eng, r->s), "itx_engine_wait_slot");
    unsigned long long vetoed = 0;
#pragma omp parallel for schedule(dynamic, 4096) reduction(+ : vetoed)
    for (long i = 0; i < (long)n; i++) {
        if (!r->live[i] || !side->xa[i] || st->hit_row[i] < 0) continue;
        const uint32_t rep = r->rm->rows[st->hit_row[i]].rep;
        if (xa_veto(r->xi, rep, side->nm[i], side->xa[i], (int)(r->iv[i].end - r->iv[i].start))) {
            st->flag5[i] |= ITX_F5_NOLOOKUP;
            vetoed++;
        }
    }
    if (r->hc) r->hc->diff_subfam += vetoed;
}

/* The host route for one batch: slot s is collected and refilled by the reader, the host's passes run over it in the
 * reference's order (warnings with progress, -R and bed lines, veto), then it is submitted. Returns the records read (0: end). */
static size_t host_batch(stream_run *r, stream_file *f)
{
    const int s = r->s;
    if (!r->have_slots) {
        chk(itx_engine_staging(r->eng, 0, &r->st[0]), "itx_engine_staging");
        chk(itx_engine_staging(r->eng, 1, &r->st[1]), "itx_engine_staging");
        r->have_slots = 1;
    }
    itx_staging *st = &r->st[s];
    aln_side *side = &r->side[s];
    f->t_wait += drain_slot(r, s);
    int aux_xa = 0;                                                    /* per batch */
    double tq = now_s();
    const size_t n = aln_read_batch(f->rd, st, BATCH_RECORDS, r->any_side ? side : NULL, &f->any_paired, &aux_xa);
    f->t_read += now_s() - tq;
    if (n == 0) return 0;
    tq = now_s();
    warn_unknown_chromosomes(r, f, n);
    int batch_xa = 0;
    if (r->dups || r->dd || r->bed_f || r->bed_uniq_f) {
        batch_xa = ordered_pass(r, f, n);
    } else if (r->veto_on && aux_xa) {
        /* only the veto needs the intervals, and only of the records that carry XA: no order involved */
        batch_xa = 1;
#pragma omp parallel for schedule(static)
        for (long i = 0; i < (long)n; i++) {
            r->live[i] = 0;
            if (!side->xa[i] || (st->flag5[i] & ITX_F5_NOLOOKUP)) continue;
            const int32_t t = st->tid[i];
            const int32_t chrom = (t >= 0 && t < f->nt) ? f->t2c[t] : -1;
            r->live[i] = (uint8_t)host_derive(r->o, chrom, chrom >= 0 ? r->chr_sizes->value[chrom] : 0, st->flag5[i], st->pos[i], st->tmpend[i], st->mpos[i],
                                              st->isize[i], &r->iv[i]);
        }
    }
    if (r->veto_on && batch_xa) veto_pass(r, f, n);
    f->t_host += now_s() - tq;
    tq = now_s();
    chk(itx_engine_submit_slot(r->eng, s, n, f->any_paired, r->want_qnames || r->bo != NULL || r->gc != NULL), "itx_engine_submit_slot");
    f->t_submit += now_s() - tq;
    r->pend[s] = n;
    r->s ^= 1;
    return n;
}

/* The dispatcher: the device route when this file may take it and the reader stands at the start of a window that qualifies;
 * else one batch by the host route — which prints and reads only after the pending bed text is written and the names kernels
 * are through. A window the device route gave up continues here, batch by batch, to its end. */
static void record_loop(stream_run *r, stream_file *f)
{
    for (;;) {
        if (f->handoff_ok) {
            int wfl = 0;
            const uint8_t *seen = NULL;
            const double tq = now_s();
            const int direct = aln_device_window(f->rd, &wfl, &seen) && window_goes_direct(wfl, seen, f->t2c, f->nt, r->veto_on, r->dev_veto);
            const int xa_window = r->veto_on && (wfl & 2);
            if (direct && xa_window && !r->xv) create_xaveto(r, f);
            f->t_read += now_s() - tq;
            if (direct && device_window(r, f, xa_window)) continue;
            if (aln_device_exhausted(f->rd)) break;
        }
        while (r->bd && r->bed_pending) bed_write_out(r, 0);
        if (r->nm) chk(itx_names_wait_kernels(r->nm), "itx_names_wait_kernels");
        if (r->bo) chk(itx_bamout_wait_kernels(r->bo), "itx_bamout_wait_kernels");
        if (r->gc) chk(itx_gcov_wait_kernels(r->gc), "itx_gcov_wait_kernels");
        if (host_batch(r, f) == 0) break;
    }
}

static void scan_file(stream_run *r, int fi, int pass)
{
    stream_file f;
    memset(&f, 0, sizeof f);
    if (r->multi_file) fprintf(stderr, "\n* Processing %s\n", r->files[fi]);
    if (r->share[fi].lo == r->share[fi].hi) return;                    /* nothing of this file is this rank's */
    const int backlog = open_file(r, &f, fi, pass);
    itx_samtext *sam_dev = r->o->is_sam && sam_by_device() ? sam_device_attach(f.rd) : NULL;
    r->s = 0;
    r->cur = &f;
    map_targets(r, &f);
    if (backlog) submit_backlog(r);
    if (pre_bl && fi == 0 && pass == 0) {                              /* used or not (another share than the plan's): gone */
        itx_backlog_destroy(pre_bl);
        pre_bl = NULL;
        free(pre_v);
        pre_v = NULL;
        pre_n = pre_cap = 0;
    }
    record_loop(r, &f);
    while (r->bd && r->bed_pending) bed_write_out(r, 0);
    f.t_loop_done = now_s();
    drain_slots(r, 1);                                                 /* before the tid map of the next file replaces this one */
    /* a share of a multi-rank job: the line with the whole job's count comes after the exchange (rank 0's share alone
     * would differ from what the reference prints) */
    if (!r->shared) fprintf(stderr, "\r* Processed read ends: %llu\n", r->ends);
    if (r->timing)
        fprintf(stderr, "[itx timing] stream of %s: decode %.3f s, host passes %.3f s, submit %.3f s, waiting for the device %.3f s\n", r->files[fi], f.t_read,
                f.t_host, f.t_submit, f.t_wait);
    r->cur = NULL;                                                     /* (both slots are drained) */
    for (int t = 0; t < f.nt; t++) free(f.t2name[t]);
    free(f.t2name);
    free(f.t2id);
    free(f.t2c);
    const double t_drained = now_s();
    if (!aln_range_verified(f.rd)) r->boundary_missed++;
    aln_close(f.rd);
    itx_samtext_destroy(sam_dev);                                      /* after the reader, which ends whatever parse is still in flight */
    if (r->timing)
        fprintf(stderr, "[itx timing] open %.3f s, record loop %.3f s, drain %.3f s, close %.3f s\n", f.t_opened - f.t_open0, f.t_loop_done - f.t_opened,
                t_drained - f.t_loop_done, now_s() - t_drained);
}

/* the ONE exchange (exchange.c): every rank's partial, summed onto rank 0, which goes on alone */
static void exchange(stream_run *r)
{
    host_counts *hc = r->hc;
    uint64_t meta[4] = {hc ? hc->diff_subfam : 0, hc ? hc->dup_unique : 0, r->boundary_missed, r->ends};
    void *p64 = NULL, *p32 = NULL;
    exchange_partials(r->eng, meta, 4, r->timing, &p64, &p32);
    if (hc) {
        hc->diff_subfam = meta[0];
        hc->dup_unique = meta[1];
    }
    r->boundary_missed = meta[2];
    if (r->shared && !r->boundary_missed) fprintf(stderr, "\r* Processed read ends: %llu\n", (unsigned long long)meta[3]);
    if (!r->boundary_missed) {
        g_reduced_u64 = p64;
        g_reduced_u32 = p32;
    }
}

/* A share boundary did not hold (the split points are guesses that the rank before verifies): rank 0 scans the whole job again,
 * alone. */
static void scan_again_alone(stream_run *r)
{
    fprintf(stderr, "[iteres] note: a share boundary was not a record start; scanning the input again with one GPU\n");
    chk(itx_engine_reset(r->eng), "itx_engine_reset");
    if (r->hc) r->hc->diff_subfam = r->hc->dup_unique = 0;
    r->ends = 0;
    for (int i = 0; i < r->n_files; i++) r->share[i].lo = 0, r->share[i].hi = SIZE_MAX;
    r->shared = 0;
    for (int fi = 0; fi < r->n_files; fi++) scan_file(r, fi, 1);
}

/* filter -b: the last, short member, the EOF marker, and the counters for ITX_TIMING */
static void finish_bam(stream_run *r)
{
    if (!r->bam_f) return;
    if (r->bo && r->o->bam_sort) {
        /* -s: the held records are sorted and replayed a round at a time; a round's members are written while the next round's
         * kernels run */
        for (int more = 1; more;) {
            chk(itx_bamout_sort_next(r->bo, &more), "itx_bamout_sort_next");
            bam_write_out(r, more ? 1 : 0);
        }
    } else if (r->bo) {
        chk(itx_bamout_finish(r->bo), "itx_bamout_finish");
        bam_write_out(r, 0);
    }
    if (bgzf_write_eof(r->bam_f) != 0 || fclose(r->bam_f) != 0) die("writing %s: %s", r->o->bam_out_path, strerror(errno));
    r->bam_f = NULL;
    itx_bamout_index_result ir;
    memset(&ir, 0, sizeof ir);
    if (r->bo && r->o->bam_index) bam_index_end(r, &ir);
    if (r->timing) {
        itx_bamout_stats bs;
        memset(&bs, 0, sizeof bs);
        if (r->bo) chk(itx_bamout_get_stats(r->bo, &bs), "itx_bamout_get_stats");
        fprintf(stderr, "[itx timing] bam out: %llu records, %llu payload bytes, %llu members (%llu bytes), %.3f ms in the gather kernels, %.3f ms in the member kernels, host waited %.3f s, %llu batches gathered on the device, %llu batches by the host route%s",
                (unsigned long long)bs.records, (unsigned long long)bs.payload_bytes, (unsigned long long)bs.members, (unsigned long long)bs.out_bytes, bs.gather_ms,
                bs.member_ms, 1e-3 * bs.wait_ms, r->bam_dev_batches, r->bam_host_batches, r->o->bam_annotate || r->o->bam_index || r->o->bam_sort || r->o->bam_level_given ? "" : "\n");
        if (r->o->bam_annotate) {
            uint64_t tb = 0;
            if (r->bo) chk(itx_bamout_annotate_get_stats(r->bo, &tb), "itx_bamout_annotate_get_stats");
            fprintf(stderr, ", %llu tag bytes appended%s", (unsigned long long)tb + r->bam_host_tag_bytes, r->o->bam_index || r->o->bam_sort || r->o->bam_level_given ? "" : "\n");
        }
        if (r->o->bam_sort) {
            itx_bamout_sort_stats ss;
            memset(&ss, 0, sizeof ss);
            if (r->bo) chk(itx_bamout_sort_get_stats(r->bo, &ss), "itx_bamout_sort_get_stats");
            fprintf(stderr, "; sort: %llu records sorted, %llu rounds, %.3f ms in the sort kernels, %.3f ms in the replay gathers%s", (unsigned long long)ss.records,
                    (unsigned long long)ss.rounds, ss.sort_ms, ss.replay_ms, r->o->bam_index || r->o->bam_level_given ? "" : "\n");
        }
        if (r->o->bam_index)
            fprintf(stderr, "; index: %llu entries, %llu chunks, %llu bytes, %.3f ms in the entry kernels, %.3f ms in the final kernels%s", (unsigned long long)ir.entries,
                    (unsigned long long)ir.chunks, (unsigned long long)ir.len, ir.batch_ms, ir.finish_ms, r->o->bam_level_given ? "" : "\n");
        /* -l: the level the writer used ends the line; without -l the line is the one it was before there were levels */
        if (r->o->bam_level_given) fprintf(stderr, ", level %d\n", r->bo ? itx_bamout_get_level(r->bo) : r->o->bam_level);
    }
    itx_bamout_destroy(r->bo);
    r->bo = NULL;
    free(r->bbuf.bytes);
}

static void finish_names(stream_run *r, char ***locus_names)
{
    const rmsk_t *rm = r->rm;
    if (!r->want_qnames || !locus_names) return;
    char **out = xcalloc(rm->n_rows ? rm->n_rows : 1, sizeof(char *));
    *locus_names = out;
    if (r->nm) {
        /* one sort by row, stable in append order, and one text: every list is a NUL-terminated piece of it */
        itx_names_result nr;
        chk(itx_names_finish(r->nm, rm->n_rows ? rm->n_rows : 1, &nr), "itx_names_finish");
        for (size_t row = 0; row < rm->n_rows; row++)
            if (nr.row_off[row] != UINT64_MAX) out[row] = (char *)nr.text + nr.row_off[row];
        g_names_cnt = nr.row_cnt;
        return;
    }
    /* names per locus in BAM order (generic.c:1729 reverses the head-inserted list back to file order) */
    const hit_name *v = r->hn.v;
    size_t *len = xcalloc(rm->n_rows ? rm->n_rows : 1, sizeof(size_t));
    for (size_t i = 0; i < r->hn.n; i++) len[v[i].row] += strlen(v[i].name) + 1;
    for (size_t row = 0; row < rm->n_rows; row++)
        if (len[row]) {
            out[row] = xmalloc(len[row] + 1);
            out[row][0] = 0;
            len[row] = 0;
        }
    for (size_t i = 0; i < r->hn.n; i++) {
        char *dst = out[v[i].row] + len[v[i].row];
        const size_t k = strlen(v[i].name);
        if (len[v[i].row]) *dst++ = ',', len[v[i].row]++;
        memcpy(dst, v[i].name, k + 1);
        len[v[i].row] += k;
        free(v[i].name);
    }
    free(len);
}

/* the counters of bed, -R and veto for ITX_TIMING; their objects and what the host route kept go */
static void release_side_objects(stream_run *r)
{
    const int timing = r->timing;
    if (timing && r->veto_on)
        fprintf(stderr, "[itx timing] XA veto: %llu batches judged on the device, %llu by the host\n", r->veto_dev_batches, r->veto_host_batches);
    if (timing && r->want_bed) {
        itx_bed_stats bs;
        memset(&bs, 0, sizeof bs);
        if (r->bd) chk(itx_bed_get_stats(r->bd, &bs), "itx_bed_get_stats");
        fprintf(stderr, "[itx timing] bed: %llu batches built on the device (%llu bytes, %.3f ms in its kernels, host waited %.3f s), %llu by the host\n",
                (unsigned long long)bs.batches, (unsigned long long)bs.bytes, bs.kernel_ms, bs.wait_s, r->bed_host_batches);
    }
    itx_bed_destroy(r->bd);
    names_free(&r->warned);
    names_free(&r->chr_names);
    free(r->arg);
    if (r->bed_f) fclose(r->bed_f);
    if (r->bed_uniq_f) fclose(r->bed_uniq_f);
    dup_set_free(r->dups);
    if (r->dd) {
        uint64_t du = 0, dropped = 0, keys = 0;
        chk(itx_dedup_counts(r->dd, &du, &dropped, &keys), "itx_dedup_counts");
        if (r->hc) r->hc->dup_unique = du;
        if (timing) fprintf(stderr, "[itx timing] -R on the device: %llu records dropped (%llu of them MAPQ >= -Q), %llu keys, %.3f s in its kernels\n",
                            (unsigned long long)dropped, (unsigned long long)du, (unsigned long long)keys, r->t_dedup);
        itx_dedup_destroy(r->dd);
    }
    xa_index_free(r->xi);
    itx_xaveto_destroy(r->xv);
    free(r->iv);
    free(r->live);
}

/* the names' counters, the buffers of the lists (unless the caller took them) and the decoder */
static void teardown(stream_run *r, int lists_taken)
{
    const int timing = r->timing;
    free(r->hn.v);
    if (timing && r->want_qnames) {
        itx_names_stats ns;
        memset(&ns, 0, sizeof ns);
        if (r->nm) chk(itx_names_get_stats(r->nm, &ns), "itx_names_get_stats");
        fprintf(stderr, "[itx timing] names: %llu batches gathered on the device (%llu names, %llu bytes, %.3f ms in the gather kernels, %.3f ms sort + text), %llu batches by the host\n",
                (unsigned long long)ns.batches, (unsigned long long)ns.entries, (unsigned long long)ns.bytes, ns.gather_ms, ns.finish_ms, r->names_host_batches);
    }
    if (r->nm && !lists_taken) stream_names_free(NULL);
    free(r->nbuf.rows);
    free(r->nbuf.off);
    free(r->nbuf.bytes);
    free(r->gbuf.chrom);
    free(r->gbuf.start);
    free(r->gbuf.end);
    free(r->gbuf.uniq);
    for (int k = 0; k < 2; k++) {
        free(r->side[k].qname);
        free(r->side[k].xa);
        free(r->side[k].nm);
        free(r->side[k].raw);
        free(r->side[k].raw_off);
    }
    /* The decoder's device memory (17 GB for a big input) goes back NOW, not when the process ends: the driver clears released
     * memory in the background, and the next command's reservation of the same 17 GB waits for whatever is still uncleared —
     * 0.7 s now and then when one run followed another at once. With the files still to be written the driver has half a
     * second's head start, and the process's own exit has less to tear down. */
    if (g_inflater && !getenv("ITX_KEEP_DECODER")) {
        const double tr = now_s();
        itx_timing_report();
        itx_inflater_destroy(g_inflater);
        g_inflater = NULL;
        aln_use_device(NULL);
        if (timing) fprintf(stderr, "[itx timing] decoder released %.3f s\n", now_s() - tr);
    }
}

/* filter -G / -W, after the stream: the chromosomes in byte-wise order of their names (LC_ALL=C sort -k1,1), the change points of
 * both arrays; then (-W) each file's bigWig content, built on the device from those points and laid down by bigwig.c, and (-G) each
 * file's text round by round: round k is written while the device formats round k + 1 */
static const sizes_t *gcov_sort_sizes;
static int gcov_by_name(const void *a, const void *b)
{
    return strcmp(gcov_sort_sizes->names.name[*(const uint32_t *)a], gcov_sort_sizes->names.name[*(const uint32_t *)b]);
}

/* ITX_BW_HOST=1: the items from the change points copied back, everything else by bigwig.c with zlib (the reference's bytes) */
static int gcov_bigwig_host(itx_gcov *g, int w, const sizes_t *chr_sizes, const uint32_t *order, const uint32_t *size32, const char *path)
{
    itx_gcov_stats gs;
    chk(itx_gcov_get_stats(g, &gs), "itx_gcov_get_stats");
    const size_t n = (size_t)gs.points[w];
    uint32_t *pts = xmalloc(16 * (n + 1));
    chk(itx_gcov_copy_points(g, w, pts), "itx_gcov_copy_points");
    bw_item *it = xmalloc(sizeof *it * (n + 1));
    size_t k = 0;
    for (size_t j = 0; j + 1 < n; j++) {
        const uint32_t *p = pts + 4 * j, *q = p + 4;
        if (p[1] == 0 || q[2] != p[2]) continue;
        it[k++] = (bw_item){order[p[2]], p[0], q[0], (float)(double)p[1]};
    }
    /* (the points follow `order`, which is strcmp order: the items are grouped and sorted as the writer wants them) */
    const int wrote = write_bigwig_sparse(path, (const char *const *)chr_sizes->names.name, size32, it, k);
    free(it);
    free(pts);
    return wrote;
}

void stream_gcov_write(const sizes_t *chr_sizes, const char *const *text, const char *const *bigwig)
{
    itx_gcov *g = g_gcov;
    if (!g) die("filter -G / -W: no coverage was accumulated");
    const uint32_t n = chr_sizes->names.n;
    uint32_t *order = xmalloc(sizeof(uint32_t) * ((size_t)n + 1));
    for (uint32_t c = 0; c < n; c++) order[c] = c;
    gcov_sort_sizes = chr_sizes;
    qsort(order, n, sizeof(uint32_t), gcov_by_name);
    char *nb = NULL;
    uint64_t *no = NULL;
    loci_name_table(&chr_sizes->names, &nb, &no);
    const char *re = getenv("ITX_GCOV_ROUND_BYTES");                       /* tests: many rounds on a small input */
    const int rc = itx_gcov_finish(g, order, (int)n, nb, no, re && atoll(re) > 0 ? (size_t)atoll(re) : 0);
    if (rc == ITX_E_NOMEM) die("filter -G: %s", itx_last_error());
    chk(rc, "itx_gcov_finish");
    double t_write = 0, t_bw = 0;
    if (bigwig) {
        /* the visited chromosomes of finish (a size <= 2 has no slots and is not visited) in its order: place -> index */
        uint32_t *visited = xmalloc(sizeof(uint32_t) * ((size_t)n + 1)), *size32 = xmalloc(sizeof(uint32_t) * ((size_t)n + 1)), nv = 0;
        for (uint32_t k = 0; k < n; k++)
            if (chr_sizes->value[order[k]] > 2) visited[nv++] = order[k];
        for (uint32_t c = 0; c < n; c++) size32[c] = (uint32_t)chr_sizes->value[c];
        const int host = getenv("ITX_BW_HOST") != NULL;
        for (int w = 0; w < 2; w++) {
            const double t0 = now_s();
            int wrote;
            if (host) {
                wrote = gcov_bigwig_host(g, w, chr_sizes, visited, size32, bigwig[w]);
            } else {
                const int brc = itx_gcov_bigwig_build(g, w);
                if (brc == ITX_E_NOMEM || brc == ITX_E_LIMIT) die("filter -W: %s", itx_last_error());
                chk(brc, "itx_gcov_bigwig_build");
                itx_gcov_bw_result r;
                chk(itx_gcov_bigwig_result(g, w, &r), "itx_gcov_bigwig_result");
                wrote = write_bigwig_sparse_device(bigwig[w], (const char *const *)chr_sizes->names.name, size32, &r);
                if (wrote && getenv("ITX_TIMING"))
                    fprintf(stderr, "[itx timing] genome coverage bigWig %d: %llu items, %llu sections, %u levels (first reduction %u after %u tries), %llu blocks; "
                                    "device: items %.3f ms, chain %.3f ms, fold %.3f ms, deflate %.3f ms\n",
                            w, (unsigned long long)r.n_items, (unsigned long long)r.n_sec, r.n_levels, r.reduction[0], r.reduce_rounds, (unsigned long long)r.n_blocks,
                            r.items_ms, r.chain_ms, r.fold_ms, r.deflate_ms);
            }
            if (!wrote) {
                /* the reference's converter refuses an input without a line; a file an earlier run left would be taken for this run's */
                if (remove(bigwig[w]) != 0 && errno != ENOENT) die("removing %s: %s", bigwig[w], strerror(errno));
                fprintf(stderr, "* %s is not written: the coverage has no data\n", bigwig[w]);
            }
            t_bw += now_s() - t0;
        }
        free(visited);
        free(size32);
    }
    for (int w = 0; text && w < 2; w++) {
        FILE *f = fopen(text[w], "w");
        if (!f) die("mustOpen: Can't open %s to write: %s", text[w], strerror(errno));
        itx_gcov_text tx;
        do {
            chk(itx_gcov_next(g, w, &tx), "itx_gcov_next");
            const double t0 = now_s();
            if (tx.len && fwrite(tx.bytes, 1, tx.len, f) != tx.len) die("writing %s: %s", text[w], strerror(errno));
            t_write += now_s() - t0;
        } while (tx.more);
        if (fclose(f) != 0) die("writing %s: %s", text[w], strerror(errno));
    }
    if (getenv("ITX_TIMING")) {
        itx_gcov_stats gs;
        chk(itx_gcov_get_stats(g, &gs), "itx_gcov_get_stats");
        fprintf(stderr, "[itx timing] genome coverage: %llu records added (%llu with MAPQ >= -Q, %llu out of range), %llu batches on the device, %llu by the host route; "
                        "%llu + %llu change points, %llu + %llu lines, %llu + %llu bytes in %llu + %llu rounds; device: add %.3f ms, points %.3f ms, text %.3f ms, zeroing %.3f ms; "
                        "host waited %.3f s, wrote for %.3f s; two arrays of %llu slots (%llu bytes) allocated in %.3f s\n",
                (unsigned long long)gs.records, (unsigned long long)gs.records_uniq, (unsigned long long)gs.out_of_range, g_gcov_dev_batches, g_gcov_host_batches,
                (unsigned long long)gs.points[0], (unsigned long long)gs.points[1], (unsigned long long)gs.lines[0], (unsigned long long)gs.lines[1],
                (unsigned long long)gs.bytes[0], (unsigned long long)gs.bytes[1], (unsigned long long)gs.rounds[0], (unsigned long long)gs.rounds[1], gs.add_ms, gs.points_ms,
                gs.text_ms, gs.zero_ms, gs.wait_s, t_write, (unsigned long long)gs.slots, (unsigned long long)gs.device_bytes, gs.alloc_s);
        if (bigwig)
            fprintf(stderr, "[itx timing] genome coverage bigWigs: %llu + %llu items, %llu + %llu sections, %llu + %llu levels, %llu + %llu summaries; device %.3f ms; "
                            "built and written in %.3f s\n",
                    (unsigned long long)gs.bw_items[0], (unsigned long long)gs.bw_items[1], (unsigned long long)gs.bw_sections[0], (unsigned long long)gs.bw_sections[1],
                    (unsigned long long)gs.bw_levels[0], (unsigned long long)gs.bw_levels[1], (unsigned long long)gs.bw_summaries[0], (unsigned long long)gs.bw_summaries[1],
                    gs.bw_ms, t_bw);
    }
    free(nb);
    free(no);
    free(order);
    itx_gcov_destroy(g);
    g_gcov = NULL;
}

void run_stream(const run_opts *o, const rmsk_t *rm, const sizes_t *chr_sizes, int filter_mode, int multi_file,
                unsigned progress_every, int want_qnames, itx_engine **eng_out, itx_table **tab_out, char ***locus_names,
                host_counts *hc)
{
    const int want_bed = o->bed_path || o->bed_uniq_path;
    stream_run run = {.o = o, .rm = rm, .chr_sizes = chr_sizes, .filter_mode = filter_mode, .multi_file = multi_file, .progress_every = progress_every,
                      .hc = hc, .timing = getenv("ITX_TIMING") != NULL, .want_qnames = want_qnames, .want_bed = want_bed,
                      .veto_on = o->xa_veto && !filter_mode, .dev_veto = !getenv("ITX_HOST_VETO")}, *r = &run;

    make_table_and_engine(r);
    if (o->gcov) {
        /* filter -G: one u32 slot per base of the size file, twice. A device that cannot hold them ends the command here, with one
         * line, before the stream starts */
        const int rc = itx_gcov_create(multi_device(), chr_sizes->value, (int)chr_sizes->names.n, &r->p, BATCH_RECORDS, &r->gc);
        if (rc == ITX_E_NOMEM || rc == ITX_E_LIMIT) die("filter -G: %s", itx_last_error());
        chk(rc, "itx_gcov_create");
        g_gcov = r->gc;
    }
    open_outputs_and_side_buffers(r);
    list_files_and_shares(r);
    join_helper_thread(r);
    choose_dedup_set(r);
    /* this rank's shares, then (a job of several ranks) the exchange — after which rank 0 is alone */
    for (int fi = 0; fi < r->n_files; fi++) scan_file(r, fi, 0);
    if (multi_world() > 1 || multi_selftest()) {
        exchange(r);
        if (r->boundary_missed) scan_again_alone(r);
    }
    finish_bam(r);
    release_side_objects(r);
    finish_names(r, locus_names);
    teardown(r, want_qnames && locus_names);
    *eng_out = r->eng;
    *tab_out = r->tab;
}
