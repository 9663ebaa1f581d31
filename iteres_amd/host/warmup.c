/* warmup.c — the helper thread of stream.c's run. The first HIP call costs a few hundred milliseconds of runtime start-up; a helper
 * thread pays them while the main thread parses the rmsk file. It goes on to make and reserve the device decoder with its
 * page-locked chunk buffers, to open the first alignment file, and to parse records ahead of the table. What it leaves is `out`
 * (helper_out, stream_priv.h, where the rule for who touches it when is written down); gpu_warmup_join hands it over. */
#define _GNU_SOURCE
#include "stream_priv.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

static pthread_t warm_thread;
static int warm_on, warm_bam;
static int warm_single;                       /* the argument names one file */
static helper_out out = {.hi = SIZE_MAX};

/* BAM input is decoded on the device (include/iteres_amd.h: itx_bamwin_*: blocks inflated, records located and parsed
 * there) unless ITX_HOST_INFLATE is set. The reader's compressed-chunk buffers then have to be page-locked, which takes
 * its time: the helper thread gets them ready while the main thread parses the rmsk file, and hands them out from this
 * little pool. */
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

void use_device_reader(void)
{
    const aln_device_ops ops = {out.inflater,       itx_bamwin_push_begin, itx_bamwin_push_end, itx_bamwin_patch, itx_bamwin_truncate, itx_bamwin_carry, itx_bamwin_avail, itx_bamwin_peek,
                                itx_bamwin_skip, itx_bamwin_parse, itx_bamwin_fetch, itx_bamwin_bytes,    itx_bamwin_tids,  itx_bamwin_device_batch,
                                pool_alloc,      pool_release,     itx_last_error,   out.dev_windows,       out.dev_max_blocks, out.dev_max_bytes, itx_bamwin_xa_veto, itx_bamwin_push_copied,
                                itx_bamwin_bed,  itx_bamwin_names, itx_bamwin_bamout};
    aln_use_device(&ops);
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
static int pre_stop;                           /* gpu_warmup_join: table and engine are there */
void stream_prefetch_allow(const run_opts *o, int filter_mode, int allowed)
{
    pre_opts = o;
    pre_filter_mode = filter_mode;
    pre_allowed = allowed;
}
void stream_sizes_ready(const sizes_t *chr_sizes) { __atomic_store_n(&pre_sizes, chr_sizes, __ATOMIC_RELEASE); }

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
    size_t cap = out.input_bytes / 60 + ((size_t)1 << 20);                     /* no BAM record takes less than that compressed */
    if (cap > ((size_t)160 << 20)) cap = (size_t)160 << 20;
    if (itx_backlog_create(multi_device(), cap, &out.backlog) != ITX_OK) {
        out.backlog = NULL;
        free(t2c);
        return;
    }
    const int veto_on = o->xa_veto && !pre_filter_mode;
    while (!__atomic_load_n(&pre_stop, __ATOMIC_ACQUIRE)) {
        int wfl = 0;
        const uint8_t *seen = NULL;
        if (!aln_device_window(rd, &wfl, &seen)) break;                         /* end of input */
        if (!window_goes_direct(wfl, seen, t2c, nt, veto_on, 0) || aln_device_left(rd) > itx_backlog_room(out.backlog)) break;
        itx_batch db;
        const size_t n = aln_read_batch_device(rd, SIZE_MAX, &db);
        if (n == 0) break;
        size_t at = 0;
        if (itx_backlog_append(out.backlog, &db, n, &at) != ITX_OK) die("records parsed ahead: %s", itx_last_error());
        if (out.n_ent == out.cap_ent) {
            out.cap_ent = out.cap_ent ? out.cap_ent * 2 : 64;
            out.ent = xrealloc(out.ent, sizeof *out.ent * out.cap_ent);
        }
        out.ent[out.n_ent].at = at;
        out.ent[out.n_ent].n = n;
        out.ent[out.n_ent].paired = db.mpos != NULL;
        out.n_ent++;
    }
    free(t2c);
    out.seconds = now_s() - t0;
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
        const size_t mine_bytes = out.input_bytes ? out.input_bytes / (size_t)(multi_world() > 0 ? multi_world() : 1) : 0;
        step = mine_bytes && !ce ? aln_raw_step(mine_bytes + mine_bytes / 64) : chunk;
        pin_want = step + (1u << 17);
        /* as many as a file of this size makes the reader use */
        pin_count = out.input_bytes ? (int)(mine_bytes / step + 1) : 2;
        if (pin_count > ALN_DEVICE_RAW_BUFFERS) pin_count = ALN_DEVICE_RAW_BUFFERS;
        if (getenv("ITX_PIN_EARLY") && atoi(getenv("ITX_PIN_EARLY")) >= 1 && atoi(getenv("ITX_PIN_EARLY")) < pin_count) pin_count = atoi(getenv("ITX_PIN_EARLY"));   /* (A/B) */
        pool_pinning = pin_count;
        pin_on = pthread_create(&pin_th, NULL, pin_main, NULL) == 0;
        if (!pin_on) pool_pinning = 0;
    }
    if (ndev > 0 && warm_bam && !getenv("ITX_HOST_INFLATE") && (inf_rc = itx_inflater_create(multi_device(), &out.inflater)) != ITX_OK)
        snprintf(out.err, sizeof out.err, "%s", itx_last_error());
    else if (ndev <= 0)
        snprintf(out.err, sizeof out.err, "no usable GPU (%s)", itx_last_error());
    t_created = now_s();
    if (!pin_on && out.inflater) {
        pin_count = 2;
        pool_pinning = 2;
        pin_main(NULL);
    }
    t_pinned = now_s();
    if (!out.inflater) aln_use_device(NULL);                              /* it did not come up: the host decodes (run_stream says why when that will not do) */
    if (out.inflater) {
        /* the device side of the decoder, all of it, now that nothing runs there yet: windows and per-push scratch sized for
         * the most a push may carry (the block indexer cuts a chunk that inflates to more into two pushes) */
        const char *be = getenv("ITX_DEV_WINDOW_BLOCKS");
        const char *me = getenv("ITX_RESERVE_BLOCKS");                   /* scratch experiments */
        size_t max_blocks = be && atol(be) >= 1 ? (size_t)atol(be) : me && atol(me) >= 64 ? (size_t)atol(me) : 12288;
        /* no more than this rank's share of the input can need: a small file gets small buffers (a block of a real BAM takes
         * kilobytes; a file of smaller ones is simply cut into more pushes by the indexer) */
        if (out.input_bytes) {
            const size_t mine = out.input_bytes / (size_t)(multi_world() > 0 ? multi_world() : 1);
            const size_t est = mine / 2048 + 64;
            if (!be && est < max_blocks) max_blocks = est;
            const size_t nchunks = mine / chunk + 3;
            if (nchunks < ITX_BAMWIN_WINDOWS) out.dev_windows = (int)nchunks;          /* in: the most this input can use */
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
            if (out.dev_windows < 1 || out.dev_windows > ring) out.dev_windows = ring;
        }
        const size_t max_bytes = max_blocks * 65280u < ((size_t)1 << 30) ? max_blocks * 65280u : (size_t)1 << 30;
        if (!getenv("ITX_NO_RESERVE") && itx_inflater_reserve(out.inflater, step + (1u << 17), max_blocks, max_bytes, &out.dev_windows) == ITX_OK) {
            out.dev_max_blocks = max_blocks;
            out.dev_max_bytes = max_bytes;
        } else {
            out.dev_windows = 0;
        }
    }
    const double c = now_s();
    /* ITX_DECODE_AFTER_TABLE=1 (measuring): the decoder's first push waits until table and engine exist, so that it runs beside
     * nothing of theirs — the rate it reaches then is the ceiling of a run. Nothing is parsed ahead in such a run. */
    if (out.inflater && out.first && getenv("ITX_DECODE_AFTER_TABLE") && atoi(getenv("ITX_DECODE_AFTER_TABLE")) != 0)
        while (!__atomic_load_n(&pre_stop, __ATOMIC_ACQUIRE)) usleep(200);
    if (out.inflater && out.first) {
        /* the first file's header, and its first windows decoded while the main thread is still parsing the rmsk file; a
         * file that does not open is left to run_stream, which reports it where the reference does */
        use_device_reader();
        share_t sh0;
        char *one[1] = {out.first};
        /* this rank's share of the FIRST file when the list has one file (the common case); longer lists are opened by the loop */
        if (multi_world() <= 1) {
            out.reader = aln_open(out.first, 0);
        } else if (warm_single && plan_shares(one, 1, out.splittable, multi_rank(), multi_world(), multi_min_share(), &sh0) && sh0.lo != sh0.hi) {
            out.reader = aln_open_range(out.first, sh0.lo, sh0.hi);
            out.lo = sh0.lo;
            out.hi = sh0.hi;
        }
        if (out.reader) aln_readahead(out.reader);
    }
    const double t_opened = now_s();
    if (getenv("ITX_TIMING"))
        fprintf(stderr, "[itx timing] HIP runtime start-up %.3f s, device inflater + page-locked buffers %.3f s (streams %.3f, page-locked %.3f, device reserve %.3f), first file opened %.3f s (helper thread)\n", b - a,
                c - b, t_created - b, t_pinned - t_created, c - t_pinned, t_opened - c);
    {
        const char *me = getenv("ITX_PREFETCH_MIN");                       /* bytes of input below which it is not worth a backlog (tests: 0) */
        const size_t min_bytes = me ? (size_t)atoll(me) : (size_t)1 << 30;
        if (out.reader && pre_allowed && pre_opts && multi_world() <= 1 && out.input_bytes >= min_bytes && !getenv("ITX_NO_PREFETCH")) prefetch_records(out.reader);
    }
    if (pin_on) pthread_join(pin_th, NULL);                              /* (long done: it started when the runtime came up) */
    return NULL;
}
void gpu_warmup_start(int bam_input, const char *aln_arg, int multi_file, int splittable)
{
    warm_bam = bam_input;
    out.splittable = splittable;
    if (bam_input && aln_arg) {
        out.first = xstrdup(aln_arg);
        char *c = multi_file ? strchr(out.first, ',') : NULL;
        warm_single = c == NULL;
        if (c) *c = 0;
        char *all = xstrdup(aln_arg), *save = NULL;
        out.input_bytes = 0;
        for (char *tok = multi_file ? strtok_r(all, ",", &save) : all; tok; tok = multi_file ? strtok_r(NULL, ",", &save) : NULL) {
            struct stat sb;
            if (stat(tok, &sb) == 0 && S_ISREG(sb.st_mode)) out.input_bytes += (size_t)sb.st_size;
            else {
                out.input_bytes = 0;                                   /* a pipe: no idea */
                break;
            }
        }
        free(all);
    }
    /* A rank that makes its RCCL communicator beside the scan builds its table on the host, as every run did before the device
     * build: the early thread loads librccl — which registers its kernels with the HIP runtime — and runs ncclCommInitRank at the
     * very moment the device build would launch its first kernels on the main thread, and such a run (tests/test_cli_multi.py,
     * one rank walking the RCCL exchange) died with a segmentation fault in one of two tries, before either thread had printed a
     * timing line. With the host build the main thread launches nothing in that window, as before. Set here, before any other
     * thread of the process reads the environment; a value the user gave stays. */
    if (exchange_comm_early_wanted()) setenv("ITX_TABLE_HOST", "1", 0);
    if (!warm_on && pthread_create(&warm_thread, NULL, warm_main, NULL) == 0) warm_on = 1;
}
helper_out *gpu_warmup_join(void)
{
    if (getenv("ITX_PREFETCH_HOLD_MS")) usleep((useconds_t)atol(getenv("ITX_PREFETCH_HOLD_MS")) * 1000u);     /* tests: a table that takes its time */
    __atomic_store_n(&pre_stop, 1, __ATOMIC_RELEASE);                  /* table and engine are there: the helper thread finishes the window it is at */
    if (warm_on) pthread_join(warm_thread, NULL);
    warm_on = 0;
    return &out;
}
