/* stream.c — the record loop of the reference (generic.c:700-1062 stat copy, 343-697 filter copy) as a host pipeline around the
 * GPU engine. run_stream is the list of steps; record_loop is the dispatcher: a BAM window the device decoder parsed goes to the
 * engine where it lies (device_window: per batch bed text, names, veto, progress, submit — the reference's order) when the file
 * may hand off and window_goes_direct; everything else, and the rest of a window only the host can read (host_takes_over), goes
 * through host_batch: one pinned staging slot decoded while the other is in flight, then warnings with progress, -R and bed lines
 * in file order, the XA veto (side.c), submit. The helper thread that starts the runtime and decodes ahead is warmup.c; the three
 * outputs made of the rows the records chose (read lists, BAM, genome coverage) are out_names.c, out_bam.c and out_gcov.c, fed here
 * through gather_device_batch / gather_host_batch / gather_window_done on the batch's rows (batch_rows). -R, the bed text and the
 * veto act on the records before they are counted and stay here. */
#define _GNU_SOURCE
#include "stream_priv.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>

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
int32_t chrom_of_target(const char *target, const run_opts *o, const sizes_t *chr_sizes)
{
    char buf[4096];
    const char *nm = rename_chr(target, o->add_chr, buf, sizeof buf);
    if (!nm) return -2;
    const int64_t id = names_find(&chr_sizes->names, nm);
    return (id >= 0 && (int)chr_sizes->value[id] != 2) ? (int32_t)id : -1;
}

/* May this window go to the engine where it lies? Not with XA tags while the veto is on, unless the veto may run on the device
 * too (itx_xaveto_*); not with a mapped record on a chromosome the size file lacks (the warning is per record, in file order). */
int window_goes_direct(int wfl, const uint8_t *seen, const int32_t *t2c, int nt, int veto_on, int dev_veto)
{
    if (veto_on && (wfl & 2) && !dev_veto) return 0;
    for (int t = 0; t < nt; t++)
        if (seen[t] && t2c[t] == -1) return 0;
    return 1;
}

/* -R on the device: every window, right after its records are parsed (aln_set_window_hook) */
static void dedup_window(void *ctx, size_t n_rec)
{
    (void)n_rec;
    stream_run *r = ctx;
    const double t0 = now_s();
    chk(itx_bamwin_dedup(r->h->inflater, r->dd), "itx_bamwin_dedup");
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

/* ---- the three outputs made of the chosen rows, in the fixed order lists, BAM, coverage (the steps: stream_priv.h) */

/* the batch the device route has just taken. 0: only the host can read it (a name), and nothing else of it was gathered */
static int gather_device_batch(stream_run *r, stream_file *f, const itx_batch *db, size_t n, chosen_rows *rows)
{
    if (!lists_device_batch(r, f, db, n, rows)) return 0;
    bam_device_batch(r, f, db, n, rows);
    gcov_device_batch(r, db, n, rows);
    return 1;
}
/* the records of host slot k, whose rows are back */
static void gather_host_batch(stream_run *r, int k)
{
    lists_host_batch(r, k);
    bam_host_batch(r, k);
    gcov_host_batch(r, k);
}
/* their kernels are through: with the window's arrays, which are the decoder's again, or before the host route reads on */
static void gather_window_done(stream_run *r)
{
    lists_window_done(r);
    bam_window_done(r);
    gcov_window_done(r);
}

/* wait for host slot k and collect what its previous batch left behind; returns the seconds waited */
static double drain_slot(stream_run *r, int k)
{
    const double t0 = now_s();
    chk(itx_engine_wait_slot(r->eng, k), "itx_engine_wait_slot");
    const double waited = now_s() - t0;
    if (!r->pend[k]) return waited;
    gather_host_batch(r, k);
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

/* The rows of the batch (stream_priv.h: chosen_rows), classified once into the buffer of the first of lists, BAM, coverage that
 * exists. Lists and BAM are in stream order: what the host route still holds of earlier batches goes to them first. */
void batch_rows(stream_run *r, const itx_batch *db, size_t n, chosen_rows *rows)
{
    if (rows->done) return;
    int32_t *hits = NULL;
    if (lists_rows(r, &hits, &rows->stream) || bam_rows(r, &hits, &rows->stream)) drain_slots(r, 0);
    else gcov_rows(r, &hits, &rows->stream);                         /* sums commute: no order to keep with the host route's batches */
    chk(itx_engine_classify_device(r->eng, db, n, hits, rows->stream), "itx_engine_classify_device");
    rows->hits = hits;
    rows->done = 1;
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
    r->shared = plan_shares(r->files, r->n_files, r->h->splittable && !getenv("ITX_HOST_INFLATE"), multi_rank(), multi_world(), multi_min_share(), r->share) &&
                multi_world() > 1;
}

/* the helper thread (HIP start-up, device decoder, first file opened and decoding ahead) has had the rmsk parse and the table
 * build to finish */
static void join_helper_thread(stream_run *r)
{
    const double t_join = now_s();
    r->h = gpu_warmup_join();
    if (r->timing) fprintf(stderr, "[itx timing] waited %.3f s for the helper thread\n", now_s() - t_join);
    if (r->h->inflater) use_device_reader();
}

/* -R: one set over all files, like `dup` (generic.c:721). BAM decoded on the device: the set lives there too
 * (csrc/itx_dedup.hip) and marks a window's duplicates where the window lies, right after it is parsed; SAM text, the host
 * decoder and ITX_HOST_DEDUP=1: the host's hash set, record by record */
static void choose_dedup_set(stream_run *r)
{
    const run_opts *o = r->o;
    const helper_out *h = r->h;
    if (o->dedup && h->inflater && !o->is_sam && !getenv("ITX_HOST_DEDUP")) {
        size_t cells = h->input_bytes / 24;                         /* a first guess at the keys to come; the table grows */
        if (cells < ((size_t)1 << 20)) cells = (size_t)1 << 20;
        if (cells > ((size_t)1 << 28)) cells = (size_t)1 << 28;
        chk(itx_dedup_create(multi_device(), r->chr_sizes->value, (int)r->chr_sizes->names.n, &r->p, cells, &r->dd), "itx_dedup_create");
    }
    r->dups = o->dedup && !r->dd ? dup_set_new() : NULL;
    if (r->shared && !h->inflater) die("rank %d: the device decoder did not come up: %s", multi_rank(), h->err[0] ? h->err : itx_last_error());
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
    char *text = xmalloc(bytes + 1);
    uint64_t *off = xmalloc(sizeof(uint64_t) * ((size_t)nt + 1));
    size_t at = 0;
    for (int t = 0; t < nt; t++) {
        const size_t k = strlen(aln_target_name(rd, t));
        off[t] = at;
        memcpy(text + at, aln_target_name(rd, t), k);
        at += k;
    }
    off[nt] = at;
    itx_samtext *x = NULL;
    /* room for a chunk of text; for BGZF, whose chunks end with a whole member, 64 KiB more and the tail of the chunk before */
    size_t room = aln_sam_chunk_bytes() + 65536 + ALN_SAM_CARRY;
    if (room > (size_t)256 << 20) room = (size_t)256 << 20;              /* the most an object takes: a longer text is the host's */
    chk(itx_samtext_create(multi_device(), text, off, nt, room, &x), "itx_samtext_create");
    free(text);
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
    helper_out *h = r->h;
    int backlog = 0;
    f->t_open0 = now_s();
    if (fi == 0 && pass == 0 && h->reader && h->first && strcmp(r->files[0], h->first) == 0 && h->lo == sh->lo && h->hi == sh->hi) {
        f->rd = h->reader;                                               /* opened and decoding since the helper thread came up */
        h->reader = NULL;
        backlog = h->backlog != NULL;
    } else {
        if (h->reader && fi == 0 && pass == 0) {                         /* opened for another share than this plan's: not used */
            aln_close(h->reader);
            h->reader = NULL;
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
    if (!only) gcov_tidmap(r, f);
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
     * host). Nor do the read lists of filter -r on the device route (lists_open: ITX_HOST_NAMES=0). */
    f->dev_bed = r->want_bed && r->h->inflater && !o->is_sam && !getenv("ITX_HOST_BED");
    lists_open(r, f);
    f->handoff_ok = !r->dups && (!r->want_bed || f->dev_bed) && (!r->want_qnames || f->dev_names);
    if (f->dev_bed && !r->bd) create_bed(r, f);
    bam_open(r, f);
}

/* the records the helper thread parsed while the table was being built: first, in file order */
static void submit_backlog(stream_run *r)
{
    const helper_out *h = r->h;
    const double td = now_s();
    unsigned long long got = 0;
    for (size_t k = 0; k < h->n_ent; k++)
        for (size_t off = 0; off < h->ent[k].n; off += BATCH_RECORDS) {
            const size_t m = h->ent[k].n - off < BATCH_RECORDS ? h->ent[k].n - off : BATCH_RECORDS;
            itx_batch db;
            chk(itx_backlog_batch(h->backlog, h->ent[k].at + off, h->ent[k].paired, &db), "itx_backlog_batch");
            progress_marks(r, m);
            got += m;
            chk(itx_engine_submit_device_own(r->eng, &db, m, NULL), "itx_engine_submit_device_own");
        }
    chk(itx_engine_wait_own(r->eng), "itx_engine_wait_own");
    if (r->timing)
        fprintf(stderr, "\n[itx timing] parsed ahead of the table by the helper thread: %llu records of %zu windows (%.3f s there), submitted in %.3f s\n", got, h->n_ent,
                h->seconds, now_s() - td);
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
        /* lists, BAM, coverage: classify once, gather, and only then submit */
        chosen_rows rows = {NULL, NULL, 0};
        if (!gather_device_batch(r, f, &db, n, &rows)) return host_takes_over(r, f, n, 0, tq);
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
            gather_window_done(r);
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
 * else one batch by the host route — which prints and reads only after the pending bed text is written and the outputs' kernels
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
        gather_window_done(r);
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
    helper_out *h = r->h;
    if (h->backlog && fi == 0 && pass == 0) {                          /* used or not (another share than the plan's): gone */
        itx_backlog_destroy(h->backlog);
        h->backlog = NULL;
        free(h->ent);
        h->ent = NULL;
        h->n_ent = h->cap_ent = 0;
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

/* the buffers of the three outputs (the lists unless the caller took them), of the host route, and the decoder */
static void teardown(stream_run *r, int lists_taken)
{
    lists_free(r, lists_taken);
    bam_free(r);
    gcov_free(r);
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
    if (r->h->inflater && !getenv("ITX_KEEP_DECODER")) {
        const double tr = now_s();
        itx_timing_report();
        itx_inflater_destroy(r->h->inflater);
        r->h->inflater = NULL;
        aln_use_device(NULL);
        if (r->timing)fprintf(stderr, "[itx timing] decoder released %.3f s\n", now_s() - tr);
    }
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
    gcov_open(r);
    open_outputs_and_side_buffers(r);
    join_helper_thread(r);
    list_files_and_shares(r);
    choose_dedup_set(r);
    /* this rank's shares, then (a job of several ranks) the exchange — after which rank 0 is alone */
    for (int fi = 0; fi < r->n_files; fi++) scan_file(r, fi, 0);
    if (multi_world() > 1 || multi_selftest()) {
        exchange(r);
        if (r->boundary_missed) scan_again_alone(r);
    }
    bam_finish(r);
    release_side_objects(r);
    lists_finish(r, locus_names);
    teardown(r, want_qnames && locus_names);
    *eng_out = r->eng;
    *tab_out = r->tab;
}
