/* out_gcov.c — the genome coverage of filter -G / -W (csrc/itx_gcov.hip): as stream.c's record loop feeds it (the steps: stream_priv.h),
 * and the writer of its files, which runs after the stream (stream_gcov_write, called by cmd_filter.c). */
#include "stream_priv.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

/* filter -G: what the stream left on the device for stream_gcov_write, and the batches each route added (ITX_TIMING) */
static itx_gcov *g_gcov;
static unsigned long long g_gcov_dev_batches, g_gcov_host_batches;

/* filter -G: one u32 slot per base of the size file, twice. A device that cannot hold them ends the command here, with one
 * line, before the stream starts */
void gcov_open(stream_run *r)
{
    if (!r->o->gcov) return;
    const int rc = itx_gcov_create(multi_device(), r->chr_sizes->value, (int)r->chr_sizes->names.n, &r->p, BATCH_RECORDS, &r->gc);
    if (rc == ITX_E_NOMEM || rc == ITX_E_LIMIT) die("filter -G: %s", itx_last_error());
    chk(rc, "itx_gcov_create");
    g_gcov = r->gc;
}

void gcov_tidmap(stream_run *r, const stream_file *f)
{
    if (r->gc) chk(itx_gcov_set_tidmap(r->gc, f->t2c, f->nt > 0 ? f->nt : 0), "itx_gcov_set_tidmap");
}

int gcov_rows(stream_run *r, int32_t **hits, void **stream)
{
    if (!r->gc) return 0;
    *hits = itx_gcov_hits(r->gc);
    *stream = itx_gcov_stream(r->gc);
    return 1;
}

/* The coverage's kernel follows the rows on the stream they were written on. */
void gcov_device_batch(stream_run *r, const itx_batch *db, size_t n, chosen_rows *rows)
{
    if (!r->gc) return;
    batch_rows(r, db, n, rows);
    chk(itx_gcov_run(r->gc, db, rows->hits, n, rows->stream), "itx_gcov_run");
    g_gcov_dev_batches++;
}

void gcov_window_done(stream_run *r)
{
    if (r->gc) chk(itx_gcov_wait_kernels(r->gc), "itx_gcov_wait_kernels");
}

/* filter -G: the records of slot k that chose a row add the interval the lookup ran on (host_derive: itx_derive of
 * ../csrc/itx_derive.h). One that has none, which no counted record is, goes up with no chromosome and is counted as out of range. */
void gcov_host_batch(stream_run *r, int k)
{
    if (!r->gc) return;
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

void gcov_free(stream_run *r)
{
    free(r->gbuf.chrom);
    free(r->gbuf.start);
    free(r->gbuf.end);
    free(r->gbuf.uniq);
}

/* filter -G / -W, after the stream: the chromosomes in byte-wise order of their names (LC_ALL=C sort -k1,1), the change points of
 * both arrays; then (-W) each file's bigWig content, built on the device from those points and laid down by bw_sparse.c, and (-G) each
 * file's text round by round: round k is written while the device formats round k + 1 */
static const sizes_t *gcov_sort_sizes;
static int gcov_by_name(const void *a, const void *b)
{
    return strcmp(gcov_sort_sizes->names.name[*(const uint32_t *)a], gcov_sort_sizes->names.name[*(const uint32_t *)b]);
}

/* ITX_BW_HOST=1: the items from the change points copied back, everything else by bw_sparse.c with zlib (the reference's bytes) */
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
