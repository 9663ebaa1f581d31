/* out_names.c — the read lists of filter -r, as stream.c's record loop feeds them (the steps: stream_priv.h).
 * On the device (csrc/itx_names.hip): the lists are gathered where the records lie; what the host route reads goes to
 * the same pool, in stream order (itx_names_append_host), so the end of the stream has one list to sort whatever route a window
 * took. The host route (ITX_HOST_NAMES=1), SAM text and the host decoder keep the lists on the host as before. */
#include "stream_priv.h"

#include <stdlib.h>
#include <string.h>

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
void lists_host_batch(stream_run *r, int k)
{
    if (!r->want_qnames) return;
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

/* Nor do the read lists keep a window on the host when they are built on the device (ITX_HOST_NAMES=0) */
void lists_open(stream_run *r, stream_file *f)
{
    f->dev_names = r->want_qnames && r->h->inflater && !r->o->is_sam && !names_by_host();
    if (f->dev_names && !r->nm) {
        chk(itx_names_create(multi_device(), BATCH_RECORDS, 0, &r->nm), "itx_names_create");
        g_names = r->nm;
    }
}

int lists_rows(stream_run *r, int32_t **hits, void **stream)
{
    if (!r->nm) return 0;
    *hits = itx_names_hits(r->nm);
    *stream = itx_names_stream(r->nm);
    return 1;
}

/* Classify into the lists' buffer first, gather, and only then submit: a batch whose names only the host can read has then not
 * been counted yet, and the host route counts it once. (filter runs no veto: the rows are final.) */
int lists_device_batch(stream_run *r, stream_file *f, const itx_batch *db, size_t n, chosen_rows *rows)
{
    if (!r->nm) return 1;
    uint64_t hard = 0;
    batch_rows(r, db, n, rows);
    if (aln_device_names(f->rd, r->nm, n, rows->hits, rows->stream, &hard) != 0) die("device read lists: %s", itx_last_error());
    return !hard;
}

void lists_window_done(stream_run *r)
{
    if (r->nm) chk(itx_names_wait_kernels(r->nm), "itx_names_wait_kernels");
}

static void build_lists(stream_run *r, char ***locus_names)
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

/* the lists for the writer, and the names' counters for ITX_TIMING */
void lists_finish(stream_run *r, char ***locus_names)
{
    build_lists(r, locus_names);
    if (r->timing && r->want_qnames) {
        itx_names_stats ns;
        memset(&ns, 0, sizeof ns);
        if (r->nm) chk(itx_names_get_stats(r->nm, &ns), "itx_names_get_stats");
        fprintf(stderr, "[itx timing] names: %llu batches gathered on the device (%llu names, %llu bytes, %.3f ms in the gather kernels, %.3f ms sort + text), %llu batches by the host\n",
                (unsigned long long)ns.batches, (unsigned long long)ns.entries, (unsigned long long)ns.bytes, ns.gather_ms, ns.finish_ms, r->names_host_batches);
    }
}

/* the buffers of the lists (the device's unless the caller took them) */
void lists_free(stream_run *r, int lists_taken)
{
    free(r->hn.v);
    if (r->nm && !lists_taken) stream_names_free(NULL);
    free(r->nbuf.rows);
    free(r->nbuf.off);
    free(r->nbuf.bytes);
}
