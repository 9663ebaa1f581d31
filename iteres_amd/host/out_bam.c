/* out_bam.c — the BAM of filter -b (with -i its index, -s sorted, -m with the counted pairs' mates, -a annotated, -l the level), as stream.c's record loop feeds it (the
 * steps: stream_priv.h). The members are made on the device (csrc/itx_bamout.hip); this file sets the object up from the kept header,
 * hands it the host route's records and writes what comes back. */
#define _GNU_SOURCE
#include "stream_priv.h"
#include "../csrc/itx_bamsortrule.h"
#include "../csrc/itx_reptag.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

/* filter -b: the members of the batches that wait (all but the newest `keep`) are fetched and written, oldest first */
static void bam_write_out(stream_run *r, int keep)
{
    while (itx_bamout_pending(r->bo) > keep) {
        itx_bamout_members m;
        chk(itx_bamout_collect(r->bo, &m), "itx_bamout_collect");
        if (m.len && fwrite(m.bytes, 1, m.len, r->bam_f) != m.len) die("writing %s: %s", r->o->bam_out_path, strerror(errno));
    }
}

/* the kept header (magic, l_text, text, reference list): the length of its text, which lies at hb + 8 with n_ref right behind it */
static size_t bam_header_text(const stream_run *r, const uint8_t *hb, size_t hl)
{
    int32_t l_text = 0;
    if (hl >= 8) memcpy(&l_text, hb + 4, 4);
    if (hl < 12 || l_text < 0 || (size_t)l_text > hl - 12) die("%s: the kept BAM header is cut short", r->o->bam_out_path);
    return (size_t)l_text;
}

/* filter -b -i: the index is built beside the stream (csrc/itx_bamidx.hip). The reference lengths of the kept header size its linear
 * part; the first record member starts where the header's members end. */
static void bam_index_begin(stream_run *r, const uint8_t *hb, size_t hl)
{
    int32_t n_ref = 0;
    size_t at = 8 + bam_header_text(r, hb, hl);
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
    const size_t l_text = bam_header_text(r, hb, hl);
    uint8_t *nb = xcalloc(hl + ITX_BAMSORT_HEADER_GROWTH, 1);
    const size_t nl = itx_bamsort_header_text((const char *)hb + 8, l_text, (char *)nb + 8);
    if (nl > INT32_MAX) die("%s: a header text of %zu bytes", r->o->bam_out_path, nl);
    const int32_t nl32 = (int32_t)nl;
    memcpy(nb, hb, 4);
    memcpy(nb + 4, &nl32, 4);
    memcpy(nb + 8 + nl, hb + 8 + l_text, hl - 8 - l_text);
    *out_len = hl - l_text + nl;
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
void bam_host_batch(stream_run *r, int k)
{
    if (!r->bo) return;
    const itx_staging *st = &r->st[k];
    const aln_side *side = &r->side[k];
    const rmsk_t *rm = r->rm;
    size_t b = 0, n_hit = 0;
    const int want_rows = r->o->bam_mates && r->o->bam_annotate;          /* -m -a: a host-route READ1's mate takes the tags of its row */
    for (size_t i = 0; i < r->pend[k]; i++) {
        if (st->hit_row[i] < 0) continue;
        if (want_rows) {
            if (r->brows_cap <= n_hit) {
                r->brows_cap = (n_hit + 1) * 2;
                r->brows = xrealloc(r->brows, r->brows_cap * sizeof(int32_t));
            }
            r->brows[n_hit] = st->hit_row[i];
        }
        n_hit++;
        uint32_t bs;
        memcpy(&bs, side->raw + side->raw_off[i], 4);
        size_t len = 4 + (size_t)bs;
        ItxRepTag t = {0};
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
    if (want_rows && n_hit) chk(itx_bamout_mates_host_rows(r->bo, r->brows, n_hit), "itx_bamout_mates_host_rows");
    chk(itx_bamout_append_host(r->bo, r->bbuf.bytes, b), "itx_bamout_append_host");
    if (r->o->bam_mates && r->pend[k]) {
        /* -m: every record of the window, counted or not, as the reader kept its bytes: the candidates among them join the store.
         * The slot's records lie one behind the other as they did in the file; were they ever kept apart, they are laid together first. */
        const size_t lo = side->raw_off[0];
        size_t at = lo;
        int together = 1;
        for (size_t i = 0; i < r->pend[k]; i++) {
            uint32_t bs;
            if (side->raw_off[i] != at) together = 0;
            memcpy(&bs, side->raw + side->raw_off[i], 4);
            at = side->raw_off[i] + 4 + (size_t)bs;
        }
        if (together) {
            chk(itx_bamout_mates_append_host(r->bo, side->raw + lo, at - lo), "itx_bamout_mates_append_host");
        } else {
            b = 0;
            for (size_t i = 0; i < r->pend[k]; i++) {
                uint32_t bs;
                memcpy(&bs, side->raw + side->raw_off[i], 4);
                if (r->bbuf.cap < b + 4 + (size_t)bs) {
                    r->bbuf.cap = (b + 4 + (size_t)bs) * 2;
                    r->bbuf.bytes = xrealloc(r->bbuf.bytes, r->bbuf.cap);
                }
                memcpy(r->bbuf.bytes + b, side->raw + side->raw_off[i], 4 + (size_t)bs);
                b += 4 + (size_t)bs;
            }
            chk(itx_bamout_mates_append_host(r->bo, r->bbuf.bytes, b), "itx_bamout_mates_append_host");
        }
    }
    bam_write_out(r, 1);
}

/* The emitted BAM starts with the first file's header as it was read (magic, text, reference list), in members of the host's; the
 * object is made behind it */
void bam_open(stream_run *r, stream_file *f)
{
    const run_opts *o = r->o;
    if (!r->bam_f || r->bam_header_done) return;
    size_t hl = 0;
    const uint8_t *hb = aln_header_bytes(f->rd, &hl);
    if (!r->h->inflater || o->is_sam || !hb) die("filter -b needs BAM input decoded on the device: %s", r->h->err[0] ? r->h->err : "the decoder is not in use");
    uint8_t *sorted_hb = o->bam_sort ? bam_sorted_header(r, hb, hl, &hl) : NULL;
    if (sorted_hb) hb = sorted_hb;
    if (bgzf_write_members(r->bam_f, hb, hl) != 0) die("writing %s: %s", o->bam_out_path, strerror(errno));
    r->bam_header_done = 1;
    chk(itx_bamout_create(multi_device(), BATCH_RECORDS, 0, &r->bo), "itx_bamout_create");
    if (o->bam_level_given) chk(itx_bamout_set_level(r->bo, o->bam_level), "itx_bamout_set_level");
    if (o->bam_sort) chk(itx_bamout_sort_enable(r->bo), "itx_bamout_sort_enable");
    if (o->bam_mates) chk(itx_bamout_mates_enable(r->bo), "itx_bamout_mates_enable");
    if (o->bam_annotate) bam_annotate_begin(r);
    if (o->bam_index) bam_index_begin(r, hb, hl);
    free(sorted_hb);
}

int bam_rows(stream_run *r, int32_t **hits, void **stream)
{
    if (!r->bo) return 0;
    *hits = itx_bamout_hits(r->bo);
    *stream = itx_bamout_stream(r->bo);
    return 1;
}

/* The members of the batch before this one are written to the file while this one's kernels run. */
void bam_device_batch(stream_run *r, stream_file *f, const itx_batch *db, size_t n, chosen_rows *rows)
{
    if (!r->bo) return;
    batch_rows(r, db, n, rows);
    if (aln_device_bamout(f->rd, r->bo, n, rows->hits, rows->stream) != 0) die("device BAM output: %s", itx_last_error());
    r->bam_dev_batches++;
    bam_write_out(r, 1);
}

void bam_window_done(stream_run *r)
{
    if (r->bo) chk(itx_bamout_wait_kernels(r->bo), "itx_bamout_wait_kernels");
}

/* filter -b: the last, short member, the EOF marker, the index, and the counters for ITX_TIMING */
void bam_finish(stream_run *r)
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
    itx_bamout_mates_stats ms;
    memset(&ms, 0, sizeof ms);
    if (r->bo && r->o->bam_mates) {
        chk(itx_bamout_mates_get_stats(r->bo, &ms), "itx_bamout_mates_get_stats");
        if (ms.wanted > ms.found) fprintf(stderr, "[iteres] %llu counted pairs have no mate in the input\n", (unsigned long long)(ms.wanted - ms.found));
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
        fprintf(stderr, "[itx timing] bam out: %llu records, %llu payload bytes, %llu members (%llu bytes), %.3f ms in the gather kernels, %.3f ms in the member kernels, host waited %.3f s, %llu batches gathered on the device, %llu batches by the host route",
                (unsigned long long)bs.records, (unsigned long long)bs.payload_bytes, (unsigned long long)bs.members, (unsigned long long)bs.out_bytes, bs.gather_ms,
                bs.member_ms, 1e-3 * bs.wait_ms, r->bam_dev_batches, r->bam_host_batches);
        /* one line: each option that is on adds its piece, in this order */
        if (r->o->bam_annotate) {
            uint64_t tb = 0;
            if (r->bo) chk(itx_bamout_annotate_get_stats(r->bo, &tb), "itx_bamout_annotate_get_stats");
            fprintf(stderr, ", %llu tag bytes appended", (unsigned long long)tb + r->bam_host_tag_bytes);
        }
        if (r->o->bam_sort) {
            itx_bamout_sort_stats ss;
            memset(&ss, 0, sizeof ss);
            if (r->bo) chk(itx_bamout_sort_get_stats(r->bo, &ss), "itx_bamout_sort_get_stats");
            fprintf(stderr, "; sort: %llu records sorted, %llu rounds, %.3f ms in the sort kernels, %.3f ms in the replay gathers", (unsigned long long)ss.records,
                    (unsigned long long)ss.rounds, ss.sort_ms, ss.replay_ms);
        }
        if (r->o->bam_mates)
            fprintf(stderr, "; mates: %llu candidates held (%llu bytes), %llu wanted, %llu found, %.3f ms in the candidate gathers, %.3f ms in the join",
                    (unsigned long long)ms.candidates, (unsigned long long)ms.candidate_bytes, (unsigned long long)ms.wanted, (unsigned long long)ms.found, ms.gather_ms, ms.join_ms);
        if (r->o->bam_index)
            fprintf(stderr, "; index: %llu entries, %llu chunks, %llu bytes, %.3f ms in the entry kernels, %.3f ms in the final kernels", (unsigned long long)ir.entries,
                    (unsigned long long)ir.chunks, (unsigned long long)ir.len, ir.batch_ms, ir.finish_ms);
        /* -l: the level the writer used; without -l the line is the one it was before there were levels */
        if (r->o->bam_level_given) fprintf(stderr, ", level %d", r->bo ? itx_bamout_get_level(r->bo) : r->o->bam_level);
        fprintf(stderr, "\n");
    }
    itx_bamout_destroy(r->bo);
    r->bo = NULL;
}

void bam_free(stream_run *r)
{
    free(r->bbuf.bytes);
    free(r->brows);
}
