/* bw_sum.c — a bigWig's zoom summaries (cuskent/bbiWrite.c:370-446). Where a summary starts and ends is decided here; what an item
 * adds to the open one is csrc/itx_bwfold.h, which the device builders run too. */
#include "bw_priv.h"

/* ---- cuskent/bbiWrite.c:370-421 bbiAddToSummary, the list kept as an array whose last element is the open summary */
void add_to_summary(bw_sumlist *L, uint32_t chrom_id, uint32_t chrom_size, uint32_t start, uint32_t end, uint32_t valid_count, double min_val,
                    double max_val, double sum_data, double sum_squares, int reduction)
{
    if (end > chrom_size) end = chrom_size;
    while (start < end) {
        bw_summary *sum = L->n ? &L->v[L->n - 1] : NULL;
        if (!sum || sum->chrom_id != chrom_id || sum->end <= start) {
            if (L->n == L->cap) {
                L->cap = L->cap ? L->cap * 2 : 1024;
                L->v = xrealloc(L->v, L->cap * sizeof *L->v);
                sum = L->n ? &L->v[L->n - 1] : NULL;
            }
            bw_summary nw;
            nw.chrom_id = chrom_id;
            if (!sum || sum->chrom_id != chrom_id || sum->end + (uint32_t)reduction <= start)
                nw.start = start;
            else
                nw.start = sum->end;
            nw.end = nw.start + (uint32_t)reduction;
            if (nw.end > chrom_size) nw.end = chrom_size;
            itx_bwfold_open(&nw, min_val, max_val);
            L->v[L->n++] = nw;
            sum = &L->v[L->n - 1];
        }
        /* rangeIntersection, cuskent/common.c:2824-2831 */
        const int s = (int)(start > sum->start ? start : sum->start), e = (int)(end < sum->end ? end : sum->end);
        const int overlap = e - s;
        if (overlap <= 0) die("internal error: bigWig summary item %u %u does not intersect %u %u", start, end, sum->start, sum->end);
        const int item_size = (int)(end - start);
        itx_bwfold_add(sum, (double)overlap / item_size, (double)valid_count, min_val, max_val, sum_data, sum_squares);
        start += (uint32_t)overlap;
    }
}

/* Summaries never span two chromosomes (a new one starts whenever the chromosome id changes, bbiWrite.c:381), so the
 * chromosomes are reduced independently, in parallel, and their lists joined in order: same numbers, same order. */
static void sumlist_join(bw_sumlist *out, bw_sumlist *parts, size_t n_parts)
{
    size_t total = 0;
    for (size_t i = 0; i < n_parts; i++) total += parts[i].n;
    out->v = xmalloc((total ? total : 1) * sizeof *out->v);
    out->n = out->cap = total;
    size_t at = 0;
    for (size_t i = 0; i < n_parts; i++) {
        if (parts[i].n) memcpy(out->v + at, parts[i].v, parts[i].n * sizeof *out->v);
        at += parts[i].n;
        free(parts[i].v);
    }
    free(parts);
}

/* cuskent/bwgCreate.c:751-795: every base of every section, as a one-base range (bbiAddRangeToSummary, bbiWrite.c:424-433) */
bw_sumlist reduce_sections(const bw_section *sec, const size_t *sec_of, const bw_chrom *chroms, size_t n_chroms, int reduction)
{
    bw_sumlist *parts = xcalloc(n_chroms ? n_chroms : 1, sizeof *parts);
#pragma omp parallel for schedule(dynamic, 8)
    for (long c = 0; c < (long)n_chroms; c++) {
        bw_sumlist L = {NULL, 0, 0};
        for (size_t k = sec_of[c]; k < sec_of[c + 1]; k++) {
            const uint32_t chrom_size = chroms[sec[k].chrom_id].size;
            uint32_t start = sec[k].start;
            const float *vals = sec[k].val;
            const uint32_t n_items = sec[k].item_count;
            uint32_t i = 0;
            while (i < n_items) {
                if (start >= chrom_size) break;                         /* add_to_summary clips end to the chromosome: nothing is added */
                bw_summary *sum = L.n ? &L.v[L.n - 1] : NULL;
                if (!sum || sum->chrom_id != sec[k].chrom_id || sum->end <= start) {
                    const double v0 = (double)vals[i];
                    add_to_summary(&L, sec[k].chrom_id, chrom_size, start, start + 1, 1u, v0, v0, v0, v0 * v0, reduction);   /* opens the summary */
                    start += 1;
                    i++;
                    continue;
                }
                /* the open summary takes every base up to its end: add_to_summary for one-base items (overlap == item size == 1,
                 * f = 1.0) without the call and its loop per base */
                uint32_t upto = sum->end - start;
                if (upto > n_items - i) upto = n_items - i;
                bw_summary a = *sum;                                    /* (a local copy: the loop keeps it in registers) */
                for (uint32_t j = 0; j < upto; j++) {
                    const double val = (double)vals[i + j];
                    itx_bwfold_add(&a, 1.0, 1.0, val, val, val, val * val);
                }
                *sum = a;
                start += upto;
                i += upto;
            }
        }
        parts[c] = L;
    }
    bw_sumlist out;
    sumlist_join(&out, parts, n_chroms);
    return out;
}

/* cuskent/bbiWrite.c:435-446 */
bw_sumlist reduce_summaries(const bw_sumlist *in, const bw_chrom *chroms, size_t n_chroms, int reduction)
{
    /* first summary of every chromosome in the input list (ids ascend) */
    size_t *first = xcalloc(n_chroms + 2, sizeof *first);
    {
        size_t c = 0;
        for (size_t i = 0; i < in->n; i++)
            while (c <= in->v[i].chrom_id) first[c++] = i;
        while (c <= n_chroms) first[c++] = in->n;
    }
    bw_sumlist *parts = xcalloc(n_chroms ? n_chroms : 1, sizeof *parts);
#pragma omp parallel for schedule(dynamic, 8)
    for (long c = 0; c < (long)n_chroms; c++) {
        bw_sumlist L = {NULL, 0, 0};
        for (size_t i = first[c]; i < first[c + 1]; i++) {
            const bw_summary *s = &in->v[i];
            add_to_summary(&L, s->chrom_id, chroms[s->chrom_id].size, s->start, s->end, s->valid_count, s->min_val, s->max_val, s->sum_data,
                           s->sum_squares, reduction);
        }
        parts[c] = L;
    }
    free(first);
    bw_sumlist out;
    sumlist_join(&out, parts, n_chroms);
    return out;
}
