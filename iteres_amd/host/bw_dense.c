/* bw_dense.c — the bigWig of data that covers every sequence base by base from 0 (stat.c:156-158, cpgstat), made straight from the
 * value vectors instead of the text wig the reference converts ("fixedStep chrom=<repName> start=1 step=1 span=1" blocks). */
#include "bw_priv.h"

static int cmp_chrom_name(const void *a, const void *b)
{
    return strcmp(((const bw_chrom *)a)->name, ((const bw_chrom *)b)->name);
}

/* The layout of a file, made from the names and lengths alone: chromosomes in strcmp order (the section sort,
 * bwgCreate.c:138-151) with ids in that order (:584-627), the sections, and the zoom reductions. Both block sources —
 * zlib on the host (write_bigwig) and the device builder (write_bigwig_device) — are laid down by the one skeleton below
 * from such a plan, so their files can only differ in how the blocks are deflated. */
struct bw_plan {
    const char *wig_name;
    size_t n_names, n_sec;
    bw_chrom *chroms;
    size_t *src;                  /* chroms[i] is names[src[i]] */
    bw_section *sec;
    size_t *sec_of;
    uint32_t max_name;
    uint64_t n_first;
    int n_sums;
    uint32_t reductions[ITX_BWZ_MAX_LEVELS];
};

/* How many summaries a reduction gives needs no arithmetic on the values: every sequence is covered base by base from 0 to its
 * size, so its summaries tile it in steps of the reduction (bbiWrite.c:381-395) — and so do the summaries of the level below */
static uint64_t tiles(const bw_chrom *chroms, size_t n, long long reduction)
{
    uint64_t t = 0;
    for (size_t c = 0; c < n; c++) t += ((uint64_t)chroms[c].size + (uint64_t)reduction - 1) / (uint64_t)reduction;
    return t;
}

bw_plan *bw_plan_make(const char *wig_name, const char *const *names, const uint32_t *len, size_t n_names)
{
    const uint32_t items_per_slot = BW_ITEMS_PER_SLOT;
    if (n_names == 0) die("%s is empty of data", wig_name);                  /* bwgCreate.c:1108-1109 */
    bw_plan *P = xcalloc(1, sizeof *P);
    P->wig_name = wig_name;
    P->n_names = n_names;
    bw_chrom *chroms = xcalloc(n_names, sizeof *chroms);
    size_t *src = xcalloc(n_names, sizeof *src);
    for (size_t i = 0; i < n_names; i++) {
        chroms[i].name = names[i];
        chroms[i].id = (uint32_t)i;                                          /* borrowed as the source index until sorted */
        chroms[i].size = len[i];
    }
    qsort(chroms, n_names, sizeof *chroms, cmp_chrom_name);
    uint32_t max_name = 0;
    size_t n_sec = 0;
    for (size_t i = 0; i < n_names; i++) {
        src[i] = chroms[i].id;
        chroms[i].id = (uint32_t)i;
        const uint32_t l = (uint32_t)strlen(chroms[i].name);
        if (l > max_name) max_name = l;
        n_sec += (chroms[i].size + items_per_slot - 1) / items_per_slot;
    }
    bw_section *sec = xcalloc(n_sec ? n_sec : 1, sizeof *sec);
    size_t *sec_of = xcalloc(n_names + 1, sizeof *sec_of);
    size_t k = 0;
    uint64_t full_size = 0;
    for (size_t i = 0; i < n_names; i++) {
        sec_of[i] = k;
        for (uint32_t s = 0; s < chroms[i].size; s += items_per_slot) {
            const uint32_t c = chroms[i].size - s > items_per_slot ? items_per_slot : chroms[i].size - s;
            sec[k].chrom_id = (uint32_t)i;
            sec[k].start = s;
            sec[k].end = s + c;
            sec[k].item_count = c;
            sec[k].val = NULL;
            full_size += 24 + 4 * (uint64_t)c;
            k++;
        }
    }
    sec_of[n_names] = k;
    /* zoom levels (csrc/itx_bwzoomrule.h): step 1 everywhere, so the average resolution is 1 */
    itx_bwzoom Z;
    uint64_t n_first = 0;
    int w = itx_bwzoom_init(&Z, full_size, 1, n_names);
    while (w == ITX_BWZ_COUNT) w = itx_bwzoom_first(&Z, n_first = tiles(chroms, n_names, Z.red));
    if (w == ITX_BWZ_RANGE) die("%s: a first reduction of %lld", wig_name, Z.red);
    while (itx_bwzoom_next(&Z)) (void)itx_bwzoom_keep(&Z, tiles(chroms, n_names, Z.red));
    memcpy(P->reductions, Z.reduction, sizeof P->reductions);
    P->chroms = chroms;
    P->src = src;
    P->sec = sec;
    P->sec_of = sec_of;
    P->n_sec = n_sec;
    P->max_name = max_name;
    P->n_first = n_first;
    P->n_sums = Z.n_levels;
    return P;
}

void bw_plan_free(bw_plan *P)
{
    if (!P) return;
    free(P->sec);
    free(P->sec_of);
    free(P->src);
    free(P->chroms);
    free(P);
}

size_t bw_plan_chroms(const bw_plan *P, const size_t **src, uint32_t *size_out)
{
    for (size_t i = 0; i < P->n_names; i++) size_out[i] = P->chroms[i].size;
    *src = P->src;
    return P->n_names;
}

int bw_plan_levels(const bw_plan *P, const uint32_t **reductions)
{
    *reductions = P->reductions;
    return P->n_sums;
}

static uint32_t fill_fixed_step(const void *ctx, size_t i, char *buf)
{
    const bw_section *s = (const bw_section *)ctx + i;
    char *w = put_section_header(buf, s->chrom_id, s->start, s->end, 1, 1, 3, (uint16_t)s->item_count);      /* bwgTypeFixedStep */
    memcpy(w, s->val, 4 * (size_t)s->item_count);
    return 24 + 4 * s->item_count;
}

/* val: the values of names[i] (as the converter reads the wig's text: (float)strtod("%u" or "%.4f")), or dev: the device's build */
static void bw_write(const bw_plan *P, const char *path, const float *const *val, const itx_bw_result *dev)
{
    BW_T("start");
    const size_t n_names = P->n_names, n_sec = P->n_sec;
    const bw_chrom *chroms = P->chroms;
    const int n_sums = P->n_sums;
    const uint32_t *reductions = P->reductions;
    bw_section *sec = NULL;
    const bw_summary *sum[ITX_BWZ_MAX_LEVELS] = {NULL};
    uint64_t n_sum[ITX_BWZ_MAX_LEVELS];
    if (!dev) {
        sec = xcalloc(n_sec ? n_sec : 1, sizeof *sec);
        memcpy(sec, P->sec, n_sec * sizeof *sec);
        for (size_t i = 0; i < n_sec; i++) sec[i].val = val[P->src[sec[i].chrom_id]] + sec[i].start;
        BW_T("sections");
        bw_sumlist L = reduce_sections(sec, P->sec_of, chroms, n_names, (int)reductions[0]);
        if ((uint64_t)L.n != P->n_first) die("internal error: bigWig first zoom level has %zu summaries, %llu expected", L.n, (unsigned long long)P->n_first);
        for (int i = 0; i < n_sums; i++) {                                  /* every level is kept: each comes from the one before */
            if (i) L = reduce_summaries(&L, chroms, n_names, (int)reductions[i]);
            sum[i] = L.v;
            n_sum[i] = L.n;
        }
    }
    BW_T("zoom lists");
    bw_file F;
    bw_file_begin(&F, path, n_sums, reductions, chroms, n_names, P->max_name, n_sec);
    ritem *items = xcalloc(n_sec ? n_sec : 1, sizeof *items);
    uint32_t unc_buf = 0;
    for (size_t i = 0; i < n_sec; i++) {
        items[i].chrom = P->sec[i].chrom_id;
        items[i].start = P->sec[i].start;
        items[i].end = P->sec[i].end;
        if (24 + 4 * P->sec[i].item_count > unc_buf) unc_buf = 24 + 4 * P->sec[i].item_count;
    }
    if (dev) {
        const bw_blocks blocks = {dev->blocks, dev->block_off};
        put_device_blocks(F.f, &blocks, 0, items, n_sec, 1);
        bw_file_end(&F, items, n_sec, dev->sum, dev->n_sum, n_sums, unc_buf, &blocks, dev->slot_first);
    } else {
        unc_buf = put_blocks_zlib(F.f, items, n_sec, 1, 24 + 4 * (size_t)BW_ITEMS_PER_SLOT, 4096, fill_fixed_step, sec);
        bw_file_end(&F, items, n_sec, sum, n_sum, n_sums, unc_buf, NULL, NULL);
    }
    free(items);
    if (!dev)
        for (int i = 0; i < n_sums; i++) free((void *)sum[i]);
    free(sec);
}

void write_bigwig(const char *path, const char *wig_name, const char *const *names, const uint32_t *len, const float *const *val,
                  size_t n_names)
{
    bw_plan *P = bw_plan_make(wig_name, names, len, n_names);
    bw_write(P, path, val, NULL);
    bw_plan_free(P);
}

void write_bigwig_device(const bw_plan *P, const char *path, const itx_bw_result *dev)
{
    if ((uint64_t)dev->n_sec != (uint64_t)P->n_sec || (int)dev->n_levels != P->n_sums || dev->n_sum[0] != P->n_first)
        die("internal error: the device bigWig build does not fit the layout of %s", path);
    bw_write(P, path, NULL, dev);
}
