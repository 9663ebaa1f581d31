/* bw_sparse.c — sparse data: the bigWig of a bedGraph (filter -W). What bigWigFileCreate makes of bedGraph lines (sections of
 * <= itemsPerSlot items of type bwgTypeBedGraph, cuskent/bwgCreate.c:470-575): only chromosomes with an item get an id (:584-627), the
 * levels are csrc/itx_bwzoomrule.h with the average resolution of :629-686, and the summaries follow the data: they start where it
 * starts and re-anchor after a gap (bw_sum.c add_to_summary states the rule). */
#include "bw_priv.h"

typedef struct {
    const bw_item *it;
    const ritem *sec;
    const size_t *first;              /* section i holds items first[i] .. first[i + 1] */
} bw_sparse_ctx;

static uint32_t fill_bedgraph(const void *ctx, size_t i, char *buf)
{
    const bw_sparse_ctx *C = ctx;
    const size_t a = C->first[i], b = C->first[i + 1];
    char *w = put_section_header(buf, C->sec[i].chrom, C->sec[i].start, C->sec[i].end, 0, 0, 1, (uint16_t)(b - a));     /* bwgTypeBedGraph */
    for (size_t k = a; k < b; k++) {
        memcpy(w, &C->it[k].start, 4); w += 4;
        memcpy(w, &C->it[k].end, 4); w += 4;
        memcpy(w, &C->it[k].val, 4); w += 4;
    }
    return (uint32_t)(w - buf);
}

/* the chromosomes that get an id: used[k] != 0, in the order given (strcmp order of the names) */
static bw_chrom *sparse_chroms(const char *const *names, const uint32_t *sizes, const uint32_t *pick, size_t n, uint32_t *max_name)
{
    bw_chrom *ch = xcalloc(n ? n : 1, sizeof *ch);
    *max_name = 0;
    for (size_t i = 0; i < n; i++) {
        ch[i].name = names[pick[i]];
        ch[i].id = (uint32_t)i;
        ch[i].size = sizes[pick[i]];
        const uint32_t l = (uint32_t)strlen(ch[i].name);
        if (l > *max_name) *max_name = l;
        if (i && strcmp(ch[i - 1].name, ch[i].name) >= 0) die("internal error: bigWig chromosomes %s, %s are not in strcmp order", ch[i - 1].name, ch[i].name);
    }
    return ch;
}

int write_bigwig_sparse(const char *path, const char *const *names, const uint32_t *sizes, const bw_item *items, size_t n_items)
{
    const uint32_t items_per_slot = BW_ITEMS_PER_SLOT;
    if (!n_items) return 0;
    BW_T("start");
    /* ids, and the items with them */
    uint32_t *pick = xcalloc(n_items, sizeof *pick);
    bw_item *it = xmalloc(n_items * sizeof *it);
    size_t n_ids = 0;
    for (size_t k = 0; k < n_items; k++) {
        if (!k || items[k].chrom != items[k - 1].chrom) pick[n_ids++] = items[k].chrom;
        else if (items[k].start < items[k - 1].end) die("Overlap between %s %u %u and %u %u", names[items[k].chrom], items[k - 1].start, items[k - 1].end, items[k].start, items[k].end);
        if (items[k].start >= items[k].end || items[k].end > sizes[items[k].chrom]) die("bedGraph item %s %u %u is empty or ends behind the chromosome's %u bases", names[items[k].chrom], items[k].start, items[k].end, sizes[items[k].chrom]);
        it[k] = items[k];
        it[k].chrom = (uint32_t)(n_ids - 1);
    }
    uint32_t max_name = 0;
    bw_chrom *chroms = sparse_chroms(names, sizes, pick, n_ids, &max_name);
    /* sections */
    size_t n_sec = 0;
    for (size_t k = 0, run = 0; k < n_items; k++) {
        if (k && it[k].chrom != it[k - 1].chrom) run = 0;
        if (run++ % items_per_slot == 0) n_sec++;
    }
    ritem *sec = xcalloc(n_sec, sizeof *sec);
    size_t *first = xcalloc(n_sec + 1, sizeof *first);
    uint64_t total_res = 0, full_size = 0;
    {
        size_t s = 0;
        for (size_t k = 0, run = 0; k < n_items; k++) {
            if (k && it[k].chrom != it[k - 1].chrom) run = 0;
            if (run++ % items_per_slot == 0) first[s++] = k;
        }
        first[n_sec] = n_items;
        for (s = 0; s < n_sec; s++) {
            int res = 0x3fffffff;                                           /* BIGNUM */
            for (size_t k = first[s]; k < first[s + 1]; k++)
                if (res > (int)(it[k].end - it[k].start)) res = (int)(it[k].end - it[k].start);
            total_res += (uint64_t)res;
            sec[s].chrom = it[first[s]].chrom;
            sec[s].start = it[first[s]].start;
            sec[s].end = it[first[s + 1] - 1].end;
            full_size += 24 + 12 * (uint64_t)(first[s + 1] - first[s]);
        }
    }
    const int min_res = (int)((total_res + (uint32_t)n_sec / 2) / (uint32_t)n_sec);
    itx_bwzoom Z;
    bw_sumlist L = {NULL, 0, 0}, kept;
    const bw_summary *sum[ITX_BWZ_MAX_LEVELS];
    uint64_t n_sum[ITX_BWZ_MAX_LEVELS];
    int w = itx_bwzoom_init(&Z, full_size, min_res, n_ids);
    while (w == ITX_BWZ_COUNT) {
        free(L.v);
        L = (bw_sumlist){NULL, 0, 0};
        for (size_t k = 0; k < n_items; k++) {
            const int size = (int)(it[k].end - it[k].start);
            const double v = (double)it[k].val, sd = size * v;
            add_to_summary(&L, it[k].chrom, chroms[it[k].chrom].size, it[k].start, it[k].end, (uint32_t)size, v, v, sd, sd * v, (int)Z.red);
        }
        w = itx_bwzoom_first(&Z, L.n);
    }
    if (w == ITX_BWZ_RANGE) die("%s: a first reduction of %lld", path, Z.red);
    sum[0] = L.v;
    n_sum[0] = L.n;
    kept = L;                                                               /* the last level kept: the next one's source */
    while (itx_bwzoom_next(&Z)) {
        L = reduce_summaries(&kept, chroms, n_ids, (int)Z.red);
        if (itx_bwzoom_keep(&Z, L.n)) {
            kept = L;
            sum[Z.n_levels - 1] = L.v;
            n_sum[Z.n_levels - 1] = L.n;
        } else
            free(L.v);
    }
    const int n_sums = Z.n_levels;
    BW_T("zoom lists");
    bw_file F;
    bw_file_begin(&F, path, n_sums, Z.reduction, chroms, n_ids, max_name, n_sec);
    const bw_sparse_ctx ctx = {it, sec, first};
    const uint32_t unc_buf = put_blocks_zlib(F.f, sec, n_sec, 1, 24 + 12 * (size_t)items_per_slot, 4096, fill_bedgraph, &ctx);
    bw_file_end(&F, sec, n_sec, sum, n_sum, n_sums, unc_buf, NULL, NULL);
    for (int i = 0; i < n_sums; i++) free((void *)sum[i]);
    free(first);
    free(sec);
    free(chroms);
    free(it);
    free(pick);
    return 1;
}

int write_bigwig_sparse_device(const char *path, const char *const *names, const uint32_t *sizes, const itx_gcov_bw_result *dev)
{
    if (!dev->n_items) return 0;
    uint32_t max_name = 0;
    bw_chrom *chroms = sparse_chroms(names, sizes, dev->chrom, dev->n_chrom, &max_name);
    const size_t n_sec = (size_t)dev->n_sec;
    bw_file F;
    bw_file_begin(&F, path, (int)dev->n_levels, dev->reduction, chroms, dev->n_chrom, max_name, n_sec);
    ritem *sec = xcalloc(n_sec ? n_sec : 1, sizeof *sec);
    uint32_t unc_buf = 0;
    for (size_t i = 0; i < n_sec; i++) {
        sec[i].chrom = dev->sec_key[3 * i];
        sec[i].start = dev->sec_key[3 * i + 1];
        sec[i].end = dev->sec_key[3 * i + 2];
        if (24 + 12 * dev->sec_count[i] > unc_buf) unc_buf = 24 + 12 * dev->sec_count[i];
    }
    const bw_blocks blocks = {dev->blocks, dev->block_off};
    put_device_blocks(F.f, &blocks, 0, sec, n_sec, 1);
    bw_file_end(&F, sec, n_sec, dev->sum, dev->n_sum, (int)dev->n_levels, unc_buf, &blocks, dev->slot_first);
    free(sec);
    free(chroms);
    return 1;
}
