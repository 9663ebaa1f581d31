/* writers.c — the output files, byte for byte as the reference writes them: the report (generic.c:53-70), the
 * three stat tables and the two wig files (generic.c:72-113), the per-locus table (generic.c:1709-1746).
 * Row order is the iteration order of the reference's hashes (names_kent_order) and, inside a chromosome,
 * binKeeperNext's order: bins ascending, newest insertion first (cuskent/binRange.c:365-392). */
#define _GNU_SOURCE
#include "itx_host.h"
#include "../csrc/itx_lociline.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

double cal_rpkm(unsigned long long reads_count, unsigned long long total_length, unsigned long long mapped_reads_num)
{
    return itx_loci_rpkm(reads_count, total_length, mapped_reads_num);
}

double cal_rpm(unsigned long long reads_count, unsigned long long mapped_reads_num)
{
    return itx_loci_rpm(reads_count, mapped_reads_num);
}

static FILE *must_open(const char *path, const char *mode)
{
    FILE *f = fopen(path, mode);
    if (!f) die("mustOpen: Can't open %s to write: %s", path, strerror(errno));      /* cuskent/common.c mustOpen */
    return f;
}

void write_report(const char *path, const uint64_t *cnt, unsigned mapQ, const char *subfam)
{
    FILE *f = must_open(path, "w");
    fprintf(f, "total reads (pair): %llu\n", (unsigned long long)cnt[0]);
    fprintf(f, "mappable reads (pair): %llu\n", (unsigned long long)cnt[6]);
    fprintf(f, "uniquely mapped reads (pair) (mapQ >= %u): %llu\n", mapQ, (unsigned long long)cnt[7]);
    fprintf(f, "non-redundant uniquely mapped reads (pair): %llu\n", (unsigned long long)cnt[11]);
    fprintf(f, "mapped reads (pair) overlap with repeats but discarded due to mapped to different subfamilies: %llu\n",
            (unsigned long long)cnt[12]);
    fprintf(f, "mapped reads (pair) overlap with [%s] repeats: %llu\n", subfam, (unsigned long long)cnt[9]);
    fprintf(f, "uniquely mapped reads (pair) overlap with [%s] repeats: %llu\n", subfam, (unsigned long long)cnt[10]);
    fclose(f);
}

/* "%u\n" */
static inline char *put_u32_line(char *p, uint32_t v)
{
    char t[10];
    int n = 0;
    do {
        t[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) *p++ = t[--n];
    *p++ = '\n';
    return p;
}

void write_wig_and_stat(const rmsk_t *rm, const itx_result *res, const uint64_t *cov_off, const char *f_stat, const char *f_wig,
                        const char *f_fam, const char *f_cla, const char *f_wig_uniq, unsigned long long reads_num,
                        unsigned long long reads_num_unique)
{
    const uint32_t S = rm->reps.n, F = rm->fams.n, C = rm->clas.n;
    uint32_t *order = xmalloc(sizeof(uint32_t) * (S + F + C + 1));
    FILE *f1 = must_open(f_stat, "w");
    FILE *f2 = f_wig ? must_open(f_wig, "w") : NULL;
    FILE *f5 = f_wig_uniq ? must_open(f_wig_uniq, "w") : NULL;
    fprintf(f1, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", "#subfamily", "family", "class", "consensus_length", "reads_count",
            "unique_reads_count", "total_length", "genome_count", "all_reads_RPKM", "all_reads_RPM", "unique_reads_RPKM",
            "unique_reads_RPM");
    names_kent_order(&rm->reps, 12, order);
    for (uint32_t k = 0; k < S; k++) {
        const uint32_t r = order[k];
        const unsigned long long rc = res->rep_cnt[r], ru = res->rep_cnt[S + r], tl = rm->rep_total[r];
        fprintf(f1, "%s\t%s\t%s\t%u\t%llu\t%llu\t%llu\t%llu\t%.3f\t%.3f\t%.3f\t%.3f\n", rm->reps.name[r], rm->fams.name[rm->rep_fam[r]],
                rm->clas.name[rm->rep_cla[r]], rm->rep_len[r], rc, ru, tl, (unsigned long long)rm->rep_genome[r],
                cal_rpkm(rc, tl, reads_num), cal_rpm(rc, reads_num), cal_rpkm(ru, tl, reads_num_unique), cal_rpm(ru, reads_num_unique));
    }
    /* the two wigs (generic.c:83-90), same order: one "%u\n" per base. The blocks are formatted in parallel, a group of
     * names at a time, and written in order. */
    if (f2 && f5) {
        enum { GROUP = 512 };
        char *buf[2][GROUP];
        size_t len[2][GROUP];
        for (uint32_t k0 = 0; k0 < S; k0 += GROUP) {
            const uint32_t k1 = k0 + GROUP < S ? k0 + GROUP : S;
#pragma omp parallel for schedule(dynamic, 4)
            for (long k = (long)k0; k < (long)k1; k++) {
                const uint32_t r = order[k];
                for (int w = 0; w < 2; w++) {
                    buf[w][k - k0] = NULL;
                    len[w][k - k0] = 0;
                    if (rm->rep_len[r] == 0) continue;
                    const uint32_t *v = (w ? res->cov_uniq : res->cov) + cov_off[r];
                    char *b = xmalloc(64 + strlen(rm->reps.name[r]) + 11 * (size_t)rm->rep_len[r]);
                    char *p = b + sprintf(b, "fixedStep chrom=%s start=1 step=1 span=1\n", rm->reps.name[r]);
                    for (uint32_t m = 0; m < rm->rep_len[r]; m++) p = put_u32_line(p, v[m]);
                    buf[w][k - k0] = b;
                    len[w][k - k0] = (size_t)(p - b);
                }
            }
            for (uint32_t k = k0; k < k1; k++) {
                if (buf[0][k - k0]) fwrite(buf[0][k - k0], 1, len[0][k - k0], f2);
                if (buf[1][k - k0]) fwrite(buf[1][k - k0], 1, len[1][k - k0], f5);
                free(buf[0][k - k0]);
                free(buf[1][k - k0]);
            }
        }
    }
    if (f2) fclose(f2);
    fclose(f1);
    if (f5) fclose(f5);
    FILE *f3 = must_open(f_fam, "w");
    fprintf(f3, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", "#family", "class", "reads_count", "unique_reads_count", "total_length",
            "genome_count", "all_reads_RPKM", "all_reads_RPM", "unique_reads_RPKM", "unique_reads_RPM");
    names_kent_order(&rm->fams, 12, order);
    for (uint32_t k = 0; k < F; k++) {
        const uint32_t r = order[k];
        const unsigned long long rc = res->fam_cnt[r], ru = res->fam_cnt[F + r], tl = rm->fam_total[r];
        fprintf(f3, "%s\t%s\t%llu\t%llu\t%llu\t%llu\t%.3f\t%.3f\t%.3f\t%.3f\n", rm->fams.name[r], rm->clas.name[rm->fam_cla[r]], rc, ru, tl,
                (unsigned long long)rm->fam_genome[r], cal_rpkm(rc, tl, reads_num), cal_rpm(rc, reads_num),
                cal_rpkm(ru, tl, reads_num_unique), cal_rpm(ru, reads_num_unique));
    }
    fclose(f3);
    FILE *f4 = must_open(f_cla, "w");
    fprintf(f4, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", "#class", "reads_count", "unique_reads_count", "total_length", "genome_count",
            "all_reads_RPKM", "all_reads_RPM", "unique_reads_RPKM", "unique_reads_RPM");
    names_kent_order(&rm->clas, 12, order);
    for (uint32_t k = 0; k < C; k++) {
        const uint32_t r = order[k];
        const unsigned long long rc = res->cla_cnt[r], ru = res->cla_cnt[C + r], tl = rm->cla_total[r];
        fprintf(f4, "%s\t%llu\t%llu\t%llu\t%llu\t%.3f\t%.3f\t%.3f\t%.3f\n", rm->clas.name[r], rc, ru, tl, (unsigned long long)rm->cla_genome[r],
                cal_rpkm(rc, tl, reads_num), cal_rpm(rc, reads_num), cal_rpkm(ru, tl, reads_num_unique), cal_rpm(ru, reads_num_unique));
    }
    fclose(f4);
    free(order);
}

struct lo {
    int bin;
    uint32_t row;
};
static int lo_cmp(const void *a, const void *b)
{
    const struct lo *x = a, *y = b;
    if (x->bin != y->bin) return x->bin < y->bin ? -1 : 1;
    return x->row > y->row ? -1 : (x->row < y->row ? 1 : 0);      /* list head = newest insertion (binRange.c:185) */
}

/* hashRmsk's chromosome order, for the host's walk and for the device's sort key alike: corder[k] = the chromosome at place k
 * (NC + 1 elements), rank[c] = the place of chromosome c (NULL: not wanted) */
static void loci_chrom_order(const rmsk_t *rm, uint32_t *corder, uint32_t *rank)
{
    names_kent_order(&rm->chroms, 12, corder);                  /* hashRmsk = newHash(0): 2^12 buckets */
    if (rank)
        for (uint32_t k = 0; k < rm->chroms.n; k++) rank[corder[k]] = k;
}

/* The loci of a table in binKeeper order: hashRmsk's chromosome order, and for every chromosome its rows with their bin numbers
 * (itx_loci_bin of ../csrc/itx_lociline.h), to be sorted by lo_cmp (cuskent/binRange.c:365-392). */
static struct lo *loci_prepare(const rmsk_t *rm, uint32_t **corder_out, size_t **cnt_out, size_t **beg_out)
{
    const uint32_t NC = rm->chroms.n;
    uint32_t *corder = xmalloc(sizeof(uint32_t) * (NC + 1));
    loci_chrom_order(rm, corder, NULL);
    /* rows per chromosome */
    size_t *cnt = xcalloc(NC + 1, sizeof(size_t)), *beg = xcalloc(NC + 2, sizeof(size_t));
    for (size_t r = 0; r < rm->n_rows; r++) cnt[rm->row_chrom_name[r]]++;
    for (uint32_t c = 0; c < NC; c++) beg[c + 1] = beg[c] + cnt[c];
    struct lo *lo = xmalloc(sizeof *lo * (rm->n_rows ? rm->n_rows : 1));
    size_t *fill = xmalloc(sizeof(size_t) * (NC + 1));
    memcpy(fill, beg, sizeof(size_t) * (NC + 1));
    for (size_t r = 0; r < rm->n_rows; r++) {
        struct lo *e = &lo[fill[rm->row_chrom_name[r]]++];
        e->bin = itx_loci_bin((int)rm->rows[r].start, (int)rm->rows[r].end);
        e->row = (uint32_t)r;
    }
    free(fill);
    *corder_out = corder;
    *cnt_out = cnt;
    *beg_out = beg;
    return lo;
}

/* ---- the device route (include/iteres_amd.h itx_loci_*): the order is sorted on the device from the moment the table is known, the
 * lines are formatted there from the counts. Which route writes the file when ITX_HOST_LOCI is not set: the device route becomes the
 * default only on a measurement of the whole command ("The .loci file on the device"); until one exists the host writes
 * it, as before. ITX_HOST_LOCI=0 asks for the device route, ITX_HOST_LOCI=1 for the host's. filter -r stays with the host: its
 * lists are in host memory. */
struct loci_dev {
    itx_loci *obj;
    int timing;
    char why[160];               /* why the host writes the file ("": the device does) */
};

void loci_name_table(const names_t *t, char **bytes, uint64_t **off)
{
    uint64_t *o = xmalloc(sizeof(uint64_t) * ((size_t)t->n + 1));
    o[0] = 0;
    for (uint32_t i = 0; i < t->n; i++) o[i + 1] = o[i] + strlen(t->name[i]);
    char *b = xmalloc(o[t->n] + 1);
    for (uint32_t i = 0; i < t->n; i++) memcpy(b + o[i], t->name[i], o[i + 1] - o[i]);
    *bytes = b;
    *off = o;
}

loci_dev *loci_dev_begin(const rmsk_t *rm, int kind, int readlist, int device)
{
    loci_dev *d = xcalloc(1, sizeof *d);
    const char *e = getenv("ITX_HOST_LOCI");
    d->timing = getenv("ITX_TIMING") != NULL;
    if (readlist) snprintf(d->why, sizeof d->why, "-r: the read lists are in host memory");
    else if (!e || !*e) snprintf(d->why, sizeof d->why, "ITX_HOST_LOCI is not set: the host is the default");
    else if (atoi(e) != 0) snprintf(d->why, sizeof d->why, "ITX_HOST_LOCI=%s", e);
    if (d->why[0]) return d;
    const uint32_t NC = rm->chroms.n;
    uint32_t *corder = xmalloc(sizeof(uint32_t) * (NC + 1)), *rank = xmalloc(sizeof(uint32_t) * (NC + 1));
    loci_chrom_order(rm, corder, rank);
    const names_t *tabs[4] = {&rm->chroms, &rm->reps, &rm->clas, &rm->fams};
    char *nb[4];
    uint64_t *no[4];
    for (int t = 0; t < 4; t++) loci_name_table(tabs[t], &nb[t], &no[t]);
    /* writeFilterOut generic.c:1709-1746 / writeFilterOutMRE generic.c:1748-1772: the walk over hashRmsk and its binKeepers */
    const int rc = itx_loci_create(device, kind, rm->rows, rm->row_chrom_name, rm->n_rows, rank, NC, nb[0], no[0], nb[1], no[1], rm->reps.n, nb[2], no[2], rm->clas.n,
                                   nb[3], no[3], rm->fams.n, &d->obj);
    if (rc == ITX_E_RANGE) snprintf(d->why, sizeof d->why, "ITX_E_RANGE: the table does not fit the device's sort key");
    else if (rc == ITX_E_NOMEM) snprintf(d->why, sizeof d->why, "ITX_E_NOMEM: the device cannot hold the table");
    else chk(rc, "itx_loci_create");
    for (int t = 0; t < 4; t++) {
        free(nb[t]);
        free(no[t]);
    }
    free(corder);
    free(rank);
    return d;
}

void loci_dev_free(loci_dev *d)
{
    if (!d) return;
    itx_loci_destroy(d->obj);
    free(d);
}

/* after a text call: 1 when the device's text is the file's body (then the timing line is printed here) */
static int loci_dev_took(loci_dev *d, int rc, const itx_loci_text *tx, double waited)
{
    if (rc == ITX_E_NOMEM) {
        snprintf(d->why, sizeof d->why, "ITX_E_NOMEM: no room for the text");
        return 0;
    }
    chk(rc, "itx_loci text");
    if (tx->hard) {
        snprintf(d->why, sizeof d->why, "%llu lines hold a number the device does not print: not finite, or 2^63 and above", (unsigned long long)tx->hard);
        return 0;
    }
    if (d->timing)
        fprintf(stderr, "[itx timing] loci: %llu lines built on the device (%llu bytes, sort %.3f ms, text %.3f ms, host waited %.3f s)\n",
                (unsigned long long)tx->lines, (unsigned long long)tx->bytes, tx->sort_ms, tx->text_ms, waited);
    return 1;
}

static void loci_dev_host_wrote(const loci_dev *d, int lines)
{
    if (d && d->timing) fprintf(stderr, "[itx timing] loci: %d lines written by the host (%s)\n", lines, d->why);
}

void write_filter_out(const rmsk_t *rm, const uint32_t *locus_cnt, char **locus_names, const char *path, int readlist, int threshold,
                      const char *subfam, unsigned long long reads_num, loci_dev *dev)
{
    FILE *out = must_open(path, "w");
    int j = 0;
    if (readlist)
        fprintf(out, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", "#chr", "start", "end", "length", "repName", "repClass", "repFamily",
                "readsCount", "RPKM", "RPM", "readsList");
    else
        fprintf(out, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", "#chr", "start", "end", "length", "repName", "repClass", "repFamily",
                "readsCount", "RPKM", "RPM");
    if (dev && dev->obj && !readlist) {
        itx_loci_text tx;
        const double t0 = now_s();
        const int rc = itx_loci_filter_text(dev->obj, locus_cnt, threshold, reads_num, &tx);
        if (loci_dev_took(dev, rc, &tx, now_s() - t0)) {
            if (tx.bytes && fwrite(tx.text, 1, tx.bytes, out) != tx.bytes) die("%s: %s", path, strerror(errno));
            fclose(out);
            fprintf(stderr, "* Total %d [%s] TEs have at least %d reads mapped.\n", (int)tx.lines, subfam, threshold);
            return;
        }
    }
    const uint32_t NC = rm->chroms.n;
    uint32_t *corder;
    size_t *cnt, *beg;
    struct lo *lo = loci_prepare(rm, &corder, &cnt, &beg);
    for (uint32_t k = 0; k < NC; k++) {
        const uint32_t c = corder[k];
        qsort(lo + beg[c], cnt[c], sizeof *lo, lo_cmp);
        for (size_t i = beg[c]; i < beg[c] + cnt[c]; i++) {
            const uint32_t r = lo[i].row;
            const itx_row *os = &rm->rows[r];
            const int count = (int)locus_cnt[r];
            if (count < threshold) continue;
            j++;
            const unsigned length = os->end - os->start;
            /* filter by name: rows carry no name ids (the hashes stay empty): the strings come from the filter itself */
            fprintf(out, "%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%.3f\t%.3f", rm->chroms.name[c], (int)os->start, (int)os->end, (int)length,
                    rm->reps.name[os->rep], rm->clas.name[os->cla], rm->fams.name[os->fam], count,
                    cal_rpkm((unsigned long long)count, (unsigned long long)length, reads_num), cal_rpm((unsigned long long)count, reads_num));
            if (readlist) fprintf(out, "\t%s", locus_names && locus_names[r] ? locus_names[r] : "");
            fputc('\n', out);
        }
    }
    fclose(out);
    fprintf(stderr, "* Total %d [%s] TEs have at least %d reads mapped.\n", j, subfam, threshold);
    loci_dev_host_wrote(dev, j);
    free(lo);
    free(cnt);
    free(beg);
    free(corder);
}

/* writeFilterOutMRE, generic.c:1748-1772 */
void write_cpg_loci(const rmsk_t *rm, const int *cpg_count, const double *cpg_total, const char *path, const char *subfam, double threshold, loci_dev *dev)
{
    FILE *out = must_open(path, "w");
    int j = 0;
    fprintf(out, "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", "#chr", "start", "end", "length", "repName", "repClass", "repFamily", "covered_CpG_site",
            "total_CpG_score");
    if (dev && dev->obj) {
        itx_loci_text tx;
        const double t0 = now_s();
        const int rc = itx_loci_cpg_text(dev->obj, cpg_count, cpg_total, threshold, &tx);
        if (loci_dev_took(dev, rc, &tx, now_s() - t0)) {
            if (tx.bytes && fwrite(tx.text, 1, tx.bytes, out) != tx.bytes) die("%s: %s", path, strerror(errno));
            fclose(out);
            fprintf(stderr, "* Total %d [%s] TEs have CpG score larger than %.3f.\n", (int)tx.lines, subfam, threshold);
            return;
        }
    }
    const uint32_t NC = rm->chroms.n;
    uint32_t *corder;
    size_t *cnt, *beg;
    struct lo *lo = loci_prepare(rm, &corder, &cnt, &beg);
    for (uint32_t k = 0; k < NC; k++) {
        const uint32_t c = corder[k];
        qsort(lo + beg[c], cnt[c], sizeof *lo, lo_cmp);
        for (size_t i = beg[c]; i < beg[c] + cnt[c]; i++) {
            const uint32_t r = lo[i].row;
            const itx_row *os = &rm->rows[r];
            if (!(cpg_total[r] > threshold)) continue;
            j++;
            fprintf(out, "%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%.3f\n", rm->chroms.name[c], (int)os->start, (int)os->end, (int)(os->end - os->start),
                    rm->reps.name[os->rep], rm->clas.name[os->cla], rm->fams.name[os->fam], cpg_count[r], cpg_total[r]);
        }
    }
    fclose(out);
    fprintf(stderr, "* Total %d [%s] TEs have CpG score larger than %.3f.\n", j, subfam, threshold);
    loci_dev_host_wrote(dev, j);
    free(lo);
    free(cnt);
    free(beg);
    free(corder);
}
