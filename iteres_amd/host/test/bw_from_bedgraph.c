/* bw_from_bedgraph.c — test tool: feeds a bedGraph ("chrom start end value" lines) and a chromosome size file to the product's
 * sparse bigWig writer (bw_sparse.c write_bigwig_sparse), so the writer can be checked on a machine without a GPU.
 *   bw_from_bedgraph <in.bedGraph> <chrom.sizes> <out.bigWig>
 * Status 255 and no file when the bedGraph has no line, as the reference's converter ends. */
#define _GNU_SOURCE
#include "../itx_host.h"

#include <stdlib.h>
#include <string.h>

static char **names;
static uint32_t *sizes, *rank_of;
static size_t n_names;

static int by_name(const void *a, const void *b) { return strcmp(names[*(const uint32_t *)a], names[*(const uint32_t *)b]); }
static int by_place(const void *a, const void *b)
{
    const bw_item *x = a, *y = b;
    if (rank_of[x->chrom] != rank_of[y->chrom]) return rank_of[x->chrom] < rank_of[y->chrom] ? -1 : 1;
    return x->start < y->start ? -1 : x->start > y->start;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: bw_from_bedgraph <in.bedGraph> <chrom.sizes> <out.bigWig>\n");
        return 2;
    }
    char *line = NULL, name[1024];
    size_t lcap = 0, cap = 0;
    FILE *f = fopen(argv[2], "r");
    if (!f) return 3;
    while (getline(&line, &lcap, f) >= 0) {
        unsigned long size;
        if (sscanf(line, "%1023s %lu", name, &size) != 2) continue;
        if (n_names == cap) {
            cap = cap ? cap * 2 : 64;
            names = realloc(names, cap * sizeof *names);
            sizes = realloc(sizes, cap * sizeof *sizes);
        }
        names[n_names] = strdup(name);
        sizes[n_names++] = (uint32_t)size;
    }
    fclose(f);
    f = fopen(argv[1], "r");
    if (!f) return 3;
    bw_item *it = NULL;
    size_t n = 0, icap = 0;
    while (getline(&line, &lcap, f) >= 0) {
        unsigned long s, e;
        double v;
        if (sscanf(line, "%1023s %lu %lu %lf", name, &s, &e, &v) != 4) continue;
        size_t c = 0;
        while (c < n_names && strcmp(names[c], name)) c++;
        if (c == n_names) die("%s is not in %s", name, argv[2]);
        if (n == icap) {
            icap = icap ? icap * 2 : 4096;
            it = realloc(it, icap * sizeof *it);
        }
        it[n++] = (bw_item){(uint32_t)c, (uint32_t)s, (uint32_t)e, (float)v};      /* lineFileNeedDouble, then the packed float */
    }
    fclose(f);
    /* the converter sorts the chromosomes by name and a chromosome's items by start */
    uint32_t *order = malloc((n_names + 1) * sizeof *order);
    rank_of = malloc((n_names + 1) * sizeof *rank_of);
    for (size_t c = 0; c < n_names; c++) order[c] = (uint32_t)c;
    qsort(order, n_names, sizeof *order, by_name);
    for (size_t c = 0; c < n_names; c++) rank_of[order[c]] = (uint32_t)c;
    qsort(it, n, sizeof *it, by_place);
    if (!write_bigwig_sparse(argv[3], (const char *const *)names, sizes, it, n)) {
        fprintf(stderr, "%s is empty of data\n", argv[1]);
        return 255;
    }
    return 0;
}
