/* oracle/bamcheck.c — a small driver of our own over the reference's BAM library (the samtools 0.1.18 it vendors, built by
 * oracle/Makefile into _ref/libbam.a). It calls the library's entry points and holds none of its code; the tests hand it files
 * the product wrote and compare what the library makes of them with the Python restatements (tests/baicase.py and the stable sort).
 *
 *   bamcheck index <bam>                    <bam>.bai by bam_index_build
 *   bamcheck sort  <bam> <prefix>           <prefix>.bam by bam_sort_core, by coordinate, one in-memory run
 *   bamcheck view  <bam>                    header and records as SAM text; exit 1 when reading stops with an error
 *   bamcheck fetch <bam> <tid> <beg> <end>  the records of [beg, end) (0-based, half open) on reference tid, found through
 *                                           <bam>.bai by bam_index_load and bam_fetch, as SAM text
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sam.h"

/* bam_sort.c defines it; no header of the library declares it */
void bam_sort_core(int is_by_qname, const char *fn, const char *prefix, size_t max_mem);

#define SORT_MEM ((size_t)1 << 30)      /* the records of a test input stay far below it: one run, no temporary files, no merge */

static int usage(void)
{
    fprintf(stderr, "usage: bamcheck index <bam> | sort <bam> <prefix> | view <bam> | fetch <bam> <tid> <beg> <end>\n");
    return 2;
}

static int do_view(const char *fn)
{
    samfile_t *in = samopen(fn, "rb", 0), *out;
    bam1_t *b;
    int ret;
    if (in == 0 || in->header == 0) {
        fprintf(stderr, "bamcheck view: cannot open %s\n", fn);
        return 1;
    }
    out = samopen("-", "wh", in->header);
    if (out == 0) return 1;
    b = bam_init1();
    while ((ret = samread(in, b)) >= 0) samwrite(out, b);
    bam_destroy1(b);
    samclose(out);
    samclose(in);
    if (ret < -1) {                        /* -1: the end of the file; below it: a record that breaks off or does not parse */
        fprintf(stderr, "bamcheck view: reading %s stopped with %d\n", fn, ret);
        return 1;
    }
    return 0;
}

struct fetch_out { bam_header_t *header; };

static int print_one(const bam1_t *b, void *data)
{
    char *s = bam_format1(((struct fetch_out*)data)->header, b);
    puts(s);
    free(s);
    return 0;
}

static int do_fetch(const char *fn, int tid, int beg, int end)
{
    struct fetch_out fo;
    bam_index_t *idx;
    bamFile fp = bam_open(fn, "r");
    int ret;
    if (fp == 0) {
        fprintf(stderr, "bamcheck fetch: cannot open %s\n", fn);
        return 1;
    }
    fo.header = bam_header_read(fp);
    idx = bam_index_load(fn);
    if (fo.header == 0 || idx == 0) return 1;
    if (tid < 0 || tid >= fo.header->n_targets) {
        fprintf(stderr, "bamcheck fetch: no reference %d in %s\n", tid, fn);
        return 1;
    }
    ret = bam_fetch(fp, idx, tid, beg, end, &fo, print_one);
    bam_index_destroy(idx);
    bam_header_destroy(fo.header);
    bam_close(fp);
    if (ret < -1) {
        fprintf(stderr, "bamcheck fetch: reading %s stopped with %d\n", fn, ret);
        return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return usage();
    if (!strcmp(argv[1], "index") && argc == 3) return bam_index_build(argv[2]) == 0 ? 0 : 1;
    if (!strcmp(argv[1], "sort") && argc == 4) {
        bam_sort_core(0, argv[2], argv[3], SORT_MEM);
        return 0;
    }
    if (!strcmp(argv[1], "view") && argc == 3) return do_view(argv[2]);
    if (!strcmp(argv[1], "fetch") && argc == 6) return do_fetch(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    return usage();
}
