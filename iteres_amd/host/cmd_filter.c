/* cmd_filter.c — `iteres filter`: same options, banners, output names and exit codes as filter.c:30-161 of the
 * reference; per-locus counting runs on the GPU engine (stream.c). */
#define _GNU_SOURCE
#include "itx_host.h"

#include <getopt.h>
#include <libgen.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static int filter_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Obtain alignment statistics of individual loci of each repeat subfamily, family or class.\n\n");
    fprintf(stderr, "Usage:   iteres filter [options] <chromosome size file> <repeat size file> <rmsk.txt> <bam/sam alignment file>\n\n");
    fprintf(stderr, "Options: -S       input is SAM [off]\n");
    fprintf(stderr, "         -Q       mapping Quality threshold [10]\n");
    fprintf(stderr, "         -g       coverage threshold for overlapping [0.0001]\n");
    fprintf(stderr, "         -N       normalized by number of (0: non-redundant unique mapped reads, 1: unique reads, 2: mapped reads, 3: total reads) [0])\n");
    fprintf(stderr, "         -n       use repName (subfamily) as filter [null]\n");
    fprintf(stderr, "         -f       use repFamily as filter [null]\n");
    fprintf(stderr, "         -c       use repClass as filter [null]\n");
    fprintf(stderr, "         -t       only output repeats have more than [1] reads mapped\n");
    fprintf(stderr, "         -r       output the list of reads [off]\n");
    fprintf(stderr, "         -b       output the counted reads as <prefix>_<filter>.iteres.bam, every one of them whatever -t says; BAM input only (an extension: not in the reference) [off]\n");
    fprintf(stderr, "         -i       with -b: also write its index <prefix>_<filter>.iteres.bam.bai, for coordinate-sorted input (an extension) [off]\n");
    fprintf(stderr, "         -s       with -b: write the counted reads sorted by coordinate, so that -i works on input in any order (an extension) [off]\n");
    fprintf(stderr, "         -l       with -b: level of its BGZF members, 0 (stored), 1 (fast) or 6 (smallest) (an extension) [6]\n");
    fprintf(stderr, "         -a       with -b: tag every emitted read with the repeat it was counted for, ZN/ZC/ZF (repName, repClass, repFamily) and ZS/ZE (genoStart, genoEnd) (an extension) [off]\n");
    fprintf(stderr, "         -m       with -b -s: also write the mate of every counted pair, found on the device among the reads that were not counted (an extension) [off]\n");
    fprintf(stderr, "         -G       output the genome coverage of the counted reads as <prefix>_<filter>.iteres.bedGraph and, for MAPQ >= -Q, .iteres.unique.bedGraph (an extension) [off]\n");
    fprintf(stderr, "         -W       output that genome coverage as bigWig, <prefix>_<filter>.iteres.bigWig and .iteres.unique.bigWig, with or without -G (an extension) [off]\n");
    fprintf(stderr, "         -R       remove redundant reads [off]\n");
    fprintf(stderr, "         -T       treat 1 paired-end read as 2 single-end reads [off]\n");
    fprintf(stderr, "         -D       discard if only one end mapped in a paired end reads [off]\n");
    fprintf(stderr, "         -C       Add 'chr' string as prefix of reference sequence [off]\n");
    fprintf(stderr, "         -E       extend reads to represent fragment [150], specify 0 if want no extension\n");
    fprintf(stderr, "         -I       Insert length threshold [500]\n");
    fprintf(stderr, "         -o       output prefix [basename of input without extension]\n");
    fprintf(stderr, "         -h       help message\n");
    fprintf(stderr, "         -?       help message\n");
    fprintf(stderr, "\n");
    return 1;
}

int main_filter(int argc, char **argv)
{
    run_opts o;
    memset(&o, 0, sizeof o);
    o.mapq = 10;
    o.isize = 500;
    o.extension = 150;
    o.min_cov = 0.0001f;
    int optthreshold = 1, optreadlist = 0, optbam = 0, optindex = 0, optsort = 0, optlevel = -1, optannotate = 0, optmates = 0, optgcov = 0, optbigwig = 0, optNorm = 0, c, filterField = 0;
    char *optoutput = NULL, *optname = NULL, *optclass = NULL, *optfamily = NULL;
    const time_t start_time = time(NULL);
    while ((c = getopt(argc, argv, "SQ:g:N:n:c:t:f:rbisl:amGWRTDCE:I:o:h?")) >= 0) {
        switch (c) {
        case 'S': o.is_sam = 1; break;
        case 'Q': o.mapq = (unsigned)strtol(optarg, 0, 0); break;
        case 'g': o.min_cov = (float)atof(optarg); break;
        case 'N': optNorm = (int)(unsigned)strtol(optarg, 0, 0); break;
        case 't': optthreshold = (int)(unsigned)strtol(optarg, 0, 0); break;
        case 'r': optreadlist = 1; break;
        case 'b': optbam = 1; break;
        case 'i': optindex = 1; break;
        case 's': optsort = 1; break;
        case 'a': optannotate = 1; break;
        case 'm': optmates = 1; break;
        case 'G': optgcov = 1; break;
        case 'W': optbigwig = 1; break;
        case 'l': {
            char *end = NULL;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || (v != 0 && v != 1 && v != 6)) die("-l takes the level of the BAM's members, 0 (stored), 1 (fast) or 6 (the default): not '%s'", optarg);
            optlevel = (int)v;
            break;
        }
        case 'R': o.dedup = 1; break;
        case 'T': o.treat = 1; break;
        case 'D': o.discard = 1; break;
        case 'C': o.add_chr = 1; break;
        case 'n': optname = strdup(optarg); break;
        case 'c': optclass = strdup(optarg); break;
        case 'f': optfamily = strdup(optarg); break;
        case 'E': o.extension = (unsigned)strtol(optarg, 0, 0); break;
        case 'I': o.isize = (unsigned)strtol(optarg, 0, 0); break;
        case 'o': optoutput = strdup(optarg); break;
        case 'h':
        case '?': return filter_usage();
        default: return 1;
        }
    }
    if (optind + 4 > argc) return filter_usage();
    /* -b (an extension) copies records out of the BAM windows the device decoded: there are none for SAM text, nor when the host inflates */
    if (optbam && o.is_sam) die("-b writes BAM records as they lie in the input: it cannot be combined with -S (SAM text has none)");
    if (optindex && !optbam) die("-i writes the index of the BAM that -b writes: it cannot be used without -b");
    if (optsort && !optbam) die("-s sorts the BAM that -b writes: it cannot be used without -b");
    if (optlevel >= 0 && !optbam) die("-l chooses the level of the BAM that -b writes: it cannot be used without -b");
    if (optannotate && !optbam) die("-a tags the reads of the BAM that -b writes: it cannot be used without -b");
    if (optmates && !optbam) die("-m adds the mates to the BAM that -b -s writes: it cannot be used without -b");
    if (optmates && !optsort) die("-m gives a mate its place in the sorted BAM of -b -s: it cannot be used without -s");
    if (optmates && o.treat) die("-m completes the pairs counted through their READ1: it cannot be combined with -T, which counts both ends on their own");
    if (optbam && getenv("ITX_HOST_INFLATE"))
        die("-b gathers the records on the device, where the BAM is decoded: it cannot be combined with ITX_HOST_INFLATE (the host decoder)");
    o.chr_size_file = argv[optind];
    o.rep_size_file = argv[optind + 1];
    o.rmsk_file = argv[optind + 2];
    o.aln_arg = argv[optind + 3];
    if ((optname && optclass) || (optname && optfamily) || (optclass && optfamily))
        die("Please specify only one filter, either -n, -c or -f.");
    int nindex = 0;
    if (optNorm == 0) nindex = 7;
    else if (optNorm == 1) nindex = 8;
    else if (optNorm == 2) nindex = 6;
    else if (optNorm == 3) nindex = 4;
    else die("Wrong normalization method specified");
    const char *subfam = "ALL";
    if (optname) { subfam = optname; filterField = 10; }
    else if (optclass) { subfam = optclass; filterField = 11; }
    else if (optfamily) { subfam = optfamily; filterField = 12; }
    if (strcmp(subfam, "ALL") == 0) {
        fprintf(stderr, "* You didn't specify any filter, will output all repeats\n");
        filterField = 0;
    }
    char *output;
    if (optoutput) {
        output = optoutput;
    } else {
        char *copy = xstrdup(o.aln_arg);
        output = filename_without_ext(basename(copy));
        free(copy);
    }

    /* what is order-dependent stays with one rank: -R, the read-name lists (-r), the emitted BAM (-b), SAM text; so
     * does the genome coverage (-G, -W), whose dense arrays are not reduced across ranks */
    const int splittable = !o.is_sam && !o.dedup && !optreadlist && !optbam && !optgcov && !optbigwig;
    o.gcov = optgcov || optbigwig;                /* -W accumulates the coverage -G accumulates, whether or not its text is wanted */
    multi_begin(splittable, o.aln_arg, 0);
    /* (-b: the records parsed ahead are kept as 14 bytes each, their bytes are gone) */
    stream_prefetch_allow(&o, 1, splittable);
    char *outBam = NULL;
    if (optbam) {
        if (asprintf(&outBam, "%s_%s.iteres.bam", output, subfam) < 0) die("Preparing output wrong");
        o.bam_out_path = outBam;
        o.bam_index = optindex;
        o.bam_sort = optsort;
        o.bam_annotate = optannotate;
        o.bam_mates = optmates;
        o.bam_level_given = optlevel >= 0;
        o.bam_level = optlevel >= 0 ? optlevel : 6;
        aln_keep_header(1);                      /* before the helper thread opens the file */
    }
    gpu_warmup_start(!o.is_sam, o.aln_arg, 0, splittable);
    sizes_t chr_sizes, rep_sizes;
    sizes_load(o.chr_size_file, &chr_sizes);
    stream_sizes_ready(&chr_sizes);
    sizes_load(o.rep_size_file, &rep_sizes);
    fprintf(stderr, "* Start to parse the rmsk file\n");
    rmsk_t rm;
    rmsk_load(o.rmsk_file, &chr_sizes, &rep_sizes, filterField, subfam, &rm);
    if (filterField == 0) {
        fprintf(stderr, "* Total %d repeats found.\n", rm.repeat_num);
    } else {
        if (rm.repeat_num <= 0) die("* No repeats found related to [%s], typo? or specify wrong repName/Class/Family filter?", subfam);
        fprintf(stderr, "* Total %d repeats for [%s].\n", rm.repeat_num, subfam);
    }
    /* the .loci order depends on the table alone: its sort runs on the device beside the scan (rank 0 writes the files) */
    loci_dev *ldev = multi_rank() == 0 ? loci_dev_begin(&rm, ITX_LOCI_FILTER, optreadlist, multi_device()) : NULL;
    fprintf(stderr, "* Start to parse the SAM/BAM file\n");
    itx_engine *eng = NULL;
    itx_table *tab = NULL;
    char **locus_names = NULL;
    host_counts hc = {0, 0};
    run_stream(&o, &rm, &chr_sizes, 1, 0, 10000, optreadlist, &eng, &tab, optreadlist ? &locus_names : NULL, &hc);

    fprintf(stderr, "* Preparing the output file\n");
    char *out = NULL, *outReport = NULL;
    if (asprintf(&out, "%s_%s.iteres.loci", output, subfam) < 0) die("Preparing output wrong");
    if (asprintf(&outReport, "%s_%s.iteres.reportloci", output, subfam) < 0) die("Preparing output wrong");
    uint64_t cnt[13];
    itx_result res;
    memset(&res, 0, sizeof res);
    res.cnt = cnt;
    res.locus_cnt = xcalloc(rm.n_rows + 1, sizeof(uint32_t));
    if (stream_finish(eng, &res) != ITX_OK) die("itx_engine_finish: %s", itx_last_error());
    cnt[11] -= hc.dup_unique;                     /* reads_nonredundant_unique: -R duplicates never reach it (generic.c:524-539) */
    const uint32_t *names_cnt = stream_names_counts();
    if (names_cnt)                                /* the lists came from the device: one name per counted read, or something is wrong */
        for (size_t r = 0; r < rm.n_rows; r++)
            if (names_cnt[r] != res.locus_cnt[r])
                die("read lists: row %zu has %u names but %u counted reads (ITX_HOST_NAMES=1 builds the lists on the host)", r, names_cnt[r], res.locus_cnt[r]);
    write_filter_out(&rm, res.locus_cnt, locus_names, out, optreadlist, optthreshold, subfam, cnt[nindex], ldev);
    if (optgcov || optbigwig) {
        char *text[2] = {NULL, NULL}, *bw[2] = {NULL, NULL};
        if (asprintf(&text[0], "%s_%s.iteres.bedGraph", output, subfam) < 0) die("Preparing output wrong");
        if (asprintf(&text[1], "%s_%s.iteres.unique.bedGraph", output, subfam) < 0) die("Preparing output wrong");
        if (asprintf(&bw[0], "%s_%s.iteres.bigWig", output, subfam) < 0) die("Preparing output wrong");
        if (asprintf(&bw[1], "%s_%s.iteres.unique.bigWig", output, subfam) < 0) die("Preparing output wrong");
        stream_gcov_write(&chr_sizes, optgcov ? (const char *const *)text : NULL, optbigwig ? (const char *const *)bw : NULL);
        for (int w = 0; w < 2; w++) {
            free(text[w]);
            free(bw[w]);
        }
    }
    loci_dev_free(ldev);
    if (names_cnt) {
        stream_names_free(locus_names);
    } else if (locus_names) {
        for (size_t r = 0; r < rm.n_rows; r++) free(locus_names[r]);
        free(locus_names);
    }
    fprintf(stderr, "* Preparing report file\n");
    write_report(outReport, cnt, o.mapq, subfam);
    itx_engine_destroy(eng);
    itx_table_destroy(tab);
    rmsk_free(&rm);
    sizes_free(&chr_sizes);
    sizes_free(&rep_sizes);
    fprintf(stderr, "* Done, time used %.0f seconds.\n", difftime(time(NULL), start_time));
    return 0;
}
