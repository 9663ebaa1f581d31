/* bw_priv.h — between the four files that write bigWig files (itx_host.h has what the commands call): bigwig.c is the file (skeleton,
 * B+ tree, R trees, deflated blocks), bw_sum.c the zoom summaries, bw_dense.c the writers of data that covers every base (stat,
 * cpgstat), bw_sparse.c those of bedGraph items (filter -W). Which levels a file gets is csrc/itx_bwzoomrule.h, run by both. */
#ifndef ITX_BW_PRIV_H
#define ITX_BW_PRIV_H
#include "itx_host.h"
#include <stdlib.h>
#include <string.h>
#include "../csrc/itx_bwfold.h"
#include "../csrc/itx_bwzoomrule.h"

#define BW_ITEMS_PER_SLOT 1024u         /* stat.c:157-158 */
#define BW_BLOCK_SIZE 256u

typedef itx_bw_summary bw_summary;      /* a zoom record as the file holds it, and as the device hands it out */

typedef struct {
    bw_summary *v;                      /* the last element is the open summary */
    size_t n, cap;
} bw_sumlist;
typedef struct {
    const char *name;
    uint32_t id, size;
} bw_chrom;
typedef struct {
    uint32_t chrom_id, start, end, item_count;
    const float *val;                   /* item_count values, as a fixed-step section stores them */
} bw_section;
typedef struct {                        /* what the R tree indexes: a section, or a zoom record */
    uint32_t chrom, start, end;
    uint64_t off;
} ritem;
typedef struct {                        /* blocks the device deflated, packed: block i at bytes [off[i], off[i + 1]) */
    const uint8_t *bytes;
    const uint64_t *off;
} bw_blocks;

/* ---- bw_sum.c */
void add_to_summary(bw_sumlist *L, uint32_t chrom_id, uint32_t chrom_size, uint32_t start, uint32_t end, uint32_t valid_count, double min_val,
                    double max_val, double sum_data, double sum_squares, int reduction);
/* sec_of[c] .. sec_of[c + 1]: the sections of chromosome c */
bw_sumlist reduce_sections(const bw_section *sec, const size_t *sec_of, const bw_chrom *chroms, size_t n_chroms, int reduction);
bw_sumlist reduce_summaries(const bw_sumlist *in, const bw_chrom *chroms, size_t n_chroms, int reduction);

/* ---- bigwig.c: bw_file_begin writes everything up to the section count, the caller lays its sections down (put_blocks_zlib or
 * put_device_blocks, which record where), bw_file_end writes the index, the zoom levels and the numbers that are known only then */
typedef struct {
    FILE *f;
    const char *path;
    long chrom_tree_pos, data_pos, index_pos, total_pos, unc_pos, zoom_pos[ITX_BWZ_MAX_LEVELS];
    uint64_t total_summary_off;
} bw_file;

void bw_file_begin(bw_file *F, const char *path, int n_levels, const uint32_t *reductions, const bw_chrom *chroms, size_t n_chroms, uint32_t max_name,
                   uint64_t section_count);
/* sec[i]: section i's key and offset; unc_buf: the largest payload; dev: the zoom blocks (NULL: zlib), level k's from slot_first[k] */
void bw_file_end(bw_file *F, const ritem *sec, size_t n_sec, const bw_summary *const *sum, const uint64_t *n_sum, int n_levels, uint32_t unc_buf,
                 const bw_blocks *dev, const uint64_t *slot_first);
/* Blocks (sections, or a zoom level's records) laid down one after the other; block i holds items i * per .. of the n, which get
 * its file offset. put_blocks_zlib deflates them in parallel into memory, `group` at a time: fill(ctx, i, buf) writes block i's payload
 * (at most cap bytes) and returns its length; the largest is returned. put_device_blocks takes the device's, from block `first` on. */
typedef uint32_t (*bw_fill_fn)(const void *ctx, size_t i, char *buf);
uint32_t put_blocks_zlib(FILE *f, ritem *items, size_t n, uint32_t per, size_t cap, size_t group, bw_fill_fn fill, const void *ctx);
void put_device_blocks(FILE *f, const bw_blocks *dev, uint64_t first, ritem *items, size_t n, uint32_t per);
char *put_section_header(char *w, uint32_t chrom_id, uint32_t start, uint32_t end, uint32_t step, uint32_t span, uint8_t type, uint16_t cnt);
/* ITX_TIMING_BW: the time since the last call, on stderr */
void bw_tick(const char *what);
#define BW_T(x) bw_tick(x)

#endif
