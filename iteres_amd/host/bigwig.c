/* bigwig.c — the bigWig files `iteres stat` leaves beside its stat files (stat.c:156-158), written straight from the
 * coverage vectors instead of re-parsing the text wig. The layout and every derived number follow what the
 * reference's converter produces for a wig of "fixedStep chrom=<repName> start=1 step=1 span=1" blocks
 * (bigWigFileCreate(wig, repSizes, blockSize 256, itemsPerSlot 1024, clip 0, compress 1)):
 *   sections        cuskent/bwgCreate.c:186-262 (<= itemsPerSlot values each), sorted by chromosome name (:138-151)
 *   chromosome ids  cuskent/bwgCreate.c:584-627, B+ tree cuskent/bPlusTree.c:419-576
 *   zoom levels     cuskent/bwgCreate.c:826-885 with the summaries of cuskent/bbiWrite.c:370-446
 *   section writer  cuskent/bwgCreate.c:45-135, zoom writer cuskent/bbiWrite.c:478-536
 *   R tree          cuskent/cirTree.c:141-367
 *   file skeleton   cuskent/bwgCreate.c:887-1019
 * Blocks are deflated with zlib's compress() like cuskent/zlibFace.c:37-50; with the same zlib the files come out
 * byte for byte the same, with another one they decode to the same content.
 * This is the file, whoever deflated its blocks; bw_priv.h says what bw_sum.c, bw_dense.c and bw_sparse.c add. */
#define _GNU_SOURCE
#include "bw_priv.h"

#include <errno.h>
#include <zlib.h>

#define BW_SIG 0x888FFC26u
#define BPT_SIG 0x78CA8C91u
#define CIR_SIG 0x2468ACE0u
#define BW_VERSION 4

_Static_assert(sizeof(bw_summary) == 32, "a zoom record is written as it lies in memory");
static void put(FILE *f, const void *p, size_t n)
{
    if (fwrite(p, 1, n, f) != n) die("mustWrite: Couldn't write to bigWig file");
}
#define PUT(f, x) put(f, &(x), sizeof(x))
static void put_zero(FILE *f, size_t n)
{
    static const char z[64] = {0};
    while (n) {
        const size_t k = n < sizeof z ? n : sizeof z;
        put(f, z, k);
        n -= k;
    }
}

/* ---- cuskent/zlibFace.c:37-56 */
static size_t z_buf_size(size_t n) { return (size_t)(1.001 * (double)n + 13); }
/* zlib's compress() with the stream kept per thread: compress() is deflateInit + deflate(Z_FINISH) + deflateEnd, and for the 4 KB
 * sections of a bigWig the 268 KB of state it allocates and clears every time are a third of its time (12 800 sections: 1.08 s
 * with compress(), 0.69 s with deflateReset on one core — the bytes are the same, the parameters being compress()'s). */
static size_t z_compress(const void *src, size_t n, void *dst, size_t cap)
{
    static __thread z_stream z;
    static __thread int z_on;
    if (!z_on) {
        memset(&z, 0, sizeof z);
        if (deflateInit(&z, Z_DEFAULT_COMPRESSION) != Z_OK) die("Couldn't zCompress %lld bytes", (long long)n);
        z_on = 1;
    } else if (deflateReset(&z) != Z_OK) {
        die("Couldn't zCompress %lld bytes", (long long)n);
    }
    z.next_in = (Bytef *)src;
    z.avail_in = (uInt)n;
    z.next_out = (Bytef *)dst;
    z.avail_out = (uInt)cap;
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) die("Couldn't zCompress %lld bytes", (long long)n);
    return cap - (size_t)z.avail_out;
}

/* ---- cuskent/cirTree.c: the index over items that carry (chromIx, start, end) and a file offset ------------------- */
typedef struct {
    uint32_t start_chrom, start_base, end_chrom, end_base;
    uint64_t start_off, end_off;
    size_t first_child, n_child;       /* children in the level below (unused at the item level) */
} rnode;

static void rnode_widen(rnode *p, const rnode *e)
{
    if (e->start_chrom < p->start_chrom) {
        p->start_chrom = e->start_chrom;
        p->start_base = e->start_base;
    } else if (e->start_chrom == p->start_chrom && e->start_base < p->start_base) {
        p->start_base = e->start_base;
    }
    if (e->end_chrom > p->end_chrom) {
        p->end_chrom = e->end_chrom;
        p->end_base = e->end_base;
    } else if (e->end_chrom == p->end_chrom && e->end_base > p->end_base) {
        p->end_base = e->end_base;
    }
}

/* cuskent/cirTree.c:338-367 with rTreeFromChromRangeArray (:141-262) and writeTreeToOpenFile (:264-336) */
static void cir_tree_write(FILE *f, const ritem *it, uint64_t n_items, uint32_t block_size, uint32_t items_per_slot, uint64_t end_file_offset)
{
    /* level 0 here = the slots (what the reference calls the first level above the leaves' items) */
    size_t n0 = (size_t)((n_items + items_per_slot - 1) / items_per_slot);
    rnode *cur = xcalloc(n0 ? n0 : 1, sizeof *cur);
    for (size_t k = 0; k < n0; k++) {
        const uint64_t i = (uint64_t)k * items_per_slot;
        uint64_t one = n_items - i;
        const int final = one <= items_per_slot;
        if (!final) one = items_per_slot;
        rnode *el = &cur[k];
        el->start_chrom = el->end_chrom = it[i].chrom;
        el->start_base = it[i].start;
        el->end_base = it[i].end;
        el->start_off = it[i].off;
        el->end_off = final ? end_file_offset : it[i + one].off;
        for (uint64_t j = 1; j < one; j++) {
            rnode key = {it[i + j].chrom, it[i + j].start, it[i + j].chrom, it[i + j].end, 0, 0, 0, 0};
            rnode_widen(el, &key);
        }
    }
    /* condense until one node is left, at least once (cirTree.c:206-259): levels[0] = root ... levels[count-1] = slots */
    rnode *levels[64];
    size_t level_n[64];
    int count = 1;
    levels[0] = cur;
    level_n[0] = n0;
    while (level_n[0] > 1 || count < 2) {
        const size_t nc = level_n[0];
        const size_t np = (nc + block_size - 1) / block_size;
        rnode *par = xcalloc(np ? np : 1, sizeof *par);
        for (size_t k = 0; k < np; k++) {
            const size_t a = k * block_size, b = a + block_size < nc ? a + block_size : nc;
            par[k] = levels[0][a];
            par[k].first_child = a;
            par[k].n_child = b - a;
            for (size_t j = a + 1; j < b; j++) rnode_widen(&par[k], &levels[0][j]);
        }
        memmove(levels + 1, levels, sizeof(levels[0]) * (size_t)count);
        memmove(level_n + 1, level_n, sizeof(level_n[0]) * (size_t)count);
        levels[0] = par;
        level_n[0] = np;
        count++;
    }
    const rnode *root = &levels[0][0];
    const uint32_t magic = CIR_SIG, reserved = 0;
    PUT(f, magic);
    PUT(f, block_size);
    PUT(f, n_items);
    PUT(f, root->start_chrom);
    PUT(f, root->start_base);
    PUT(f, root->end_chrom);
    PUT(f, root->end_base);
    PUT(f, end_file_offset);
    PUT(f, items_per_slot);
    PUT(f, reserved);
    /* offsets of the levels: every level is priced as index nodes, the leaves included (cirTree.c:276-285) */
    const uint64_t i_node = 4 + 24 * (uint64_t)block_size, l_node = 4 + 32 * (uint64_t)block_size;
    uint64_t level_off[64], off = (uint64_t)ftello(f);
    for (int i = 0; i < count; i++) {
        level_off[i] = off;
        off += level_n[i] * i_node;
    }
    /* levels 0 .. count-3 are index nodes, whose slots point at the nodes of the next level; the nodes of level count-2 are the
     * leaves, whose slots are the elements of the last level (offset and size). Empty slots are padded with 24 bytes each in
     * both, not 32 in the leaves (cirTree.c:119-122) */
    for (int i = 0; i <= count - 2; i++) {
        const uint8_t is_leaf = i == count - 2, res8 = 0;
        const uint64_t child_size = i == count - 3 ? l_node : i_node;
        uint64_t child_off = level_off[i + 1];
        for (size_t k = 0; k < level_n[i]; k++) {
            const rnode *nd = &levels[i][k];
            const uint16_t cnt = (uint16_t)nd->n_child;
            PUT(f, is_leaf);
            PUT(f, res8);
            PUT(f, cnt);
            for (size_t c = 0; c < nd->n_child; c++) {
                const rnode *el = &levels[i + 1][nd->first_child + c];
                const uint64_t size = el->end_off - el->start_off;
                PUT(f, el->start_chrom);
                PUT(f, el->start_base);
                PUT(f, el->end_chrom);
                PUT(f, el->end_base);
                if (is_leaf) {
                    PUT(f, el->start_off);
                    PUT(f, size);
                } else
                    PUT(f, child_off);
                child_off += child_size;
            }
            put_zero(f, 24 * (size_t)(block_size - cnt));
        }
        if (!is_leaf && (uint64_t)ftello(f) != level_off[i + 1]) die("Internal error: offset mismatch in the bigWig index");
    }
    for (int i = 0; i < count; i++) free(levels[i]);
}

/* ---- cuskent/bPlusTree.c:419-576 over the chromosome array (key = name padded with zeros, value = id, size) -------- */
static void bpt_write(FILE *f, const bw_chrom *chroms, uint64_t n, uint32_t block_size, uint32_t key_size)
{
    const uint32_t magic = BPT_SIG, reserved = 0, val_size = 8;
    PUT(f, magic);
    PUT(f, block_size);
    PUT(f, key_size);
    PUT(f, val_size);
    PUT(f, n);
    PUT(f, reserved);
    PUT(f, reserved);
    uint64_t index_offset = (uint64_t)ftello(f);
    int levels = 1;
    for (uint64_t c = n; c > block_size; c = (c + block_size - 1) / block_size) levels++;
    char *key = xcalloc(key_size + 1, 1);
    for (int level = levels - 1; level > 0; level--) {
        uint64_t slot_per = 1;
        for (int i = 0; i < level; i++) slot_per *= block_size;
        const uint64_t node_per = slot_per * block_size;
        const uint64_t node_count = (n + node_per - 1) / node_per;
        const uint64_t in_index = 4 + (uint64_t)block_size * (key_size + 8), in_leaf = 4 + (uint64_t)block_size * (key_size + val_size);
        const uint64_t next_block = level == 1 ? in_leaf : in_index;
        /* the reference passes the running offset through a 32-bit parameter (bPlusTree.c:431); a chromosome tree
         * never gets there */
        uint64_t next_child = (uint64_t)(uint32_t)index_offset + node_count * in_index;
        for (uint64_t i = 0; i < n; i += node_per) {
            uint64_t count_one = (n - i + slot_per - 1) / slot_per;
            if (count_one > block_size) count_one = block_size;
            const uint8_t is_leaf = 0, res8 = 0;
            const uint16_t c16 = (uint16_t)count_one;
            PUT(f, is_leaf);
            PUT(f, res8);
            PUT(f, c16);
            uint64_t end_ix = i + node_per;
            if (end_ix > n) end_ix = n;
            for (uint64_t j = i; j < end_ix; j += slot_per) {
                memset(key, 0, key_size);
                strcpy(key, chroms[j].name);
                put(f, key, key_size);
                PUT(f, next_child);
                next_child += next_block;
            }
            put_zero(f, (size_t)(block_size - count_one) * (key_size + 8));
        }
        index_offset = (uint64_t)ftello(f);
    }
    uint64_t left = n;
    for (uint64_t i = 0; i < n;) {
        const uint16_t count_one = (uint16_t)(left > block_size ? block_size : left);
        const uint8_t is_leaf = 1, res8 = 0;
        PUT(f, is_leaf);
        PUT(f, res8);
        PUT(f, count_one);
        for (uint16_t j = 0; j < count_one; j++) {
            memset(key, 0, key_size);
            strcpy(key, chroms[i + j].name);
            put(f, key, key_size);
            PUT(f, chroms[i + j].id);
            PUT(f, chroms[i + j].size);
        }
        put_zero(f, (size_t)(block_size - count_one) * (key_size + val_size));
        left -= count_one;
        i += count_one;
    }
    free(key);
}

void put_device_blocks(FILE *f, const bw_blocks *dev, uint64_t first, ritem *items, size_t n, uint32_t per)
{
    for (size_t i = 0; i < n; i += per) {
        const uint64_t b = first + i / per, pos = (uint64_t)ftello(f);
        for (size_t k = i; k < n && k < i + per; k++) items[k].off = pos;
        put(f, dev->bytes + dev->off[b], (size_t)(dev->off[b + 1] - dev->off[b]));
    }
}

uint32_t put_blocks_zlib(FILE *f, ritem *items, size_t n, uint32_t per, size_t cap, size_t group, bw_fill_fn fill, const void *ctx)
{
    const size_t n_blocks = (n + per - 1) / per, ccap = z_buf_size(cap);
    const int chunk = (int)(group / 256);
    char *comp = xmalloc(ccap * group);
    size_t *csize = xcalloc(group, sizeof *csize);
    uint32_t unc_buf = 0;
    for (size_t g0 = 0; g0 < n_blocks; g0 += group) {
        const size_t g1 = g0 + group < n_blocks ? g0 + group : n_blocks;
        uint32_t unc_max = 0;
#pragma omp parallel for schedule(dynamic, chunk) reduction(max : unc_max)
        for (long i = (long)g0; i < (long)g1; i++) {
            char *buf = xmalloc(cap);
            const uint32_t unc = fill(ctx, (size_t)i, buf);
            if (unc > unc_max) unc_max = unc;
            csize[i - (long)g0] = z_compress(buf, unc, comp + (size_t)(i - (long)g0) * ccap, ccap);
            free(buf);
        }
        if (unc_max > unc_buf) unc_buf = unc_max;
        for (size_t i = g0; i < g1; i++) {
            const uint64_t pos = (uint64_t)ftello(f);
            for (size_t k = i * per; k < n && k < (i + 1) * per; k++) items[k].off = pos;
            put(f, comp + (i - g0) * ccap, csize[i - g0]);
        }
    }
    free(comp);
    free(csize);
    return unc_buf;
}

typedef struct {
    const bw_summary *v;
    uint32_t count;
} zoom_ctx;

static uint32_t fill_records(const void *ctx, size_t i, char *buf)
{
    const zoom_ctx *z = ctx;
    const uint32_t at = (uint32_t)i * BW_ITEMS_PER_SLOT, n = z->count - at > BW_ITEMS_PER_SLOT ? BW_ITEMS_PER_SLOT : z->count - at;
    memcpy(buf, z->v + at, sizeof *z->v * n);                       /* a record is its 32 bytes as they lie in memory */
    return (uint32_t)sizeof *z->v * n;
}

/* cuskent/bbiWrite.c:478-536: the zoom records, itemsPerSlot to a deflated block, then their R tree */
static uint64_t write_summary_and_index(FILE *f, const bw_summary *v, uint32_t count, const bw_blocks *dev, uint64_t first_block)
{
    const zoom_ctx ctx = {v, count};
    PUT(f, count);
    ritem *items = xcalloc(count ? count : 1, sizeof *items);
    for (uint32_t i = 0; i < count; i++) {
        items[i].chrom = v[i].chrom_id;
        items[i].start = v[i].start;
        items[i].end = v[i].end;
    }
    if (dev) put_device_blocks(f, dev, first_block, items, count, BW_ITEMS_PER_SLOT);
    else (void)put_blocks_zlib(f, items, count, BW_ITEMS_PER_SLOT, sizeof *v * BW_ITEMS_PER_SLOT, 1024, fill_records, &ctx);
    const uint64_t index_offset = (uint64_t)ftello(f);
    cir_tree_write(f, items, count, BW_BLOCK_SIZE, BW_ITEMS_PER_SLOT, index_offset);
    free(items);
    return index_offset;
}

/* ---- the file skeleton (cuskent/bwgCreate.c:887-1019), shared by the dense and the sparse writer (bw_priv.h) */
void bw_file_begin(bw_file *F, const char *path, int n_sums, const uint32_t *reductions, const bw_chrom *chroms, size_t n_chroms, uint32_t max_name,
                   uint64_t section_count)
{
    const uint32_t block_size = BW_BLOCK_SIZE;
    FILE *f = fopen(path, "wb");
    if (!f) die("mustOpen: Can't open %s to write: %s", path, strerror(errno));
    F->f = f;
    F->path = path;
    const uint32_t sig = BW_SIG, res32 = 0, unc_buf = 0;
    const uint16_t version = BW_VERSION, summary_count = (uint16_t)n_sums, res16 = 0;
    const uint64_t res64 = 0;
    PUT(f, sig);
    PUT(f, version);
    PUT(f, summary_count);
    F->chrom_tree_pos = ftell(f);
    PUT(f, res64);
    F->data_pos = ftell(f);
    PUT(f, res64);
    F->index_pos = ftell(f);
    PUT(f, res64);
    PUT(f, res16);
    PUT(f, res16);
    PUT(f, res64);
    F->total_pos = ftell(f);
    PUT(f, res64);
    F->unc_pos = ftell(f);
    PUT(f, unc_buf);
    PUT(f, res64);
    for (int i = 0; i < n_sums; i++) {
        PUT(f, reductions[i]);
        PUT(f, res32);
        F->zoom_pos[i] = ftell(f);
        PUT(f, res64);
        PUT(f, res64);
    }
    F->total_summary_off = (uint64_t)ftello(f);
    put_zero(f, 40);
    const uint64_t chrom_tree_off = (uint64_t)ftello(f);
    bpt_write(f, chroms, n_chroms, block_size < n_chroms ? block_size : (uint32_t)n_chroms, max_name);
    const uint64_t data_off = (uint64_t)ftello(f);
    PUT(f, section_count);
    fseek(f, F->data_pos, SEEK_SET);
    PUT(f, data_off);
    fseek(f, F->chrom_tree_pos, SEEK_SET);
    PUT(f, chrom_tree_off);
    fseeko(f, (off_t)data_off + 8, SEEK_SET);
}

void bw_file_end(bw_file *F, const ritem *sec, size_t n_sec, const bw_summary *const *sum, const uint64_t *n_sum, int n_sums, uint32_t unc_buf,
                 const bw_blocks *dev, const uint64_t *slot_first)
{
    const uint32_t block_size = BW_BLOCK_SIZE, items_per_slot = BW_ITEMS_PER_SLOT;
    FILE *f = F->f;
    BW_T("data");
    const uint64_t index_off = (uint64_t)ftello(f);
    cir_tree_write(f, sec, n_sec, block_size, 1, index_off);
    BW_T("index");
    uint64_t zoom_data[10], zoom_index[10];
    for (int i = 0; i < n_sums; i++) {
        zoom_data[i] = (uint64_t)ftello(f);
        zoom_index[i] = write_summary_and_index(f, sum[i], (uint32_t)n_sum[i], dev, dev ? slot_first[i] : 0);
    }
    BW_T("zooms");
    /* the file-wide summary from the first zoom level (bwgCreate.c:966-988) */
    uint64_t total_summary_off = F->total_summary_off;
    if (n_sum[0]) {
        const bw_summary *s = &sum[0][0];
        uint64_t valid = s->valid_count;
        double mn = s->min_val, mx = s->max_val, sd = s->sum_data, sq = s->sum_squares;
        for (uint64_t i = 1; i < n_sum[0]; i++) {
            s = &sum[0][i];
            valid += s->valid_count;
            if (s->min_val < mn) mn = s->min_val;
            if (s->max_val > mx) mx = s->max_val;
            sd += s->sum_data;
            sq += s->sum_squares;
        }
        fseeko(f, (off_t)total_summary_off, SEEK_SET);
        PUT(f, valid);
        PUT(f, mn);
        PUT(f, mx);
        PUT(f, sd);
        PUT(f, sq);
    } else
        total_summary_off = 0;
    fseek(f, F->index_pos, SEEK_SET);
    PUT(f, index_off);
    fseek(f, F->total_pos, SEEK_SET);
    PUT(f, total_summary_off);
    if (32 * items_per_slot > unc_buf) unc_buf = 32 * items_per_slot;
    fseek(f, F->unc_pos, SEEK_SET);
    PUT(f, unc_buf);
    for (int i = 0; i < n_sums; i++) {
        fseek(f, F->zoom_pos[i], SEEK_SET);
        PUT(f, zoom_data[i]);
        PUT(f, zoom_index[i]);
    }
    fseek(f, 0L, SEEK_END);
    const uint32_t sig = BW_SIG;
    PUT(f, sig);
    if (fclose(f) != 0) die("carefulClose: error closing %s", F->path);
}

char *put_section_header(char *w, uint32_t chrom_id, uint32_t start, uint32_t end, uint32_t step, uint32_t span, uint8_t type, uint16_t cnt)
{
    const uint8_t r8 = 0;
    memcpy(w, &chrom_id, 4); w += 4;
    memcpy(w, &start, 4); w += 4;
    memcpy(w, &end, 4); w += 4;
    memcpy(w, &step, 4); w += 4;
    memcpy(w, &span, 4); w += 4;
    memcpy(w, &type, 1); w += 1;
    memcpy(w, &r8, 1); w += 1;
    memcpy(w, &cnt, 2); w += 2;
    return w;
}

static __thread double bw_t0;
void bw_tick(const char *what)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const double t = (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    if (getenv("ITX_TIMING_BW")) fprintf(stderr, "[itx timing] bw: %s %.3f s\n", what, t - bw_t0);
    bw_t0 = t;
}
