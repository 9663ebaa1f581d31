/* bamio.c — alignment input for the host: BGZF/BAM and SAM text decoded straight into the engine's pinned
 * record SoA (tid, pos, tmpend, mapq, flag5, mpos, isize). Follows the file formats and, where behaviour is
 * observable, samtools 0.1.18 as vendored by the reference: bgzf.c:401-411,471-565 (block framing), bam.c:69-109
 * (header), bam.c:179-210 (record), bam.c:17-27 (bam_calend: only M, D, N advance), bam_aux.c:36-48 (aux walk),
 * bam_import.c:237-330 (SAM text; a mapped record without CIGAR is flagged unmapped).
 * This file: the host BAM route (raw read-ahead, parallel inflate, the record hop, the parse), the BAM header, and at the
 * end what opens, closes and dispatches a reader. The BGZF member is bgzf.c's, the device decoder's feeder bamdev.c, SAM
 * text samio.c; the reader's state and who owns which part of it: aln_priv.h. */
#define _GNU_SOURCE
#include "aln_priv.h"

#include <omp.h>
#include <sys/stat.h>
#include <unistd.h>

double t_io, t_inflate, t_hop, t_parse;

#define CHUNK_COMPRESSED_DEFAULT (48u << 20)
#define CHUNK_COMPRESSED_DEVICE ALN_DEVICE_CHUNK  /* a lane per block on the device: it takes thousands of blocks to fill it */
/* compressed bytes read and inflated per step; ITX_BGZF_CHUNK overrides it (tests force many small steps) */
static size_t chunk_compressed(void)
{
    static size_t v;
    if (!v) {
        const char *e = getenv("ITX_BGZF_CHUNK");
        const long x = e ? atol(e) : 0;
        v = x >= 1 ? (size_t)x : dev_attached() ? CHUNK_COMPRESSED_DEVICE : CHUNK_COMPRESSED_DEFAULT;
    }
    return v;
}
#define CHUNK_COMPRESSED chunk_compressed()

/* ---- raw read-ahead: the file is read by its own thread, one chunk ahead, into the spare raw buffer behind RAW_HEAD
 * bytes of room for the incomplete block the indexer leaves over (less than one BGZF block). */
#define RAW_HEAD (BGZF_MAX + 64)
#define RAW_STEP (CHUNK_COMPRESSED < 256 ? (size_t)256 : CHUNK_COMPRESSED)      /* bytes per fread */
/* ... of a regular file with `left` bytes to go: no more than those (the buffers are page-locked when the device decodes, which
 * takes its time: a small file gets small ones) */
size_t aln_raw_step(size_t left)
{
    const size_t full = RAW_STEP, need = ((left + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1)) + ((size_t)1 << 20);
    return need < full ? need : full;
}
/* how many chunks the reader may be ahead of the one raw_next hands out next: from a regular file as many as there are
 * buffers beyond the one being indexed and the one whose pushes may still be copying (the reader used to wait for raw_next
 * after every chunk: while the producer sat in a push the file was not read, and then the producer waited for the file —
 * a quarter of the record loop of a BAM the device takes at the rate the page cache delivers it); else one.
 * THE TWO-CHUNK INVARIANT: with n_raw - 3 chunks ahead, chunk f + n_raw is read once raw_next has taken chunk f + 2, so a raw
 * buffer returns to the reader two raw_next calls after the pushes cut from it began — all of them were begun before the
 * chunk after it was taken, and another whole chunk has been indexed since. dev_pushes_copied, on the IO thread, reads one
 * word of a slot on the device side, copy_live (csrc/itx_inflater.h), which the producer stores with release in push_begin /
 * push_end and itx_bamwin_push_copied loads with acquire; the slot's `copied` event itself has no such guard: it is this
 * distance, nothing else, that keeps it from being re-recorded under the IO thread. Whoever changes io_ahead or n_raw changes that. */
static long io_ahead(const aln_reader *r) { return r->raw.n_raw == N_RAW_DEVICE_FILE ? r->raw.n_raw - 3 : 0; }

static void *io_main(void *arg)
{
    aln_reader *r = arg;
    pthread_mutex_lock(&r->raw.io_mu);
    for (;;) {
        /* chunk io_fill goes into buffer io_fill % n_raw, last used by chunk io_fill - n_raw: raw_next has long moved on from it */
        while (!r->raw.io_stop && (r->raw.io_eof_seen || r->raw.io_fill - r->raw.io_take > io_ahead(r))) pthread_cond_wait(&r->raw.io_cv, &r->raw.io_mu);
        if (r->raw.io_stop) break;
        const int b = (int)(r->raw.io_fill % r->raw.n_raw);
        const uint32_t lanes = r->raw.raw_lanes[b];
        r->raw.raw_lanes[b] = 0;
        pthread_mutex_unlock(&r->raw.io_mu);
        /* ... and the pushes cut from it have copied their bytes (all of them were begun before the chunk after it was taken) */
        if (lanes) dev_pushes_copied(lanes);
        if (!r->raw.craw[b]) r->raw.craw[b] = buf_alloc(RAW_HEAD + r->raw.raw_step + 64);       /* page-locking a buffer takes a while: not under the lock */
        uint8_t *dst = r->raw.craw[b] + RAW_HEAD;
        size_t got;
        if (r->raw.io_fd >= 0) {
            /* a regular file: the step is read as eight slices at once (one thread copying out of the page cache delivers
             * about 7 GB/s; the device takes a BAM of real content at the 55 GB/s of its PCIe link) */
            const size_t step = r->raw.raw_step;
            size_t want = r->raw.io_size > r->raw.io_off ? r->raw.io_size - r->raw.io_off : 0;
            if (want > step) want = step;
            static int max_parts;                                   /* ITX_READ_PARTS (1..16) overrides */
            if (!max_parts) {
                const char *e = getenv("ITX_READ_PARTS");
                const int v = e ? atoi(e) : 0;
                max_parts = v >= 1 && v <= 16 ? v : 8;
            }
            const int parts = want >= (4u << 20) ? max_parts : 1;
            const size_t per = (want + (size_t)parts - 1) / (size_t)parts;
            size_t done[16] = {0};
#pragma omp parallel for num_threads(parts) schedule(static, 1)
            for (int q = 0; q < parts; q++) {
                const size_t lo = (size_t)q * per, hi = lo + per < want ? lo + per : want;
                size_t at = lo;
                while (at < hi) {
                    const ssize_t k = pread(r->raw.io_fd, dst + at, hi - at, (off_t)(r->raw.io_off + at));
                    if (k <= 0) break;                             /* end of file or an error: what came before counts */
                    at += (size_t)k;
                }
                done[q] = at - lo;
            }
            got = 0;
            for (int q = 0; q < parts; q++) {
                got += done[q];
                if (done[q] < ((size_t)q * per + per < want ? per : want - (size_t)q * per)) break;     /* a short slice ends the stream there */
            }
            r->raw.io_off += got;
        } else {
            got = fread(dst, 1, r->raw.raw_step, r->cm.f);
        }
        pthread_mutex_lock(&r->raw.io_mu);
        r->raw.io_got[b] = got;
        if (got < r->raw.raw_step) r->raw.io_eof_seen = 1;                 /* a short read: end of file (or an error, same thing here) */
        r->raw.io_fill++;
        pthread_cond_broadcast(&r->raw.io_cv);
    }
    pthread_mutex_unlock(&r->raw.io_mu);
    return NULL;
}

/* Appends the next raw chunk behind the carried-over bytes; returns the bytes added (0 once the file is read out). */
size_t raw_next(aln_reader *r)
{
    if (r->raw.io_done) return 0;
    if (!r->raw.io_on) {
        r->raw.n_raw = 2;
        {
            struct stat sb;
            const int fd = fileno(r->cm.f);
            r->raw.io_fd = -1;
            if (fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && ftello(r->cm.f) == 0) {
                r->raw.io_fd = fd;
                r->raw.io_off = 0;
                r->raw.io_size = (size_t)sb.st_size;
                if (r->rg.rg_on) {
                    r->raw.io_off = r->rg.rg_lo_block;
                    /* the share ends inside the block at rg_end_block: nothing behind that block is this reader's */
                    if (r->rg.rg_end_block != SIZE_MAX && r->rg.rg_end_block + r->rg.rg_end_csize < r->raw.io_size) r->raw.io_size = r->rg.rg_end_block + r->rg.rg_end_csize;
                }
            } else if (r->rg.rg_on) {
                die("a share of %s was asked for, but it is not a regular file", "the alignment file");
            }
            r->raw.io_abs_end = r->raw.io_off;
            if (r->dv.dev) r->raw.n_raw = dev_raw_buffers(r->raw.io_fd >= 0);
        }
        r->raw.raw_step = r->raw.io_fd >= 0 ? aln_raw_step(r->raw.io_size > r->raw.io_off ? r->raw.io_size - r->raw.io_off : 0) : RAW_STEP;
        /* (Mapping the file and letting the device copy straight out of the page cache was tried twice and lost: through the
         * runtime's own path for unlocked memory the pipeline's copies go in staged pieces and hold the producer, 4.0 - 4.1 s per
         * run against 3.0 - 3.4 s; page-locking the mapping ahead with hipHostRegister costs 62 ms per GB — 3.5 s for the 56 GB
         * file, more when several threads do it — against the 11 core-seconds of pread it was meant to save:
         * profiles/r03_mmap_probe.txt, r03_cli_500M_hiseq_mmap*.json.) */
        pthread_mutex_init(&r->raw.io_mu, NULL);
        pthread_cond_init(&r->raw.io_cv, NULL);
        r->raw.io_fill = r->raw.io_take = 0;
        r->raw.io_eof_seen = 0;
        r->raw.io_stop = 0;
        if (pthread_create(&r->raw.io_thread, NULL, io_main, r) != 0) die("cannot start the file read-ahead thread");
        r->raw.io_on = 1;
    }
    pthread_mutex_lock(&r->raw.io_mu);
    while (r->raw.io_fill <= r->raw.io_take) pthread_cond_wait(&r->raw.io_cv, &r->raw.io_mu);
    const int b = (int)(r->raw.io_take % r->raw.n_raw);
    const size_t got = r->raw.io_got[b];
    uint8_t *nb = r->raw.craw[b];
    if (r->raw.clen > RAW_HEAD) die("BGZF: %zu bytes left over by the block indexer", r->raw.clen);    /* cannot happen: < one block */
    if (r->raw.clen) memcpy(nb + RAW_HEAD - r->raw.clen, r->raw.cbuf, r->raw.clen);
    r->raw.cbuf = nb + RAW_HEAD - r->raw.clen;
    r->raw.clen += got;
    r->raw.io_abs_end += got;
    r->raw.raw_cur = b;
    r->raw.io_take++;
    if (got < r->raw.raw_step) r->raw.io_done = 1;                         /* the reader has stopped behind this chunk */
    pthread_cond_broadcast(&r->raw.io_cv);                             /* a buffer further back has become the reader's */
    pthread_mutex_unlock(&r->raw.io_mu);
    return got;
}

/* Reads the next chunk of compressed blocks and inflates them in parallel into *pbuf at offset `at` (the buffer is
 * grown as needed, bytes before `at` are kept). Returns the number of bytes inflated; *peof is set when there is no
 * more input (end of file or a damaged block). Touches only the compressed-side state of the reader. */
static size_t bgzf_inflate_chunk(aln_reader *r, uint8_t **pbuf, size_t *pcap, size_t at, int *peof)
{
    double tq = now_s();
    const size_t got = raw_next(r);
    t_io += now_s() - tq;
    if (r->raw.clen == 0) {
        *peof = 1;
        return 0;
    }
    size_t off = 0, utot = 0;
    int damaged = 0;
    int capped = 0;
    const size_t nb = index_blocks(r->raw.cbuf, r->raw.clen, &r->hb.blk, &r->hb.blk_cap, SIZE_MAX, SIZE_MAX, &off, &utot, &damaged, &capped);
    struct blk *bl = r->hb.blk;
    if (at + utot + 64 > *pcap) {
        const size_t old_cap = *pcap;
        *pcap = (at + utot) * 5 / 4 + BGZF_MAX + 64;
        *pbuf = buf_grow(*pbuf, at < old_cap ? at : old_cap, *pcap);      /* the bytes before `at` are the caller's */
    }
    tq = now_s();
    int bad = 0;
    uint8_t *dst0 = *pbuf + at;
    const struct blk *blocks = bl;
    const uint8_t *cbase = r->raw.cbuf;
#pragma omp parallel for schedule(dynamic, 16) reduction(| : bad)
    for (long i = 0; i < (long)nb; i++)
        if (blocks[i].usize && inflate_block(cbase + blocks[i].coff, blocks[i].csize, dst0 + blocks[i].uoff, blocks[i].usize) != 0) bad |= 1;
    t_inflate += now_s() - tq;
    if (bad) {
        /* a block that does not inflate ends the stream there, like bgzf_read returning an error (bgzf.c:471-521) */
        size_t ok = 0;
        for (size_t i = 0; i < nb; i++) {
            if (bl[i].usize && inflate_block(r->raw.cbuf + bl[i].coff, bl[i].csize, dst0 + bl[i].uoff, bl[i].usize) != 0) break;
            ok = bl[i].uoff + bl[i].usize;
        }
        utot = ok;
        damaged = 1;
    }
    /* the incomplete tail block stays where it is; raw_next carries it over */
    r->raw.cbuf += off;
    r->raw.clen -= off;
    if (damaged || (got == 0 && nb == 0)) *peof = 1;
    return utot;
}

/* ---- read-ahead: while the caller hops over and parses one chunk, a loader thread reads and inflates the next one
 * into the spare buffer, behind PF_HEAD bytes of room for the caller's unconsumed tail (a partial record). */
#define PF_HEAD (4u << 20)
static void *pf_main(void *arg)
{
    aln_reader *r = arg;
    if (r->dv.dev) return dev_producer(r);
    pthread_mutex_lock(&r->cm.pf_mu);
    for (;;) {
        while (r->hb.pf_state != 1 && !r->cm.pf_stop) pthread_cond_wait(&r->cm.pf_cv, &r->cm.pf_mu);
        if (r->cm.pf_stop) break;
        pthread_mutex_unlock(&r->cm.pf_mu);
        int eof = 0;
        const size_t n = bgzf_inflate_chunk(r, &r->hb.nbuf, &r->hb.ncap, PF_HEAD, &eof);
        pthread_mutex_lock(&r->cm.pf_mu);
        r->hb.nlen = n;
        r->hb.n_eof = eof;
        r->hb.pf_state = 2;
        pthread_cond_broadcast(&r->cm.pf_cv);
    }
    pthread_mutex_unlock(&r->cm.pf_mu);
    return NULL;
}

static void pf_request(aln_reader *r)
{
    pthread_mutex_lock(&r->cm.pf_mu);
    r->hb.pf_state = 1;
    pthread_cond_broadcast(&r->cm.pf_cv);
    pthread_mutex_unlock(&r->cm.pf_mu);
}

void pf_start(aln_reader *r)
{
    pthread_mutex_init(&r->cm.pf_mu, NULL);
    pthread_cond_init(&r->cm.pf_cv, NULL);
    r->hb.pf_state = 0;
    r->cm.pf_stop = 0;
    if (pthread_create(&r->cm.pf_thread, NULL, pf_main, r) != 0) die("cannot start the BAM read-ahead thread");
    r->cm.pf_on = 1;
    if (!r->cm.eof && !r->dv.dev) pf_request(r);                        /* the device producer drives itself */
}

/* Makes more inflated bytes available behind the unconsumed ones. Returns the number of bytes added (0 at end of
 * input). Synchronous while the header is read, from the read-ahead thread afterwards. */
static size_t bgzf_load_chunk(aln_reader *r)
{
    if (r->cm.eof) return 0;
    if (!r->cm.pf_on) {
        /* keep what the record parser has not consumed */
        if (r->hb.upos) {
            memmove(r->hb.ubuf, r->hb.ubuf + r->hb.upos, r->hb.ulen - r->hb.upos);
            r->hb.ulen -= r->hb.upos;
            r->hb.upos = 0;
        }
        int eof = 0;
        const size_t n = bgzf_inflate_chunk(r, &r->hb.ubuf, &r->hb.ucap, r->hb.ulen, &eof);
        r->hb.ulen += n;
        if (eof) r->cm.eof = 1;
        return n;
    }
    pthread_mutex_lock(&r->cm.pf_mu);
    while (r->hb.pf_state != 2) pthread_cond_wait(&r->cm.pf_cv, &r->cm.pf_mu);
    r->hb.pf_state = 0;
    pthread_mutex_unlock(&r->cm.pf_mu);
    const size_t tail = r->hb.ulen - r->hb.upos, n = r->hb.nlen;
    if (tail > PF_HEAD) {                                      /* a record of more than 4 MB: make room the slow way */
        uint8_t *big = buf_alloc(tail + n + 64);
        memcpy(big, r->hb.ubuf + r->hb.upos, tail);
        memcpy(big + tail, r->hb.nbuf + PF_HEAD, n);
        buf_free(r->hb.ubuf);
        r->hb.ubuf = big;
        r->hb.ucap = tail + n + 64;
        r->hb.upos = 0;
        r->hb.ulen = tail + n;
    } else {
        memcpy(r->hb.nbuf + PF_HEAD - tail, r->hb.ubuf + r->hb.upos, tail);
        uint8_t *tb = r->hb.ubuf;
        r->hb.ubuf = r->hb.nbuf;
        r->hb.nbuf = tb;
        const size_t tc = r->hb.ucap;
        r->hb.ucap = r->hb.ncap;
        r->hb.ncap = tc;
        r->hb.upos = PF_HEAD - tail;
        r->hb.ulen = PF_HEAD + n;
    }
    if (r->hb.n_eof)
        r->cm.eof = 1;
    else
        pf_request(r);
    return n;
}

/* sequential read of n bytes (header parsing) */
static size_t bgzf_read(aln_reader *r, void *dst, size_t n)
{
    if (r->hb.hz) return hz_read((hz_t *)r->hb.hz, dst, n);
    if (r->dv.dev) return dev_read(r, dst, n);
    while (r->hb.ulen - r->hb.upos < n) {
        if (bgzf_load_chunk(r) == 0 && r->cm.eof) break;
    }
    size_t k = r->hb.ulen - r->hb.upos;
    if (k > n) k = n;
    memcpy(dst, r->hb.ubuf + r->hb.upos, k);
    r->hb.upos += k;
    return k;
}

void add_target(aln_reader *r, const char *name)
{
    r->cm.tname = xrealloc(r->cm.tname, sizeof(char *) * (size_t)(r->cm.n_targets + 1));
    r->cm.tname[r->cm.n_targets++] = xstrdup(name);
}

/* filter -b: the header's bytes are kept as they are read (aln_keep_header before the reader is opened) */
static int keep_header;
void aln_keep_header(int on) { keep_header = on; }
const uint8_t *aln_header_bytes(const aln_reader *r, size_t *len)
{
    *len = r->cm.hdr_raw_len;
    return r->cm.hdr_raw;
}
static size_t hdr_read(aln_reader *r, void *dst, size_t n)
{
    const size_t k = bgzf_read(r, dst, n);
    if (keep_header && k) {
        if (r->cm.hdr_raw_len + k > r->cm.hdr_raw_cap) {
            r->cm.hdr_raw_cap = (r->cm.hdr_raw_len + k) * 2 + 4096;
            r->cm.hdr_raw = xrealloc(r->cm.hdr_raw, r->cm.hdr_raw_cap);
        }
        memcpy(r->cm.hdr_raw + r->cm.hdr_raw_len, dst, k);
        r->cm.hdr_raw_len += k;
    }
    return k;
}

static int bam_read_header(aln_reader *r)
{
    uint8_t b[8];
    if (hdr_read(r, b, 4) != 4 || memcmp(b, "BAM\1", 4) != 0) {
        fprintf(stderr, "[bam_header_read] invalid BAM binary header (this is not a BAM file).\n");
        return -1;
    }
    if (hdr_read(r, b, 4) != 4) return -1;
    int32_t l_text = rd_i32(b);
    while (l_text > 0) {                     /* the text header is not needed: tids come from the binary list */
        uint8_t skip[4096];
        size_t k = (size_t)l_text < sizeof skip ? (size_t)l_text : sizeof skip;
        if (hdr_read(r, skip, k) != k) return -1;
        l_text -= (int32_t)k;
    }
    if (hdr_read(r, b, 4) != 4) return -1;
    const int32_t n_ref = rd_i32(b);
    for (int32_t i = 0; i < n_ref; i++) {
        if (hdr_read(r, b, 4) != 4) return -1;
        const int32_t l_name = rd_i32(b);
        if (l_name <= 0 || l_name > 1 << 20) return -1;
        char *nm = xmalloc((size_t)l_name + 1);
        if (hdr_read(r, nm, (size_t)l_name) != (size_t)l_name) {
            free(nm);
            return -1;
        }
        nm[l_name] = 0;
        add_target(r, nm);
        free(nm);
        if (hdr_read(r, b, 4) != 4) return -1;     /* l_ref */
    }
    return 0;
}

/* ---- locating the records --------------------------------------------------------------------------------------
 * A BAM stream is a chain: a record's length field says where the next record starts (bam.c:179-210 reads them one by one).
 * Walking that chain is a pointer chase through hundreds of megabytes per chunk — one core, one cache miss per record. The
 * chunk is cut into pieces instead and every piece is walked by its own thread from a GUESSED start: the first offset in the
 * piece from which a few records in a row look like records. A guess proves nothing by itself; what makes the result exact
 * is the check afterwards, in stream order: piece 0 starts at a known record start, and a piece is accepted only if its
 * guess is precisely where the chain of the pieces before it arrives — otherwise that piece is walked again from there. */
typedef struct {
    size_t c, end, n, first;   /* guessed start (SIZE_MAX none), where the walk stopped, starts found, their place in spec */
    int why;                   /* 0 reached the piece's limit, 1 needs more input, 2 malformed length (bam.c:186-190) */
} hop_piece;

static size_t hop_run(const uint8_t *u, size_t p, size_t lim, size_t L, size_t *off, size_t *pn, int *why)
{
    size_t n = *pn;
    while (p < lim) {
        if (p + 4 > L) {
            *why = 1;
            *pn = n;
            return p;
        }
        __builtin_prefetch(u + p + 1024);
        __builtin_prefetch(u + p + 2048);
        const int32_t bl = rd_i32(u + p);
        if (bl < 32) {
            *why = 2;
            *pn = n;
            return p;
        }
        if (p + 4 + (size_t)bl > L) {
            *why = 1;
            *pn = n;
            return p;
        }
        off[n++] = p;
        p += 4 + (size_t)bl;
    }
    *why = 0;
    *pn = n;
    return p;
}

/* does a complete record that looks like one start at p? (only ever used to pick a guess) */
static inline size_t looks_like_record(const uint8_t *u, size_t p, size_t L, int n_targets)
{
    size_t step = 0;
    return record_or_short(u, p, L, n_targets, &step) == 1 ? step : 0;
}

static size_t hop_piece_bytes(void)
{
    static size_t v;
    if (!v) {
        const char *e = getenv("ITX_HOP_PIECE");                  /* tests force tiny pieces: many guesses, many of them wrong */
        const long x = e ? atol(e) : 0;
        v = x >= 1 ? (size_t)x : (1u << 20);
    }
    return v;
}

/* Fills rec_off / n_rec with the starts of the complete records in ubuf[upos, ulen), exactly as the one-by-one walk would;
 * sets upos behind the last of them (when there is one), and eof / ulen at a malformed length. */
static void locate_records(aln_reader *r)
{
    const uint8_t *u = r->hb.ubuf;
    const size_t p0 = r->hb.upos, L = r->hb.ulen;
    r->hb.n_rec = r->hb.rec_next = 0;
    if (p0 >= L) return;
    const size_t worst = (L - p0) / 36 + 2;                        /* a record is at least 36 bytes */
    const size_t piece = hop_piece_bytes();
    size_t T = (L - p0) / piece;
    const size_t tmax = (size_t)omp_get_max_threads() * 8;
    if (T > tmax) T = tmax;
    if (r->hb.rec_cap < worst) {
        r->hb.rec_cap = worst + worst / 4;
        r->hb.rec_off = xrealloc(r->hb.rec_off, sizeof(size_t) * r->hb.rec_cap);
    }
    size_t p;
    int why = 0;
    if (T < 2) {
        p = hop_run(u, p0, L, L, r->hb.rec_off, &r->hb.n_rec, &why);
    } else {
        if (r->hb.spec_cap < worst + T) {
            r->hb.spec_cap = worst + worst / 4 + T;
            r->hb.spec = xrealloc(r->hb.spec, sizeof(size_t) * r->hb.spec_cap);
        }
        hop_piece *pc = xcalloc(T, sizeof *pc);
        const size_t span = (L - p0) / T;
        const int n_targets = r->cm.n_targets;
        size_t *spec = r->hb.spec;
#pragma omp parallel for schedule(dynamic, 1)
        for (long t = 0; t < (long)T; t++) {
            const size_t b = p0 + (size_t)t * span, lim = (size_t)t + 1 < T ? p0 + ((size_t)t + 1) * span : L;
            hop_piece *q = &pc[t];
            q->first = (b - p0) / 36 + (size_t)t;                  /* room for every start this piece can hold */
            q->c = SIZE_MAX;
            q->n = 0;
            if (t == 0) {
                q->c = b;
            } else {
                for (size_t c = b; c < lim; c++) {
                    size_t a = c, k = 0;
                    while (k < 3 && a < L) {                       /* three in a row, or up to the end of what is inflated */
                        const size_t step = looks_like_record(u, a, L, n_targets);
                        if (!step) break;
                        a += step;
                        k++;
                    }
                    if (k == 3 || (k > 0 && a >= L)) {
                        q->c = c;
                        break;
                    }
                }
            }
            q->end = q->c;
            if (q->c != SIZE_MAX) q->end = hop_run(u, q->c, lim, L, spec + q->first, &q->n, &q->why);
        }
        /* in stream order: accept a piece whose guess is where the chain arrives, walk it again otherwise */
        size_t cur = p0;
        p = p0;
        for (size_t t = 0; t < T; t++) {
            const size_t lim = t + 1 < T ? p0 + (t + 1) * span : L;
            hop_piece *q = &pc[t];
            if (cur >= lim) {                                      /* a record reaches over the whole piece */
                q->n = 0;
                continue;
            }
            if (q->c != cur) {
                q->n = 0;
                q->end = hop_run(u, cur, lim, L, spec + q->first, &q->n, &q->why);
                r->hb.hop_redone++;
            }
            p = cur = q->end;
            why = q->why;
            if (why) {
                for (size_t k = t + 1; k < T; k++) pc[k].n = 0;
                break;
            }
        }
        size_t tot = 0;
        for (size_t t = 0; t < T; t++) {
            const size_t n = pc[t].n;
            pc[t].c = tot;                                         /* reused: the piece's place in rec_off */
            tot += n;
        }
#pragma omp parallel for schedule(static)
        for (long t = 0; t < (long)T; t++)
            if (pc[t].n) memcpy(r->hb.rec_off + pc[t].c, spec + pc[t].first, sizeof(size_t) * pc[t].n);
        r->hb.n_rec = tot;
        r->hb.hop_pieces += T;
        free(pc);
    }
    if (why == 2) {                                                /* bam.c:186-190: a malformed length ends the file */
        r->cm.eof = 1;
        r->hb.ulen = p;
    }
    if (r->hb.n_rec) r->hb.upos = p;                                     /* consumed up to here once these are parsed */
}

static size_t bam_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa)
{
    if (r->dv.dev) return dev_read_batch(r, st, cap, side, any_paired, aux_xa);
    if (side) side->has_strings = 1;
    size_t n = 0;
    if (!r->cm.pf_on && !r->cm.eof) pf_start(r);
    while (n < cap) {
        if (r->hb.rec_next == r->hb.n_rec) {
            /* locate the records of what is inflated; load more when none is complete */
            r->hb.n_rec = r->hb.rec_next = 0;
            double th = now_s();
            for (;;) {
                locate_records(r);
                if (r->hb.n_rec) break;
                const double tl = now_s();
                const size_t more = bgzf_load_chunk(r);
                th += now_s() - tl;                               /* the load is accounted as io / inflate */
                if (more == 0 && r->cm.eof) break;                   /* end of input (a truncated tail record is dropped) */
            }
            t_hop += now_s() - th;
            if (r->hb.n_rec == 0) break;
        }
        size_t m = r->hb.n_rec - r->hb.rec_next;
        if (m > cap - n) m = cap - n;
        const size_t *ro = r->hb.rec_off + r->hb.rec_next;
        const double tp = now_s();
        int ap = 0, xa = 0;
#pragma omp parallel for schedule(static) reduction(| : ap, xa)
        for (long i = 0; i < (long)m; i++) {
            int a1 = 0, x1 = 0;
            bam_parse_one(r->hb.ubuf + ro[i], n + (size_t)i, st, side, &a1, &x1);
            ap |= a1;
            xa |= x1;
        }
        t_parse += now_s() - tp;
        if (ap) *any_paired = 1;
        if (xa) *aux_xa = 1;
        r->hb.rec_next += m;
        n += m;
    }
    return n;
}


/* ---- open, close, dispatch ----------------------------------------------------------------------------------------------- */
aln_reader *reader_new(FILE *f)
{
    ld_probe();
    aln_reader *r = xcalloc(1, sizeof *r);
    r->cm.f = f;
    names_init(&r->cm.tnames);
    r->dv.dk_cur = -1;
    r->sam.pending_len = -1;
    r->sam.sz_prev_slot = -1;
    r->sam.sam_fd = -1;
    return r;
}

/* the reference list of the file behind fd, by the plain host reader (a few blocks); *consumed: the inflated bytes it takes */
static int header_by_host(aln_reader *r, int fd, size_t size, size_t *consumed)
{
    hz_t z;
    memset(&z, 0, sizeof z);
    z.fd = fd;
    z.size = size;
    r->hb.hz = &z;
    const int rc = bam_read_header(r);
    r->hb.hz = NULL;
    if (consumed) *consumed = z.pos;
    hz_free(&z);
    return rc;
}

aln_reader *aln_open(const char *path, int is_sam)
{
    if (is_sam) return sam_open(path);
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    aln_reader *r = reader_new(f);
    r->dv.dev = dev_attached();
    if (r->dv.dev) dev_drain_windows();
    int rc;
    struct stat sb;
    if (r->dv.dev && !getenv("ITX_HEADER_BY_DEVICE") && fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode)) {
        /* a regular file: the reference list by the plain host reader (a few blocks, milliseconds), and the device's stream
         * skips that many bytes when its first window arrives. Reading the header through the device meant one whole push —
         * a chunk read, copied and decoded while nothing else ran (0.19 s) — before the pipeline of pushes could start. */
        rc = header_by_host(r, fileno(f), (size_t)sb.st_size, &r->dv.dskip_left);
        r->dv.dparsed = 1;                                        /* nothing to parse before the first window is in */
    } else {
        rc = bam_read_header(r);
        if (r->dv.dev && rc == 0) dev_header_done(r);
    }
    if (rc != 0) {
        aln_close(r);
        return NULL;
    }
    for (int i = 0; i < r->cm.n_targets; i++) names_intern(&r->cm.tnames, r->cm.tname[i]);    /* first occurrence wins a lookup */
    return r;
}

/* A share of a BAM file for one rank of a multi-GPU job: the records that START in the compressed byte range [lo, hi) of
 * the file — more exactly between the split points find_split gives for lo and for hi (hi = SIZE_MAX: up to the end).
 * Device decoder only. The header is read like any reader's (every rank needs the reference list). */
aln_reader *aln_open_range(const char *path, size_t lo, size_t hi)
{
    if (lo == 0 && hi == SIZE_MAX) return aln_open(path, 0);
    if (!dev_attached()) die("a share of %s was asked for without the device decoder", path);
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    struct stat sb;
    if (fstat(fileno(f), &sb) != 0 || !S_ISREG(sb.st_mode)) {
        fclose(f);
        return NULL;
    }
    const size_t fsize = (size_t)sb.st_size;
    aln_reader *r = reader_new(f);
    r->dv.dev = 1;
    r->rg.rg_on = 1;
    r->rg.rg_end_block = SIZE_MAX;
    dev_drain_windows();
    /* the reference list, by the plain host reader (a few blocks) */
    if (header_by_host(r, fileno(f), fsize, NULL) != 0) {
        aln_close(r);
        return NULL;
    }
    int empty = 0;
    size_t B = 0, c = 0, cs = 0;
    if (hi != SIZE_MAX && hi < fsize) {
        const int fs = find_split(fileno(f), fsize, hi, r->cm.n_targets, &B, &c, &cs);
        if (fs > 0) {
            r->rg.rg_end_block = B;
            r->rg.rg_end_off = c;
            r->rg.rg_end_csize = cs;
        } else if (fs < 0) {
            r->rg.rg_suspect = 1;                                     /* the search was given up: no share of this job can be trusted (whole-job fallback) */
        }
    }
    if (lo > 0) {
        const int fs = find_split(fileno(f), fsize, lo, r->cm.n_targets, &B, &c, &cs);
        if (fs <= 0) {
            empty = 1;                                             /* 0: no record starts behind lo, the share before this one runs to the end */
            if (fs < 0) r->rg.rg_suspect = 1;                         /* given up: see above */
        } else {
            if (r->rg.rg_end_block != SIZE_MAX && (B > r->rg.rg_end_block || (B == r->rg.rg_end_block && c >= r->rg.rg_end_off))) empty = 1;
            r->rg.rg_lo_block = B;
            r->dv.dskip_left = c;
            r->dv.dparsed = 1;                                        /* nothing to parse before the first window is in */
        }
    } else {
        /* from the start of the file: the header goes by once more, in front of the records, through the device's windows */
        for (int i = 0; i < r->cm.n_targets; i++) free(r->cm.tname[i]);
        free(r->cm.tname);
        r->cm.tname = NULL;
        r->cm.n_targets = 0;
        r->cm.hdr_raw_len = 0;
        if (bam_read_header(r) != 0) {
            aln_close(r);
            return NULL;
        }
        dev_header_done(r);
    }
    if (empty) {
        r->cm.eof = 1;
        r->dv.dlast = 1;
        r->dv.dparsed = 1;
        r->rg.rg_verified = 1;
    }
    for (int i = 0; i < r->cm.n_targets; i++) names_intern(&r->cm.tnames, r->cm.tname[i]);
    return r;
}

/* find_split for callers outside this file (the CPU test tool): the reference list is read first, like aln_open_range does */
int aln_find_split(const char *path, size_t at, size_t *block, size_t *off, size_t *csize)
{
    FILE *f = fopen(path, "rb");
    if (!f) return -1;
    aln_reader *r = reader_new(f);
    struct stat sb;
    int found = -1;
    if (fstat(fileno(f), &sb) == 0 && header_by_host(r, fileno(f), (size_t)sb.st_size, NULL) == 0)
        found = find_split(fileno(f), (size_t)sb.st_size, at, r->cm.n_targets, block, off, csize);     /* 1 found, 0 none up to the end, -1 given up */
    aln_close(r);
    return found;
}

/* after the last batch: 1 when the share's end boundary held (the record chain arrived exactly there) or it has none */
int aln_range_verified(const aln_reader *r)
{
    if (!r->rg.rg_on) return 1;
    if (r->rg.rg_suspect) return 0;
    if (r->rg.rg_end_block == SIZE_MAX) return 1;
    return r->rg.rg_verified == 1;
}

void aln_close(aln_reader *r)
{
    if (!r) return;
    if (getenv("ITX_TIMING") && !r->cm.is_sam)
        fprintf(stderr, "[itx timing] BAM decode so far: file read %.3f s, inflate (%s) %.3f s, record hop %.3f s (%zu pieces, %zu walked again), parse %.3f s\n", t_io,
                r->dv.dev ? "device" : inflater_name(), t_inflate, t_hop, r->hb.hop_pieces, r->hb.hop_redone + r->dv.d_rewalked, t_parse);
    if (r->cm.pf_on) {
        pthread_mutex_lock(&r->cm.pf_mu);
        while (!r->dv.dev && r->hb.pf_state == 1) pthread_cond_wait(&r->cm.pf_cv, &r->cm.pf_mu);      /* let a chunk in flight land */
        r->cm.pf_stop = 1;
        pthread_cond_broadcast(&r->cm.pf_cv);
        pthread_mutex_unlock(&r->cm.pf_mu);
        pthread_join(r->cm.pf_thread, NULL);
    }
    dev_close(r);
    if (r->raw.io_on) {
        pthread_mutex_lock(&r->raw.io_mu);
        r->raw.io_stop = 1;                                                        /* (a read in flight lands first: the thread looks when it is back) */
        pthread_cond_broadcast(&r->raw.io_cv);
        pthread_mutex_unlock(&r->raw.io_mu);
        pthread_join(r->raw.io_thread, NULL);
    }
    sam_close(r);
    if (r->cm.f) fclose(r->cm.f);
    for (int k = 0; k < N_RAW_DEVICE; k++) buf_free(r->raw.craw[k]);
    buf_free(r->hb.nbuf);
    free(r->hb.blk);
    for (int i = 0; i < r->cm.n_targets; i++) free(r->cm.tname[i]);
    free(r->cm.tname);
    free(r->cm.hdr_raw);
    names_free(&r->cm.tnames);
    buf_free(r->hb.ubuf);
    free(r->hb.rec_off);
    free(r->hb.spec);
    free(r);
}

int aln_n_targets(const aln_reader *r) { return r->cm.n_targets; }
const char *aln_target_name(const aln_reader *r, int tid) { return r->cm.tname[tid]; }

void aln_readahead(aln_reader *r)
{
    if (!r->cm.is_sam && !r->cm.pf_on && !r->cm.eof) pf_start(r);
}

size_t aln_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa)
{
    return r->cm.is_sam ? sam_read_batch(r, st, cap, side, any_paired, aux_xa) : bam_read_batch(r, st, cap, side, any_paired, aux_xa);
}
