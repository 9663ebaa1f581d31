/* bamdev.c — the device decoder's feeder (aln_use_device): BGZF blocks are inflated, records located and parsed on the
 * device; this side cuts the compressed chunks into pushes, settles the blocks the device declines, and hands the records'
 * arrays out. Of the reader it touches the common, raw, share and device groups (aln_priv.h). */
#define _GNU_SOURCE
#include "aln_priv.h"

#include <unistd.h>

static aln_device_ops dev;                   /* .push_begin == NULL: the host decodes */
static int dev_nwin = ITX_BAMWIN_WINDOWS;   /* windows the pushes rotate through */
void aln_use_device(const aln_device_ops *ops)
{
    if (ops) dev = *ops;
    else memset(&dev, 0, sizeof dev);
    dev_nwin = dev.n_windows >= 2 && dev.n_windows <= ITX_BAMWIN_WINDOWS ? dev.n_windows : ITX_BAMWIN_WINDOWS;
}
#define DEV_CHK(call, what)                                                                                    \
    do {                                                                                                       \
        if ((call) != 0) die("device decoder: %s failed: %s", what, dev.last_error ? dev.last_error() : "?"); \
    } while (0)

/* the big byte buffers (compressed chunks, inflated chunks): page-locked when the device inflates */
uint8_t *buf_alloc(size_t n)
{
    if (dev.alloc) {
        uint8_t *p = dev.alloc(n);
        if (!p) die("cannot get %zu bytes of page-locked memory", n);
        return p;
    }
    return xmalloc(n);
}
void buf_free(uint8_t *p)
{
    if (!p) return;
    if (dev.release) dev.release(p);
    else free(p);
}
uint8_t *buf_grow(uint8_t *old, size_t keep, size_t ncap)
{
    uint8_t *p = buf_alloc(ncap);
    if (old && keep) memcpy(p, old, keep);
    buf_free(old);
    return p;
}

int dev_attached(void) { return dev.push_begin != NULL; }

/* raw buffers a reader with the device decoder rotates through (struct aln_reader: craw) */
int dev_raw_buffers(int regular_file) { return regular_file && dev.push_copied ? N_RAW_DEVICE_FILE : N_RAW_DEVICE; }

/* (the IO thread, before it fills a raw buffer again:) the pushes of these lanes, bit s = lane s, have copied their bytes */
void dev_pushes_copied(uint32_t lanes)
{
    for (int sl = 0; sl < ITX_BAMWIN_LANES; sl++)
        if (lanes >> sl & 1u) DEV_CHK(dev.push_copied(dev.ctx, sl), "push_copied");
}

/* whatever an earlier file left unconsumed is not this file's */
void dev_drain_windows(void)
{
    for (int w = 0; w < ITX_BAMWIN_WINDOWS; w++) {
        size_t left = 0;
        DEV_CHK(dev.avail(dev.ctx, w, &left), "avail");
        DEV_CHK(dev.skip(dev.ctx, w, left), "skip");
    }
}

/* the header has gone by through the device's windows (dev_read): the records start here */
void dev_header_done(aln_reader *r)
{
    DEV_CHK(dev.skip(dev.ctx, r->dv.dw, r->dv.hdr_pos), "skip");
    free(r->dv.hdr);
    r->dv.hdr = NULL;
    r->dv.hdr_len = r->dv.hdr_pos = 0;
}

/* pushes kept in flight: pass 1 of the device decoder is a lane per block and latency-bound (a chunk's 8 k blocks take the
 * same ~9 ms as 1 k would), so several chunks' pass 1 run side by side on a chip that one of them fills to a tenth;
 * ITX_PUSHES (1 .. ITX_BAMWIN_LANES) overrides */
static long pushes_in_flight(void)
{
    static long v;
    if (!v) {
        const char *e = getenv("ITX_PUSHES");
        const long x = e ? atol(e) : 0;
        v = x >= 1 && x <= ITX_BAMWIN_LANES ? x : ITX_BAMWIN_LANES_DEFAULT;
    }
    return v;
}

/* ---- the device decoder (aln_use_device): this side only moves compressed bytes in ------------------------------------
 * Chunk k of the file is pushed into window k % ITX_BAMWIN_WINDOWS of the device on lane k % pushes_in_flight() (a lane = a
 * stream with its own scratch): that many pushes are kept in flight, so the Huffman pass of one chunk — a lane per block, latency-bound, most of the chip idle —
 * runs beside the token replay of the chunk before it. A block the device decoder flags is given to zlib here, whose verdict
 * is the reference's: inflated after all, its bytes are patched in; not inflatable, the stream ends in front of it
 * (bgzf.c:471-521). */
static void dev_begin(aln_reader *r)
{
    /* a window takes at most this much (extremely compressible input inflates a chunk to many gigabytes; the device side
     * counts in 32 bits and keeps a quarter megabyte of scratch per block) */
    enum { DEV_MAX_BLOCKS = 16384, DEV_MAX_BYTES = 1u << 30 };
    static size_t max_blocks;
    if (!max_blocks) {
        const char *e = getenv("ITX_DEV_WINDOW_BLOCKS");              /* tests: windows of a few blocks */
        const long x = e ? atol(e) : 0;
        max_blocks = x >= 1 ? (size_t)x : dev.max_blocks ? dev.max_blocks : DEV_MAX_BLOCKS;
        if (dev.max_blocks && max_blocks > dev.max_blocks) max_blocks = dev.max_blocks;
    }
    const size_t max_bytes = dev.max_bytes ? dev.max_bytes : DEV_MAX_BYTES;
    const long k = r->dv.dk_begin;
    struct dev_job *j = &r->dv.dj[k % pushes_in_flight()];
    double tq = now_s();
    size_t got = 1;
    if (!r->dv.dmore) got = raw_next(r);                              /* complete blocks of the last raw chunk are still waiting */
    t_io += now_s() - tq;
    size_t off = 0, utot = 0;
    int damaged = 0, capped = 0;
    const size_t nb = r->raw.clen ? index_blocks(r->raw.cbuf, r->raw.clen, &j->bl, &j->bl_cap, max_blocks, max_bytes, &off, &utot, &damaged, &capped) : 0;
    r->dv.dmore = capped;
    if (r->dv.dblk_cap < nb + 1) {
        r->dv.dblk_cap = nb + nb / 4 + 1;
        r->dv.dblk = xrealloc(r->dv.dblk, sizeof *r->dv.dblk * r->dv.dblk_cap);
        r->dv.dstatus = xrealloc(r->dv.dstatus, r->dv.dblk_cap);
    }
    size_t nb_use = nb;
    j->trunc = SIZE_MAX;
    int share_done = 0;
    if (r->rg.rg_on && r->rg.rg_end_block != SIZE_MAX && !r->rg.rg_stop_hit) {
        /* where the share ends: rg_end_off inflated bytes into the block that starts at file offset rg_end_block. The
         * record before that point ends exactly there when the boundary is a true record start (checked once the last
         * window is parsed), so the window is cut there and nothing behind is decoded. */
        const size_t abs0 = r->raw.io_abs_end - r->raw.clen;
        for (size_t i = 0; i < nb; i++) {
            const size_t at = abs0 + j->bl[i].coff;
            if (at == r->rg.rg_end_block) {
                r->rg.rg_stop_hit = 1;
                j->trunc = j->bl[i].uoff + r->rg.rg_end_off;
                if (j->trunc > j->bl[i].uoff + j->bl[i].usize) {      /* the boundary lies behind the block's bytes: not this stream's */
                    r->rg.rg_stop_missed = 1;
                    j->trunc = j->bl[i].uoff;
                }
                nb_use = i + 1;
                share_done = 1;
                break;
            }
            if (at > r->rg.rg_end_block) {                                 /* the chain of blocks steps over it: a false boundary */
                r->rg.rg_stop_missed = 1;
                nb_use = i;
                j->trunc = j->bl[i].uoff;
                share_done = 1;
                break;
            }
        }
        if (share_done) {
            off = nb_use < nb ? j->bl[nb_use].coff : off;
            utot = nb_use ? j->bl[nb_use - 1].uoff + j->bl[nb_use - 1].usize : 0;
            r->dv.dmore = 0;
        }
    }
    for (size_t i = 0; i < nb_use; i++)
        r->dv.dblk[i] = (itx_bgzf_block){(uint32_t)j->bl[i].coff, (uint32_t)j->bl[i].csize, (uint32_t)j->bl[i].uoff, (uint32_t)j->bl[i].usize};
    r->dv.dstream_total += utot;
    j->nb = nb_use;
    j->cbase = r->raw.cbuf;
    j->cabs = r->raw.io_fd >= 0 ? r->raw.io_abs_end - r->raw.clen : SIZE_MAX;
    if (r->raw.n_raw == N_RAW_DEVICE_FILE && r->raw.io_on) {
        pthread_mutex_lock(&r->raw.io_mu);
        r->raw.raw_lanes[r->raw.raw_cur] |= 1u << (k % pushes_in_flight());
        pthread_mutex_unlock(&r->raw.io_mu);
    }
    j->w = (int)(k % dev_nwin);
    j->last = damaged || share_done || (got == 0 && nb == 0);
    if (damaged && r->rg.rg_on) r->rg.rg_suspect = 1;
    static const uint8_t none[16];
    tq = now_s();
    DEV_CHK(dev.push_begin(dev.ctx, j->w, (int)(k % pushes_in_flight()), r->raw.clen ? r->raw.cbuf : none, off, r->dv.dblk, nb_use), "push");
    t_inflate += now_s() - tq;
    r->raw.cbuf += off;
    r->raw.clen -= off;
    r->dv.dk_begin = k + 1;
}

/* waits for the oldest push in flight and settles its flagged blocks; the caller publishes dk_ready */
static void dev_end(aln_reader *r)
{
    const long k = r->dv.dk_ready;
    struct dev_job *j = &r->dv.dj[k % pushes_in_flight()];
    size_t n_new = 0;
    const double tq = now_s();
    DEV_CHK(dev.push_end(dev.ctx, (int)(k % pushes_in_flight()), r->dv.dstatus, &n_new), "push");
    int damaged = 0;
    for (size_t i = 0; i < j->nb; i++)
        if (r->dv.dstatus[i]) {
            uint8_t tmp[BGZF_MAX + 8], again[BGZF_MAX + 64];
            const uint8_t *cb = j->cbase + j->bl[i].coff;
            if (r->raw.n_raw == N_RAW_DEVICE_FILE) {
                /* the compressed bytes may have left their buffer by now: from the file once more */
                cb = again;
                if (j->bl[i].csize > sizeof again || pread(r->raw.io_fd, again, j->bl[i].csize, (off_t)(j->cabs + j->bl[i].coff)) != (ssize_t)j->bl[i].csize)
                    die("cannot read the BGZF block at offset %zu again", j->cabs + j->bl[i].coff);
            }
            if (inflate_block(cb, j->bl[i].csize, tmp, j->bl[i].usize) == 0) {
                fprintf(stderr, "[iteres] note: BGZF block at chunk offset %zu declined by the device decoder (code %d), inflated by zlib\n", j->bl[i].coff,
                        r->dv.dstatus[i]);
                DEV_CHK(dev.patch(dev.ctx, j->w, j->bl[i].uoff, tmp, j->bl[i].usize), "patch");
            } else {
                DEV_CHK(dev.truncate(dev.ctx, j->w, j->bl[i].uoff), "truncate");
                n_new = j->bl[i].uoff;
                damaged = 1;
                break;
            }
        }
    if (j->trunc != SIZE_MAX && !damaged && j->trunc <= n_new) {
        DEV_CHK(dev.truncate(dev.ctx, j->w, j->trunc), "truncate");
        n_new = j->trunc;
    }
    t_inflate += now_s() - tq;
    r->dv.dring_n[j->w] = n_new;
    r->dv.dring_eof[j->w] = j->last || damaged;
    if (damaged && r->rg.rg_on) r->rg.rg_suspect = 1;
}

/* The producer (read-ahead thread): begin a push whenever a window and a lane are free and input is left, end the oldest
 * one otherwise. */
void *dev_producer(void *arg)
{
    aln_reader *r = arg;
    pthread_mutex_lock(&r->cm.pf_mu);
    for (;;) {
        int act = 0;                                               /* 1 begin, 2 end */
        while (!r->cm.pf_stop) {
            const long begun = r->dv.dk_begin, ready = r->dv.dk_ready, cur = r->dv.dk_cur;
            if (!r->dv.dinput_done && begun - cur < dev_nwin && begun - ready < pushes_in_flight()) {
                act = 1;
                break;
            }
            if (begun > ready) {
                act = 2;
                break;
            }
            pthread_cond_wait(&r->cm.pf_cv, &r->cm.pf_mu);
        }
        if (r->cm.pf_stop) break;
        pthread_mutex_unlock(&r->cm.pf_mu);
        if (act == 1) {
            dev_begin(r);
            pthread_mutex_lock(&r->cm.pf_mu);
            if (r->dv.dj[(r->dv.dk_begin - 1) % pushes_in_flight()].last) r->dv.dinput_done = 1;
        } else {
            dev_end(r);
            pthread_mutex_lock(&r->cm.pf_mu);
            if (r->dv.dring_eof[r->dv.dk_ready % dev_nwin]) r->dv.dinput_done = 1;
            r->dv.dk_ready++;
            pthread_cond_broadcast(&r->cm.pf_cv);
        }
    }
    pthread_mutex_unlock(&r->cm.pf_mu);
    return NULL;
}

/* chunk k's window is the one being consumed from now on: the window left behind is free */
static void dev_set_cur(aln_reader *r, long k)
{
    if (r->cm.pf_on) pthread_mutex_lock(&r->cm.pf_mu);
    r->dv.dk_cur = k;
    if (r->cm.pf_on) {
        pthread_cond_broadcast(&r->cm.pf_cv);
        pthread_mutex_unlock(&r->cm.pf_mu);
    }
}

/* The next window becomes the current one: the unconsumed tail (a partial record, or header bytes) moves in front of its
 * fresh bytes. Synchronous while the header is read, fed by the producer afterwards. Returns bytes added. */
static size_t dev_advance(aln_reader *r)
{
    if (r->cm.eof) return 0;
    const long nxt = r->dv.dk_cur + 1;
    if (!r->cm.pf_on) {
        if (r->dv.dk_begin <= nxt) dev_begin(r);
        while (r->dv.dk_ready <= nxt) {
            dev_end(r);
            r->dv.dk_ready++;
        }
    } else {
        pthread_mutex_lock(&r->cm.pf_mu);
        while (r->dv.dk_ready <= nxt) pthread_cond_wait(&r->cm.pf_cv, &r->cm.pf_mu);
        pthread_mutex_unlock(&r->cm.pf_mu);
    }
    const int w = (int)(nxt % dev_nwin);
    if (r->dv.dk_cur >= 0) {
        if (r->rg.rg_on && r->rg.rg_lo_block) {
            /* a share that starts at a guessed record start: a record "too long to carry" is what a false start looks
             * like — the share ends here, unverified, and the job is done again by one rank */
            if (dev.carry(dev.ctx, r->dv.dw, w) != 0) {
                r->rg.rg_suspect = 1;
                r->cm.eof = 1;
                r->dv.dlast = 1;
                dev_set_cur(r, nxt);
                r->dv.dparsed = 1;
                r->dv.dn_rec = r->dv.drec_next = 0;
                return 0;
            }
        } else {
            DEV_CHK(dev.carry(dev.ctx, r->dv.dw, w), "carry");
        }
    }
    dev_set_cur(r, nxt);
    r->dv.dw = w;
    r->dv.dparsed = 0;
    r->dv.dn_rec = r->dv.drec_next = 0;
    if (r->dv.dring_eof[w]) r->cm.eof = 1;
    if (r->dv.dskip_left) {                                           /* a share starts rg_skip bytes into its first block */
        size_t av = 0;
        DEV_CHK(dev.avail(dev.ctx, w, &av), "avail");
        const size_t sk = av < r->dv.dskip_left ? av : r->dv.dskip_left;
        DEV_CHK(dev.skip(dev.ctx, w, sk), "skip");
        r->dv.dskip_left -= sk;
    }
    return r->dv.dring_n[w];
}

/* sequential read of n bytes from the device window's front (header parsing): through a host copy fetched 1 MiB at a time */
size_t dev_read(aln_reader *r, void *dst, size_t n)
{
    for (;;) {
        if (r->dv.hdr_len - r->dv.hdr_pos >= n) {
            memcpy(dst, r->dv.hdr + r->dv.hdr_pos, n);
            r->dv.hdr_pos += n;
            return n;
        }
        size_t avail = 0;
        DEV_CHK(dev.avail(dev.ctx, r->dv.dw, &avail), "avail");
        if (avail > r->dv.hdr_len) {                                  /* more of this window */
            size_t want = r->dv.hdr_pos + n > r->dv.hdr_len + (1u << 20) ? r->dv.hdr_pos + n : r->dv.hdr_len + (1u << 20);
            if (want > avail) want = avail;
            r->dv.hdr = xrealloc(r->dv.hdr, want);
            DEV_CHK(dev.peek(dev.ctx, r->dv.dw, r->dv.hdr_len, r->dv.hdr + r->dv.hdr_len, want - r->dv.hdr_len), "peek");
            r->dv.hdr_len = want;
            continue;
        }
        /* the window is used up: what was read is consumed, the rest travels to the next window */
        if (r->cm.eof) {
            const size_t k = r->dv.hdr_len - r->dv.hdr_pos;
            memcpy(dst, r->dv.hdr + r->dv.hdr_pos, k);
            r->dv.hdr_pos += k;
            return k;
        }
        DEV_CHK(dev.skip(dev.ctx, r->dv.dw, r->dv.hdr_pos), "skip");
        r->dv.hdr_len = r->dv.hdr_pos = 0;
        dev_advance(r);
    }
}

/* The device decoder's batch: the records of the current window are located and parsed on the device in one go; a batch
 * is a slice of them copied into the staging arrays. Read names and XA / NM strings, when somebody wants them, are cut
 * out of the records' raw bytes, fetched for just the records concerned. */
/* makes drec_next < dn_rec: parses the current window, moves on to the next one when it is used up; 0 at end of input */
static int dev_ensure_records(aln_reader *r)
{
    if (!r->cm.pf_on && !r->cm.eof) pf_start(r);
    while (r->dv.drec_next == r->dv.dn_rec) {
        if (!r->dv.dparsed) {
            const double th = now_s();
            int malformed = 0, flags = 0;
            size_t redo = 0;
            DEV_CHK(dev.parse(dev.ctx, r->dv.dw, r->cm.n_targets, &r->dv.dn_rec, &malformed, &flags, &redo), "parse");
            t_hop += now_s() - th;
            r->dv.dparsed = 1;
            r->dv.drec_next = 0;
            r->dv.d_rewalked += redo;
            r->dv.dflags = flags;
            r->dv.dseen_ok = 0;
            if (malformed) {
                r->dv.dlast = 1;                                  /* bam.c:186-190: nothing after this window counts */
                if (r->rg.rg_on) r->rg.rg_suspect = 1;               /* ... of the whole file: the other shares must not count either */
            }
            if (r->dv.win_hook && r->dv.dn_rec) r->dv.win_hook(r->dv.win_hook_ctx, r->dv.dn_rec);
            continue;
        }
        if (r->dv.dlast || r->cm.eof) {                              /* end of input (a truncated tail record is dropped) */
            if (r->rg.rg_on && r->rg.rg_end_block != SIZE_MAX && !r->rg.rg_verified) {
                /* the share's end is a true record start iff the chain of records arrives exactly there: nothing is left over */
                size_t left = 1;
                DEV_CHK(dev.avail(dev.ctx, r->dv.dw, &left), "avail");
                r->rg.rg_verified = (r->rg.rg_stop_hit && !r->rg.rg_stop_missed && !r->dv.dlast && left == 0 && r->dv.dskip_left == 0) ? 1 : -1;
            }
            return 0;
        }
        dev_advance(r);
    }
    return 1;
}

int aln_device_window(aln_reader *r, int *flags, const uint8_t **tid_seen)
{
    if (!r->dv.dev || !dev_ensure_records(r) || r->dv.drec_next != 0) return 0;
    if (!r->dv.dseen_ok) {
        r->dv.dseen = xrealloc(r->dv.dseen, (size_t)r->cm.n_targets + 1);
        DEV_CHK(dev.tids(dev.ctx, r->dv.dseen, r->cm.n_targets), "tids");
        r->dv.dseen_ok = 1;
    }
    *flags = r->dv.dflags;
    *tid_seen = r->dv.dseen;
    return 1;
}

void aln_set_window_hook(aln_reader *r, void (*fn)(void *ctx, size_t n_rec), void *ctx)
{
    r->dv.win_hook = fn;
    r->dv.win_hook_ctx = ctx;
}

size_t aln_device_left(const aln_reader *r) { return r->dv.dev ? r->dv.dn_rec - r->dv.drec_next : 0; }

int aln_device_xa_veto(aln_reader *r, itx_xaveto *x, size_t n, uint64_t *n_vetoed, uint64_t *n_hard)
{
    if (!r->dv.dev || !dev.xa_veto || n > r->dv.drec_next) return -1;
    DEV_CHK(dev.xa_veto(dev.ctx, x, r->dv.drec_next - n, n, n_vetoed, n_hard), "xa_veto");
    return 0;
}

int aln_device_bed(aln_reader *r, itx_bed *b, size_t n, uint64_t *n_hard)
{
    if (!r->dv.dev || !dev.bed || n > r->dv.drec_next) return -1;
    DEV_CHK(dev.bed(dev.ctx, b, r->dv.drec_next - n, n, n_hard), "bed");
    return 0;
}

int aln_device_names(aln_reader *r, itx_names *nm, size_t n, const int32_t *d_hit_row, void *stream, uint64_t *n_hard)
{
    if (!r->dv.dev || !dev.names || n > r->dv.drec_next) return -1;
    DEV_CHK(dev.names(dev.ctx, nm, r->dv.drec_next - n, n, d_hit_row, stream, n_hard), "names");
    return 0;
}

int aln_device_bamout(aln_reader *r, itx_bamout *bo, size_t n, const int32_t *d_hit_row, void *stream)
{
    if (!r->dv.dev || !dev.bamout || n > r->dv.drec_next) return -1;
    DEV_CHK(dev.bamout(dev.ctx, bo, r->dv.drec_next - n, n, d_hit_row, stream), "bamout");
    return 0;
}

void aln_device_rewind(aln_reader *r, size_t n)
{
    if (r->dv.dev && r->dv.dparsed) r->dv.drec_next = n <= r->dv.drec_next ? r->dv.drec_next - n : 0;
}

int aln_device_exhausted(aln_reader *r) { return r->dv.dev && !dev_ensure_records(r); }

size_t aln_read_batch_device(aln_reader *r, size_t cap, itx_batch *b)
{
    if (!r->dv.dev || !dev_ensure_records(r)) return 0;
    size_t m = r->dv.dn_rec - r->dv.drec_next;
    if (m > cap) m = cap;
    DEV_CHK(dev.device_batch(dev.ctx, r->dv.drec_next, r->dv.dflags & 1, b), "device_batch");
    r->dv.drec_next += m;
    return m;
}

size_t dev_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa)
{
    size_t n = 0;
    while (n < cap) {
        if (r->dv.drec_next == r->dv.dn_rec) {
            if (n) break;                                          /* a batch stays inside one window */
            if (!dev_ensure_records(r)) break;
        }
        size_t m = r->dv.dn_rec - r->dv.drec_next;
        if (m > cap - n) m = cap - n;
        const double tp = now_s();
        const int want_q = side && side->want_qnames, want_a = side && side->want_aux && (r->dv.dflags & 2);
        const int want_r = side && side->want_raw;                     /* filter -b: the records' bytes themselves */
        if (want_r && n == 0) side->raw_len = 0;
        if (want_q || want_a || want_r) {
            if (r->dv.d_side_cap < m + 1) {
                r->dv.d_side_cap = m + m / 4 + 1;
                r->dv.d_off = xrealloc(r->dv.d_off, sizeof(uint32_t) * r->dv.d_side_cap);
                r->dv.d_xa = xrealloc(r->dv.d_xa, r->dv.d_side_cap);
            }
            DEV_CHK(dev.fetch(dev.ctx, r->dv.drec_next, m, st, n, r->dv.d_off, r->dv.d_xa), "fetch");
            /* the raw bytes from the first wanted record to the end of the last one */
            size_t i0 = 0, i1 = m;
            if (!want_q && !want_r) {
                while (i0 < m && !r->dv.d_xa[i0]) i0++;
                while (i1 > i0 && !r->dv.d_xa[i1 - 1]) i1--;
            }
            if (i1 > i0) {
                uint8_t lenb[4];
                DEV_CHK(dev.bytes(dev.ctx, r->dv.d_off[i1 - 1], lenb, 4), "bytes");
                const size_t lo = r->dv.d_off[i0], hi = (size_t)r->dv.d_off[i1 - 1] + 4 + (size_t)rd_u32(lenb);
                if (r->dv.d_raw_cap < hi - lo) {
                    r->dv.d_raw_cap = (hi - lo) + (hi - lo) / 4;
                    free(r->dv.d_raw);
                    r->dv.d_raw = xmalloc(r->dv.d_raw_cap);
                }
                DEV_CHK(dev.bytes(dev.ctx, lo, r->dv.d_raw, hi - lo), "bytes");
                const uint8_t *raw = r->dv.d_raw;
                const uint32_t *ro = r->dv.d_off;
                const uint8_t *xa = r->dv.d_xa;
                if (want_r) {                                      /* kept with the slot until its chosen rows are back */
                    if (side->raw_cap < side->raw_len + (hi - lo)) {
                        side->raw_cap = (side->raw_len + (hi - lo)) + (hi - lo) / 4;
                        side->raw = xrealloc(side->raw, side->raw_cap);
                    }
                    memcpy(side->raw + side->raw_len, raw, hi - lo);
                    for (size_t i = 0; i < m; i++) side->raw_off[n + i] = side->raw_len + (ro[i] - lo);
                    side->raw_len += hi - lo;
                }
#pragma omp parallel for schedule(static)
                for (long i = (long)i0; i < (long)i1; i++)
                    if (want_q || (want_a && xa[i])) {
                        int a1 = 0, x1 = 0;
                        const uint8_t marked = st->flag5[n + (size_t)i] & ITX_F5_NOLOOKUP;       /* set on the device (-R): the record's bytes do not hold it */
                        bam_parse_one(raw + (ro[i] - lo), n + (size_t)i, st, side, &a1, &x1);   /* the same field values again, plus the strings */
                        st->flag5[n + (size_t)i] |= marked;
                    }
            }
            if (want_q || want_a) side->has_strings = 1;                 /* entries outside [i0, i1) were never written: still NULL */
        } else {
            DEV_CHK(dev.fetch(dev.ctx, r->dv.drec_next, m, st, n, NULL, NULL), "fetch");
        }
        t_parse += now_s() - tp;
        if (r->dv.dflags & 1) *any_paired = 1;
        if (r->dv.dflags & 2) *aux_xa = 1;
        r->dv.drec_next += m;
        n += m;
    }
    return n;
}


void dev_close(aln_reader *r)
{
    if (r->dv.dev)
        while (r->dv.dk_ready < r->dv.dk_begin) {                     /* pushes still in flight: the lanes must be idle for the next file */
            dev_end(r);
            r->dv.dk_ready++;
        }
    free(r->dv.dblk);
    free(r->dv.dstatus);
    for (int k = 0; k < ITX_BAMWIN_LANES; k++) free(r->dv.dj[k].bl);
    free(r->dv.hdr);
    free(r->dv.dseen);
    free(r->dv.d_off);
    free(r->dv.d_xa);
    free(r->dv.d_raw);
}
