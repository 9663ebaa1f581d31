/* aln_priv.h — what the pieces of the alignment reader share and nobody else sees: bgzf.c (the BGZF member and the plain
 * sequential reader), bamio.c (open / close / dispatch, the BAM header, the host BAM route), bamdev.c (the device decoder's
 * feeder) and samio.c (SAM text). The first half knows no reader; bgzf.c takes only that half (ALN_PRIV_NO_READER). */
#ifndef ALN_PRIV_H
#define ALN_PRIV_H
#include "itx_host.h"
#include "../csrc/itx_auxwalk.h"

#include <ctype.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>

#define BGZF_MAX 0x10000

static inline int32_t rd_i32(const uint8_t *p) { return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24); }
static inline uint32_t rd_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* Does a BAM record that looks like one start at u[p], in a run of inflated bytes that may end inside it? *step = the record's bytes when it is well-formed
 * and complete; returns 1 then, 0 when what is there rules a record out, -1 when only more data can tell (the fixed part
 * or the record's end lies beyond u[0, L)) */
static inline int record_or_short(const uint8_t *u, size_t p, size_t L, int n_targets, size_t *step)
{
    if (p + 36 > L) return -1;
    const int32_t bl = rd_i32(u + p);
    if (bl < 32) return 0;
    const uint8_t *core = u + p + 4;
    const int32_t tid = rd_i32(core), pos = rd_i32(core + 4), l_qseq = rd_i32(core + 16), mtid = rd_i32(core + 20), mpos = rd_i32(core + 24);
    const uint32_t x1 = rd_u32(core + 8), x2 = rd_u32(core + 12);
    const size_t l_qname = x1 & 0xff, n_cigar = x2 & 0xffff;
    if (tid < -1 || tid >= n_targets || mtid < -1 || mtid >= n_targets || pos < -1 || mpos < -1 || l_qseq < 0 || l_qname == 0) return 0;
    const size_t need = l_qname + 4 * n_cigar + ((size_t)l_qseq + 1) / 2 + (size_t)l_qseq;
    if (need > (size_t)bl - 32) return 0;
    if (p + 36 + l_qname > L) return -1;
    if (u[p + 36 + l_qname - 1] != 0) return 0;
    if (p + 4 + (size_t)bl > L) return -1;
    *step = 4 + (size_t)bl;
    return 1;
}

struct blk {
    size_t coff, csize, uoff, usize;
};

/* ---- bgzf.c ------------------------------------------------------------------------------------------------------------- */
int bgzf_header_ok(const uint8_t *h);
size_t bgzf_member_size(const uint8_t *h);
int bgzf_member(const uint8_t *p, size_t n, size_t *csize, size_t *usize);
void ld_probe(void);
const char *inflater_name(void);             /* "libdeflate" or "zlib": who inflates on the host (ITX_TIMING) */
int inflate_block(const uint8_t *src, size_t csize, uint8_t *dst, size_t usize);
size_t index_blocks(const uint8_t *buf, size_t len, struct blk **blk, size_t *blk_cap, size_t max_blocks, size_t max_utot, size_t *poff,
                    size_t *putot, int *pdamaged, int *pcapped);
/* a plain sequential BGZF reader on the host (pread + one block at a time) */
typedef struct {
    int fd;
    size_t off, size;          /* the next block starts at file offset off; size of the file                         */
    uint8_t *u;                /* inflated bytes so far                                                               */
    size_t len, cap, pos;
    struct blk *b;             /* the blocks behind u: coff = file offset, csize, uoff, usize                         */
    size_t nb, bcap;
} hz_t;
size_t hz_read(hz_t *z, void *dst, size_t n);
void hz_free(hz_t *z);
int find_split(int fd, size_t fsize, size_t at, int n_targets, size_t *pB, size_t *pc, size_t *pcsize);

#ifndef ALN_PRIV_NO_READER
extern double t_io, t_inflate, t_hop, t_parse;          /* ITX_TIMING: where the decoder's wall time goes */

#define N_RAW_DEVICE (ITX_BAMWIN_LANES + 2)
#define N_RAW_DEVICE_FILE ALN_DEVICE_RAW_BUFFERS

/* Who touches what. The CONSUMER is the caller's thread (aln_open, aln_read_batch, aln_device_*, aln_close). Up to three more
 * threads belong to a reader: the IO thread (bamio.c io_main) reads the file ahead; the READ-AHEAD thread (pf_main) is the host
 * route's loader or, with the device decoder, its producer (bamdev.c dev_producer); the SAM thread (samio.c sam_chunk_thread /
 * sam_bgzf_thread) fills the text chunks. The INDEXER is whoever calls raw_next and cuts blocks from what it returns: the
 * consumer while the header is read, the read-ahead thread afterwards (the two never run at the same time: the thread is
 * started once the header is through). */
struct aln_reader {
    /* common: the file, the header, the reference names, the read-ahead thread's handle. Written by the open functions before
     * any thread exists and read-only afterwards, except: eof is the consumer's alone; pf_stop is written by the consumer and
     * read by the read-ahead thread under pf_mu, which also guards what the `hb` and `dv` groups say it guards; and f, which
     * the SAM thread reads (sam_chunk_thread), is closed and opened anew by the consumer in sam_hand_over, between the end of one
     * SAM thread and the start of the next. */
    struct {
        FILE *f;
        int is_sam;
        /* header */
        int n_targets;
        char **tname;
        names_t tnames;
        uint8_t *hdr_raw;         /* aln_keep_header: the BAM header's bytes as they were read                     */
        size_t hdr_raw_len, hdr_raw_cap;
        int eof;                  /* no more compressed input (end of file or a damaged block)                     */
        int pf_on, pf_stop;
        pthread_t pf_thread;
        pthread_mutex_t pf_mu;
        pthread_cond_t pf_cv;
    } cm;
    /* raw read-ahead (raw_next): a reader thread freads the next compressed chunk while this one is being inflated.
     * Under io_mu, IO thread and indexer: io_fill, io_take, io_got, io_eof_seen, io_stop, raw_lanes (the producer sets a lane's
     * bit in dev_begin, the IO thread takes the bits). The indexer's alone: cbuf, clen, raw_cur, io_abs_end, io_done, n_raw,
     * raw_step (the last two fixed before the IO thread starts). The IO thread's alone once it runs: io_off, and craw[b] of the
     * buffer it fills. */
    struct {
        /* BGZF state: the file is consumed in chunks of many blocks; the blocks of a chunk are inflated in parallel
         * (they are independent gzip members), then records are located by one sequential hop over the block_len
         * fields and parsed in parallel straight into the staging SoA */
        uint8_t *cbuf;            /* compressed bytes of the current chunk (+ the incomplete block carried over):   */
        size_t clen;              /* a window into one of the two raw buffers below                                 */
        uint8_t *craw[N_RAW_DEVICE]; /* two for the host decoder. The device's, from a regular file: one being indexed, one whose pushes are
                                      * copying, the others read ahead (a buffer is free again once the pushes cut from it have COPIED their bytes: a
                                      * block the device declines is read from the file once more); from a pipe: one per push in flight + 2, held
                                      * until the push ends */
        uint32_t raw_lanes[N_RAW_DEVICE];   /* per buffer: the lanes whose pushes read their compressed bytes from it (bit s = lane s) */
        int n_raw, raw_cur;          /* raw_cur: the buffer cbuf points into */
        size_t io_got[N_RAW_DEVICE];      /* bytes the reader put into each buffer */
        long io_fill, io_take;       /* chunks read so far / taken by raw_next so far (chunk f lives in buffer f % n_raw) */
        int io_eof_seen;             /* the reader has met a short read: it reads no further */
        int io_fd;                /* >= 0: a regular file, read with pread at io_off (of io_size bytes)              */
        size_t io_off, io_size;
        size_t raw_step;          /* bytes per read step (aln_raw_step) */
        int io_on, io_stop, io_done; /* io_done: the file is read out and its last chunk taken */
        size_t io_abs_end;        /* file offset behind the last byte raw_next has delivered                           */
        pthread_t io_thread;
        pthread_mutex_t io_mu;
        pthread_cond_t io_cv;
    } raw;
    /* a share of the file (aln_open_range; one rank of a multi-GPU job): the stream starts at the BGZF block at byte
     * rg_lo_block of the file, rg_skip inflated bytes into it, and ends where the next share starts: rg_end_off bytes into
     * the block at rg_end_block (SIZE_MAX: at the end of the file).
     * The boundaries are written by aln_open_range and read-only afterwards. rg_stop_hit and rg_stop_missed are the indexer's
     * (dev_begin); the consumer reads them only behind the last window, which reaches it through pf_mu. rg_verified is the
     * consumer's. rg_suspect is set, never cleared, by indexer and consumer alike without a lock, and read after the last batch. */
    struct {
        int rg_on;
        size_t rg_lo_block, rg_skip, rg_end_block, rg_end_off, rg_end_csize;
        int rg_stop_hit, rg_stop_missed, rg_verified;
        int rg_suspect;           /* something a false start (or damaged input) explains: the share is not to be trusted */
    } rg;
    /* host inflate and hop. The consumer's: hz, ubuf .. hop_redone. blk is the indexer's (bgzf_inflate_chunk). nbuf, ncap, nlen
     * and n_eof are the loader's while pf_state == 1 and the consumer's otherwise; pf_state changes under pf_mu. */
    struct {
        void *hz;                 /* while the header is read by the plain host reader (a share that starts inside the file) */
        uint8_t *ubuf;            /* inflated bytes: unconsumed tail of the previous chunk + this chunk            */
        size_t ulen, upos, ucap;
        size_t *rec_off;          /* start of every complete record in ubuf                                        */
        size_t n_rec, rec_next, rec_cap;
        size_t *spec;             /* locate_records: the pieces' starts before they are accepted                    */
        size_t spec_cap, hop_pieces, hop_redone;
        struct blk *blk;          /* block index of the chunk being inflated                                        */
        size_t blk_cap;
        /* read-ahead (bgzf_load_chunk): spare buffer the loader thread inflates the next chunk into */
        uint8_t *nbuf;
        size_t ncap, nlen;
        int n_eof, pf_state;      /* pf_state: 0 idle, 1 requested, 2 ready */
    } hb;
    /* device decoder (aln_use_device): two windows of inflated bytes live on the device, dw is the one being consumed.
     * Under pf_mu, producer and consumer: dk_begin, dk_ready, dk_cur, dinput_done; dring_n / dring_eof of a window are written
     * by dev_end before dk_ready is published and read by the consumer after it. The indexer's (dev_begin, dev_end): dmore, dj,
     * dblk, dstatus, dblk_cap, dstream_total. Everything else is the consumer's. */
    struct {
        int dev, dw, dparsed, dlast, dflags, dseen_ok, dmore, dinput_done;
        long dk_begin, dk_ready, dk_cur;   /* chunks whose push was begun / has ended; the chunk whose window is being consumed (-1 none) */
        struct dev_job {
            struct blk *bl;        /* the chunk's blocks and where its compressed bytes lie, kept until its push has ended */
            size_t bl_cap, nb;
            const uint8_t *cbase;
            size_t cabs;           /* file offset of cbase (regular files: SIZE_MAX otherwise) */
            int w, last;
            size_t trunc;          /* SIZE_MAX, or: the window ends this many fresh bytes in (the share's end boundary) */
        } dj[ITX_BAMWIN_LANES];
        size_t dring_n[ITX_BAMWIN_WINDOWS];
        int dring_eof[ITX_BAMWIN_WINDOWS];
        size_t dstream_total;     /* inflated bytes of all blocks indexed before the current chunk (from rg_lo_block)  */
        size_t dskip_left;        /* inflated bytes still to be skipped at the front of the stream                     */
        uint8_t *dseen;           /* references with a mapped record in the current window                             */
        size_t dn_rec, drec_next, d_rewalked;
        itx_bgzf_block *dblk;     /* block index of a chunk for the device, and its per-block verdicts                */
        uint8_t *dstatus;
        size_t dblk_cap;
        uint8_t *hdr;             /* host copy of the window's front while the header is parsed                       */
        size_t hdr_len, hdr_pos;
        uint32_t *d_off;          /* side channels: offsets, XA marks and raw bytes of a batch's records              */
        uint8_t *d_xa, *d_raw;
        size_t d_side_cap, d_raw_cap;
        void (*win_hook)(void *, size_t);   /* aln_set_window_hook */
        void *win_hook_ctx;
    } dv;
    /* SAM state. Under sc_mu, SAM thread and consumer: sc_fill, sc_take, sc_stop. A chunk sc[k] and the tail (sc_tail*) are the
     * SAM thread's while it fills them — chunk sc_fill, before the count goes up — and the consumer's from then until sc_take
     * passes the chunk. sz_off and sz_skip are the SAM thread's while it runs (sam_bgzf_thread), sz_host_chunks and t_io are
     * written by it unlocked and read after it has been joined. f is read by the SAM thread (sam_chunk_thread) and replaced
     * only while no such thread runs (sam_hand_over). Everything else is the consumer's. */
    struct {
        char *line;
        size_t line_cap;
        ssize_t pending_len;     /* first alignment line read while scanning the header, -1 none */
        long long n_lines;
        /* SAM in chunks (sam_chunks_start): a read-ahead thread fills two text buffers, each cut behind its last newline; with a
         * device object attached it also begins the chunk's parse there, so chunk k + 1 crosses the link while chunk k is consumed */
        int sc_on, sc_done;
        size_t sc_chunk;
        int sdev_on;
        aln_sam_device sdev;
        struct sam_chunk {
            uint8_t *buf;
            size_t cap, len;
            int final, begun, begin_rc, from_alloc;
            /* a chunk of BGZF members for the device to inflate (sam_bgzf_thread): the host has no copy of its text */
            int bgzf, handover;   /* handover: the decoder cannot take it, nothing was begun; `why` says what is wrong */
            uint8_t *cbuf;        /* the members' bytes */
            size_t ccap, clen, coff, utot, skip_before;     /* coff: the first member's file offset; skip_before: header bytes not yet skipped there */
            int c_from_alloc;
            struct blk *bl;       /* the members at hand, as index_blocks gives them, and as the device takes them */
            size_t bl_cap;
            itx_bgzf_block *zb;
            size_t zb_cap;
            char why[128];
        } sc[2];
        uint8_t *sc_tail;         /* the bytes behind the last newline of the chunk before */
        size_t sc_tail_len, sc_tail_cap;
        long sc_fill, sc_take;    /* chunks filled / consumed so far (chunk k lives in buffer k % 2) */
        int sc_stop;
        pthread_t sc_thread;
        pthread_mutex_t sc_mu;
        pthread_cond_t sc_cv;
        int sc_open, sc_host;     /* a chunk is being consumed; by the host's line parser */
        size_t sc_pos;            /* host: the next line's first byte */
        uint64_t sc_nrec, sc_next, sc_lines;   /* device: records of the chunk, the next one to hand out, its lines */
        int sc_flags;
        uint32_t *s_off, *s_qlen, *s_xoff, *s_xlen;   /* a batch's side values from the device */
        int32_t *s_nm;
        uint8_t *s_mark;
        size_t s_cap;
        unsigned long long st_dev_chunks, st_dev_bytes, st_host_chunks;   /* ITX_TIMING */
        double st_ms, st_wait;
        char st_reason[96];
        /* -S input through zlib; BGZF inflated on the device */
        int sam_fd;               /* the file's own descriptor (-1 none): the compressed bytes are read from it with pread   */
        int sz_gz, sz_bgzf;       /* the file starts with the gzip magic / its first member is BGZF                          */
        size_t sz_hdr;            /* inflated bytes of the header lines                                                      */
        int sz_on;                /* the device inflates: until a hand-over, which is for good                               */
        size_t sz_off, sz_skip;   /* the next member's file offset; header bytes the device stream has still to skip        */
        int sz_prev_slot;         /* where the last device chunk left its tail (-1: there is none): a hand-over's carry      */
        size_t sz_prev_at, sz_prev_tail;
        unsigned long long sz_dev_chunks, sz_comp_bytes, sz_infl_bytes, sz_host_chunks;   /* ITX_TIMING */
        double sz_inflate_ms, sz_gather_ms;
        char sz_reason[200];
    } sam;
};

/* ---- bamio.c ------------------------------------------------------------------------------------------------------------ */
aln_reader *reader_new(FILE *f);
void add_target(aln_reader *r, const char *name);
size_t raw_next(aln_reader *r);
void pf_start(aln_reader *r);

/* ---- bamdev.c ----------------------------------------------------------------------------------------------------------- */
uint8_t *buf_alloc(size_t n);
void buf_free(uint8_t *p);
uint8_t *buf_grow(uint8_t *old, size_t keep, size_t ncap);
int dev_attached(void);
int dev_raw_buffers(int regular_file);
void dev_pushes_copied(uint32_t lanes);
void dev_drain_windows(void);
void dev_header_done(aln_reader *r);
void *dev_producer(void *arg);
size_t dev_read(aln_reader *r, void *dst, size_t n);
size_t dev_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa);
void dev_close(aln_reader *r);

/* ---- samio.c ------------------------------------------------------------------------------------------------------------ */
aln_reader *sam_open(const char *path);
size_t sam_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa);
void sam_close(aln_reader *r);

/* ---- one BAM record in memory: shared by the host route and the device route's side channel, inlined into their loops ---- */
static inline char *xstrndup_bound(const char *s, size_t max)
{
    const size_t k = strnlen(s, max);
    char *d = xmalloc(k + 1);
    memcpy(d, s, k);
    d[k] = 0;
    return d;
}

/* bam.c:179-210 for one record that is completely in memory */
static inline void bam_parse_one(const uint8_t *p, size_t n, itx_staging *st, aln_side *side, int *any_paired, int *aux_xa)
{
    const int32_t block_len = rd_i32(p);
    const uint8_t *core = p + 4, *data = p + 36;
    const size_t dlen = (size_t)block_len - 32;
    const int32_t tid = rd_i32(core), pos = rd_i32(core + 4);
    const uint32_t x1 = rd_u32(core + 8), x2 = rd_u32(core + 12);
    const uint32_t l_qname = x1 & 0xff, qual = (x1 >> 8) & 0xff, flag = x2 >> 16, n_cigar = x2 & 0xffff;
    const int32_t l_qseq = rd_i32(core + 16), mpos = rd_i32(core + 24), isize = rd_i32(core + 28);
    int32_t tmpend;
    if (n_cigar && (size_t)l_qname + 4 * (size_t)n_cigar <= dlen) {
        uint32_t e = (uint32_t)pos;                               /* bam.c:17-27 */
        const uint8_t *cg = data + l_qname;
        for (uint32_t k = 0; k < n_cigar; k++) {
            const uint32_t c = rd_u32(cg + 4 * k), op = c & 0xf;
            if (op == 0 || op == 2 || op == 3) e += c >> 4;       /* M, D, N */
        }
        tmpend = (int32_t)e;
    } else {
        tmpend = (int32_t)((uint32_t)pos + (uint32_t)l_qseq);     /* generic.c:820 */
    }
    st->tid[n] = tid;
    st->pos[n] = pos;
    st->tmpend[n] = tmpend;
    st->mapq[n] = (uint8_t)qual;
    st->flag5[n] = ITX_FLAG5(flag);
    st->mpos[n] = mpos;
    st->isize[n] = isize;
    if (flag & 1) *any_paired = 1;
    if (side && side->want_qnames) side->qname[n] = xstrdup(l_qname && l_qname <= dlen ? (const char *)data : "");
    /* the optional fields as the reference walks and reads them: ../csrc/itx_auxwalk.h */
    const uint8_t *as, *ae, *xa = NULL, *nmv = NULL;
    if (itx_aux_bounds(p, &as, &ae)) itx_aux_find(as, ae, ITX_AUX_TAG('X', 'A'), &xa, ITX_AUX_TAG('N', 'M'), side && side->want_aux ? &nmv : NULL);
    if (xa) *aux_xa = 1;
    if (side && side->want_aux) {
        side->xa[n] = NULL;
        side->nm[n] = 0;
        if (xa) {
            /* bam_aux2Z (bam_aux.c:193-199): the string of a Z/H tag; an XA tag of another type has no string the
             * reference could copy (it would crash there) and reads as empty here */
            uint32_t xl;
            const uint8_t *z = itx_aux_str(xa, ae, &xl);
            side->xa[n] = xstrndup_bound((const char *)z, xl);
            side->nm[n] = itx_aux_int(nmv, ae);
        }
    }
}
#endif /* ALN_PRIV_NO_READER */
#endif
