/* samio.c — SAM text (-S): the header, the input through zlib, the line parser, and the reader in chunks whose text the
 * device splits and parses (and, for BGZF, inflates). Follows samtools 0.1.18 as vendored by the reference:
 * bam_import.c:237-330 (SAM text; a mapped record without CIGAR is flagged unmapped). Of the reader it touches the common
 * and SAM groups only (aln_priv.h). */
#define _GNU_SOURCE
#include "aln_priv.h"

#include <fcntl.h>
#include <stdarg.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

/* ---- SAM text header ------------------------------------------------------------------------------------- */
static int sam_read_header(aln_reader *r)
{
    r->sam.pending_len = -1;
    ssize_t len;
    while ((len = getline(&r->sam.line, &r->sam.line_cap, r->cm.f)) >= 0) {
        r->sam.n_lines++;
        if (r->sam.line[0] != '@') {
            r->sam.pending_len = len;
            break;
        }
        r->sam.sz_hdr += (size_t)len;
        if (strncmp(r->sam.line, "@SQ", 3) == 0) {
            char *sn = strstr(r->sam.line, "\tSN:");
            if (sn) {
                sn += 4;
                size_t k = strcspn(sn, "\t\r\n");
                char *nm = xmalloc(k + 1);
                memcpy(nm, sn, k);
                nm[k] = 0;
                add_target(r, nm);
                free(nm);
            }
        }
    }
    return 0;
}

/* ---- SAM input through zlib ------------------------------------------------------------------------------------------- */
/* The reference opens -S input with gzopen (bam_import.c:17,76,126), so plain gzip, bgzip's output and a mix of both are SAM
 * text to it, what lies behind the last member is ignored, and a file cut short gives what a streaming inflater gets out of it.
 * The same calls behind the FILE the reader already uses: a file without the gzip magic is passed through as it is. */
static ssize_t samz_read(void *c, char *buf, size_t n)
{
    const int got = gzread((gzFile)c, buf, n > (1u << 30) ? 1u << 30 : (unsigned)n);
    return got < 0 ? 0 : got;                                        /* a damaged stream ends the input, as it does there */
}

static int samz_close(void *c)
{
    return gzclose((gzFile)c) == Z_OK ? 0 : -1;
}

static FILE *samz_fopen(gzFile g)
{
    if (!g) return NULL;
    gzbuffer(g, 1u << 17);
    FILE *f = fopencookie(g, "r", (cookie_io_functions_t){.read = samz_read, .close = samz_close});
    if (!f) gzclose(g);
    return f;
}


aln_reader *sam_open(const char *path)
{
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return NULL;
    const int fd_own = dup(fd);
    FILE *f = samz_fopen(gzdopen(fd, "rb"));
    if (!f) {
        if (fd_own >= 0) close(fd_own);
        return NULL;
    }
    aln_reader *r = reader_new(f);
    r->cm.is_sam = 1;
    r->sam.sam_fd = fd_own;
    if (fd_own >= 0) {
        uint8_t h[18];
        const ssize_t got = pread(fd_own, h, sizeof h, 0);
        r->sam.sz_gz = got >= 2 && h[0] == 0x1f && h[1] == 0x8b;
        r->sam.sz_bgzf = got == (ssize_t)sizeof h && bgzf_header_ok(h);
    }
    if (sam_read_header(r) != 0) {
        aln_close(r);
        return NULL;
    }
    for (int i = 0; i < r->cm.n_targets; i++) names_intern(&r->cm.tnames, r->cm.tname[i]);    /* first occurrence wins a lookup */
    return r;
}

/* bam_import.c: the textual flag letters of samtools 0.1.x ("pPuUrR12sfd") */
static unsigned flag_from_chars(const char *s)
{
    unsigned f = 0;
    for (; *s; ++s) {
        switch (*s) {
        case 'p': f |= 0x1; break;
        case 'P': f |= 0x2; break;
        case 'u': f |= 0x4; break;
        case 'U': f |= 0x8; break;
        case 'r': f |= 0x10; break;
        case 'R': f |= 0x20; break;
        case '1': f |= 0x40; break;
        case '2': f |= 0x80; break;
        case 's': f |= 0x100; break;
        case 'f': f |= 0x200; break;
        case 'd': f |= 0x400; break;
        default: break;
        }
    }
    return f;
}

/* One line of SAM text (NUL-terminated at line[len], terminator excluded or not) into record *n of the staging slot:
 * 0 a record was taken (*n advanced), 1 the line is empty and skipped, 2 a truncated line: the parser gives up on this batch.
 * The line is cut up in place. r->sam.n_lines is the line's number (the warning prints it). */
static int sam_take_line(aln_reader *r, char *line, ssize_t len, itx_staging *st, size_t *np, aln_side *side, int *any_paired, int *aux_xa)
{
    const size_t n = *np;
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
    if (len == 0) return 1;                                          /* empty lines are skipped */
    char *fld[12];
    int nf = 0;
    char *p = line;
    while (nf < 12) {
        fld[nf++] = p;
        if (nf == 12) break;                                         /* the 12th "field" keeps all optional fields */
        char *t = strchr(p, '\t');
        if (!t) break;
        *t = 0;
        p = t + 1;
    }
    if (nf < 11) return 2;                                           /* truncated line: the parser gives up */
    char *endp;
    long flag = strtol(fld[1], &endp, 0);
    if (*endp) flag = (long)flag_from_chars(fld[1]);
    int32_t tid = -1;
    if (strcmp(fld[2], "*") != 0) {
        const int64_t t = names_find(&r->cm.tnames, fld[2]);
        if (t < 0) {
            if (r->cm.n_targets == 0) {
                fprintf(stderr, "[sam_read1] missing header? Abort!\n");
                exit(1);
            }
            fprintf(stderr, "[sam_read1] reference '%s' is recognized as '*'.\n", fld[2]);
        }
        tid = (int32_t)t;
    }
    const int32_t pos = isdigit((unsigned char)fld[3][0]) ? atoi(fld[3]) - 1 : -1;
    const int qual = isdigit((unsigned char)fld[4][0]) ? atoi(fld[4]) : 0;
    uint32_t e = (uint32_t)pos;
    int n_cigar = 0;
    if (fld[5][0] != '*') {
        const char *s = fld[5];
        while (*s) {
            char *t;
            const long x = strtol(s, &t, 10);
            const int op = toupper((unsigned char)*t);
            if (!*t) break;
            if (op == 'M' || op == 'D' || op == 'N') e += (uint32_t)x;
            n_cigar++;
            s = t + 1;
        }
    } else if (!(flag & 0x4)) {
        fprintf(stderr, "Parse warning at line %lld: mapped sequence without CIGAR\n", r->sam.n_lines);
        flag |= 0x4;
    }
    const int32_t mpos = isdigit((unsigned char)fld[7][0]) ? atoi(fld[7]) - 1 : -1;
    const int32_t isize = (fld[8][0] == '-' || isdigit((unsigned char)fld[8][0])) ? atoi(fld[8]) : 0;
    const int32_t l_qseq = strcmp(fld[9], "*") == 0 ? 0 : (int32_t)strlen(fld[9]);
    st->tid[n] = tid;
    st->pos[n] = pos;
    st->tmpend[n] = n_cigar ? (int32_t)e : (int32_t)((uint32_t)pos + (uint32_t)l_qseq);
    st->mapq[n] = (uint8_t)qual;
    st->flag5[n] = ITX_FLAG5((unsigned)flag);
    st->mpos[n] = mpos;
    st->isize[n] = isize;
    if (flag & 1) *any_paired = 1;
    if (side && side->want_qnames) side->qname[n] = xstrdup(fld[0]);
    if (side && side->want_aux) {
        side->xa[n] = NULL;
        side->nm[n] = 0;
    }
    if (nf == 12) {
        /* optional fields TAG:TYPE:VALUE (bam_import.c:402-470); the first XA and the first NM count (bam_aux_get) */
        const char *xa = NULL, *nm = NULL;
        for (char *a = fld[11]; a; a = strchr(a, '\t') ? strchr(a, '\t') + 1 : NULL) {
            if (!xa && strncmp(a, "XA:", 3) == 0) xa = a;
            if (!nm && strncmp(a, "NM:", 3) == 0) nm = a;
        }
        if (xa) *aux_xa = 1;
        if (xa && side && side->want_aux) {
            const int is_z = strlen(xa) >= 5 && (xa[3] == 'Z' || xa[3] == 'H') && xa[4] == ':';
            const char *v = is_z ? xa + 5 : "";
            side->xa[n] = xstrndup_bound(v, strcspn(v, "\t"));
            if (nm && strlen(nm) >= 5 && nm[3] == 'i' && nm[4] == ':') side->nm[n] = (int32_t)strtol(nm + 5, NULL, 10);
        }
    }
    *np = n + 1;
    return 0;
}

/* ---- SAM in chunks ------------------------------------------------------------------------------------------------------ */
size_t aln_sam_chunk_bytes(void)
{
    const char *e = getenv("ITX_SAM_CHUNK");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ALN_SAM_CHUNK;
}

void aln_set_sam_device(aln_reader *r, const aln_sam_device *d)
{
    if (!r->cm.is_sam || r->sam.sc_on) return;                              /* before the first batch only */
    r->sam.sdev_on = d && d->obj && d->parse_begin;
    if (r->sam.sdev_on) r->sam.sdev = *d;
}

static void sam_buf_release(aln_reader *r, uint8_t *p, int from_alloc)
{
    if (!p) return;
    if (from_alloc) r->sam.sdev.release(p);
    else free(p);
}

/* a call into the device object that must not fail; `what` ends with ": ", or is empty */
#define SDEV_CHK(call, what)                                                                                                 \
    do {                                                                                                                     \
        if ((call) != 0) die("SAM text on the device: " what "%s", r->sam.sdev.last_error ? r->sam.sdev.last_error() : "?"); \
    } while (0)

/* room for n bytes in a buffer, the first `keep` ones preserved: from the device's `alloc` (page-locked) when it gives */
static void sam_room(aln_reader *r, uint8_t **buf, size_t *pcap, int *from_alloc, size_t n, size_t keep)
{
    if (*pcap >= n) return;
    const size_t cap = n + n / 8 + 4096;
    uint8_t *p = r->sam.sdev_on && r->sam.sdev.alloc ? r->sam.sdev.alloc(cap) : NULL;
    const int fa = p != NULL;
    if (!p) p = xmalloc(cap);
    if (keep) memcpy(p, *buf, keep);
    sam_buf_release(r, *buf, *from_alloc);
    *buf = p;
    *pcap = cap;
    *from_alloc = fa;
}

/* ... in the chunk's text buffer */
static void sam_buf_need(aln_reader *r, struct sam_chunk *c, size_t n, size_t keep) { sam_room(r, &c->buf, &c->cap, &c->from_alloc, n, keep); }

/* the read-ahead thread's side of the two chunk buffers: waits until one is free (0: the reader is being closed) ... */
static int sam_slot_wait(aln_reader *r)
{
    pthread_mutex_lock(&r->sam.sc_mu);
    while (!r->sam.sc_stop && r->sam.sc_fill - r->sam.sc_take >= 2) pthread_cond_wait(&r->sam.sc_cv, &r->sam.sc_mu);
    const int stop = r->sam.sc_stop;
    pthread_mutex_unlock(&r->sam.sc_mu);
    return !stop;
}

/* ... and hands the chunk it has filled to the consumer */
static void sam_slot_filled(aln_reader *r)
{
    pthread_mutex_lock(&r->sam.sc_mu);
    r->sam.sc_fill++;
    pthread_cond_broadcast(&r->sam.sc_cv);
    pthread_mutex_unlock(&r->sam.sc_mu);
}

/* the consumer's side: ends the read-ahead thread, and the parses it has begun that nobody took (the object must be idle when
 * it is destroyed, or when the host takes the file over) */
static void sam_thread_stop(aln_reader *r)
{
    pthread_mutex_lock(&r->sam.sc_mu);
    r->sam.sc_stop = 1;
    pthread_cond_broadcast(&r->sam.sc_cv);
    pthread_mutex_unlock(&r->sam.sc_mu);
    pthread_join(r->sam.sc_thread, NULL);
    for (int k = 0; k < 2; k++)
        if (r->sam.sc[k].begun) {
            itx_samtext_result res;
            (void)r->sam.sdev.parse_end(r->sam.sdev.obj, k, &res);
            r->sam.sc[k].begun = 0;
        }
}

static void *sam_chunk_thread(void *arg)
{
    aln_reader *r = arg;
    for (;;) {
        if (!sam_slot_wait(r)) break;
        const int k = (int)(r->sam.sc_fill & 1);
        struct sam_chunk *c = &r->sam.sc[k];
        size_t have = r->sam.sc_tail_len, cut = 0, seen = 0;
        int eof = 0;
        sam_buf_need(r, c, have + r->sam.sc_chunk + 1, 0);
        if (have) memcpy(c->buf, r->sam.sc_tail, have);
        r->sam.sc_tail_len = 0;
        for (;;) {
            /* up to a chunk in all; a line longer than that grows the buffer a chunk at a time */
            const size_t want = have < r->sam.sc_chunk ? r->sam.sc_chunk - have : r->sam.sc_chunk;
            sam_buf_need(r, c, have + want + 1, have);
            const double t0 = now_s();
            const size_t got = fread(c->buf + have, 1, want, r->cm.f);
            t_io += now_s() - t0;
            have += got;
            if (got < want) eof = 1;
            if (eof) {
                cut = have;
                break;
            }
            const uint8_t *nl = memrchr(c->buf + seen, '\n', have - seen);
            if (nl) {
                cut = (size_t)(nl - c->buf) + 1;
                break;
            }
            seen = have;
        }
        if (have > cut) {
            if (r->sam.sc_tail_cap < have - cut) {
                r->sam.sc_tail_cap = (have - cut) + (have - cut) / 4 + 256;
                r->sam.sc_tail = xrealloc(r->sam.sc_tail, r->sam.sc_tail_cap);
            }
            memcpy(r->sam.sc_tail, c->buf + cut, have - cut);
            r->sam.sc_tail_len = have - cut;
        }
        c->len = cut;
        c->final = eof;
        c->begun = 0;
        c->begin_rc = 0;
        c->bgzf = c->handover = 0;
        if (r->sam.sz_gz && cut) r->sam.sz_host_chunks++;                        /* inflated by gzread behind r->cm.f */
        if (r->sam.sdev_on && cut) {
            c->begin_rc = r->sam.sdev.parse_begin(r->sam.sdev.obj, k, c->buf, cut, eof);
            c->begun = c->begin_rc == 0;
        }
        sam_slot_filled(r);
        if (eof) break;
    }
    return NULL;
}

/* BGZF for the device to inflate: whole members, read from the file's own descriptor, until they inflate to a chunk (the last one
 * may take it up to 64 KiB - 1 further); the chunk's parse is begun here, so that it runs while the chunk before is consumed. Ends
 * with the chunk behind which the file ends, or with a chunk the decoder cannot take: what lies at its first byte is not a BGZF
 * member, or the file ends inside it (sam_hand_over). */
static void *sam_bgzf_thread(void *arg)
{
    aln_reader *r = arg;
    const size_t step = r->sam.sc_chunk / 2 < 65536 ? 65536 : r->sam.sc_chunk / 2 > ((size_t)4 << 20) ? (size_t)4 << 20 : r->sam.sc_chunk / 2;
    for (;;) {
        if (!sam_slot_wait(r)) break;
        const int k = (int)(r->sam.sc_fill & 1);
        struct sam_chunk *c = &r->sam.sc[k];
        c->bgzf = 1;
        c->handover = c->begun = c->begin_rc = c->final = 0;
        c->len = 0;
        c->coff = r->sam.sz_off;
        c->skip_before = r->sam.sz_skip;
        c->why[0] = 0;
        size_t have = 0, off = 0, utot = 0, nb = 0;
        int damaged = 0, capped = 0, at_end = 0;
        for (;;) {                                                   /* more bytes until a chunk's worth of whole members is at hand */
            sam_room(r, &c->cbuf, &c->ccap, &c->c_from_alloc, have + step + 64, have);
            const double t0 = now_s();
            ssize_t got = pread(r->sam.sam_fd, c->cbuf + have, step, (off_t)(r->sam.sz_off + have));
            t_io += now_s() - t0;
            if (got < 0) got = 0;                                    /* a read error ends the file, as it does for gzread */
            have += (size_t)got;
            at_end = (size_t)got < step;
            nb = index_blocks(c->cbuf, have, &c->bl, &c->bl_cap, SIZE_MAX, r->sam.sc_chunk + BGZF_MAX - 1, &off, &utot, &damaged, &capped);
            if (capped || damaged || at_end) break;
        }
        for (size_t i = 0; i < nb; i++)                              /* the chunk ends with the member that takes the sum to a chunk */
            if (c->bl[i].uoff + c->bl[i].usize >= r->sam.sc_chunk) {
                nb = i + 1;
                off = c->bl[i].coff + c->bl[i].csize;
                utot = c->bl[i].uoff + c->bl[i].usize;
                break;
            }
        int last = 0;
        if (nb == 0) {
            c->handover = last = 1;
            snprintf(c->why, sizeof c->why, damaged ? "what lies there is not a BGZF member" : "the file ends inside that member");
        } else {
            if (c->zb_cap < nb) {
                c->zb_cap = nb + nb / 4 + 64;
                c->zb = xrealloc(c->zb, sizeof *c->zb * c->zb_cap);
            }
            for (size_t i = 0; i < nb; i++)
                c->zb[i] = (itx_bgzf_block){(uint32_t)c->bl[i].coff, (uint32_t)c->bl[i].csize, (uint32_t)c->bl[i].uoff, (uint32_t)c->bl[i].usize};
            const size_t skip = r->sam.sz_skip < utot ? r->sam.sz_skip : utot;
            r->sam.sz_skip -= skip;
            c->clen = off;
            c->utot = utot;
            c->final = at_end && off == have && !damaged;            /* the file ends behind the chunk's last member */
            c->begin_rc = r->sam.sdev.parse_begin_bgzf(r->sam.sdev.obj, k, c->cbuf, off, c->zb, nb, skip, c->final);
            if (c->begin_rc == 0) {
                c->begun = 1;
                r->sam.sz_off += off;
                last = c->final;
            } else {                                                 /* (a text that does not fit the object, for one) */
                c->handover = last = 1;
                c->final = 0;
                snprintf(c->why, sizeof c->why, "%s", r->sam.sdev.last_error ? r->sam.sdev.last_error() : "the device declined the chunk");
            }
        }
        sam_slot_filled(r);
        if (last) break;
    }
    return NULL;
}

/* whether the device inflates this file, and if not, who does and why (ITX_TIMING) */
static int sam_device_inflates(aln_reader *r)
{
    const char *e = getenv("ITX_HOST_SAM_INFLATE");
    struct stat sb;
    const char *why = NULL;
    if (!r->sam.sz_gz) return 0;
    if (!r->sam.sdev_on) why = "no device object attached";
    else if (e && atoi(e) == 1) why = "ITX_HOST_SAM_INFLATE=1";
    else if (!r->sam.sz_bgzf) why = "plain gzip is one stream";
    else if (!r->sam.sdev.parse_begin_bgzf || !r->sam.sdev.bgzf_info || !r->sam.sdev.text || !r->sam.sdev.strings) why = "the device object has no BGZF entries";
    else if (r->sam.sam_fd < 0 || fstat(r->sam.sam_fd, &sb) != 0 || !S_ISREG(sb.st_mode)) why = "not a regular file";
    if (why) snprintf(r->sam.sz_reason, sizeof r->sam.sz_reason, "%s", why);
    return why == NULL;
}

static void sam_chunks_start(aln_reader *r)
{
    r->sam.sc_on = 1;
    r->sam.sc_chunk = aln_sam_chunk_bytes();
    r->sam.sz_on = sam_device_inflates(r);
    if (r->sam.sz_on) {
        /* the device's stream starts again at the file's first byte and skips the header; the first body line, which the header
         * scan has read already, is in that stream too */
        if (r->sam.pending_len >= 0) r->sam.n_lines--;
        r->sam.pending_len = -1;
        r->sam.sz_off = 0;
        r->sam.sz_skip = r->sam.sz_hdr;
    } else if (r->sam.pending_len >= 0) {                                       /* the first body line goes in front of the first chunk */
        r->sam.sc_tail_cap = (size_t)r->sam.pending_len + 256;
        r->sam.sc_tail = xmalloc(r->sam.sc_tail_cap);
        memcpy(r->sam.sc_tail, r->sam.line, (size_t)r->sam.pending_len);
        r->sam.sc_tail_len = (size_t)r->sam.pending_len;
        r->sam.pending_len = -1;
        r->sam.n_lines--;                                                /* counted again when its chunk is taken */
    }
    pthread_mutex_init(&r->sam.sc_mu, NULL);
    pthread_cond_init(&r->sam.sc_cv, NULL);
    if (pthread_create(&r->sam.sc_thread, NULL, r->sam.sz_on ? sam_bgzf_thread : sam_chunk_thread, r) != 0) die("cannot start the SAM read-ahead thread");
}

static void __attribute__((format(printf, 2, 3))) sam_host_reason(aln_reader *r, const char *fmt, ...)
{
    if (r->sam.st_host_chunks++ || !fmt) return;                         /* the reason of the first one is reported */
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r->sam.st_reason, sizeof r->sam.st_reason, fmt, ap);
    va_end(ap);
}

static void sam_chunk_close(aln_reader *r)
{
    if (r->sam.sc[r->sam.sc_take & 1].final) r->sam.sc_done = 1;
    r->sam.sc_open = 0;
    pthread_mutex_lock(&r->sam.sc_mu);
    r->sam.sc_take++;
    pthread_cond_broadcast(&r->sam.sc_cv);
    pthread_mutex_unlock(&r->sam.sc_mu);
}

/* The decoder cannot take chunk c whole: nothing of it is used. The host's zlib reader takes the file from the chunk's first member
 * on, with the carry (bytes [at, at + len) of the text in `slot`: the tail of the last chunk that was used) in front; what it
 * makes of odd and damaged input is then the reference's, whose reader it is. For the rest of the file. */
static void sam_hand_over(aln_reader *r, struct sam_chunk *c, int slot, size_t at, size_t len)
{
    sam_thread_stop(r);
    if (r->sam.sc_tail_cap < len + 1) {
        r->sam.sc_tail_cap = len + len / 4 + 256;
        r->sam.sc_tail = xrealloc(r->sam.sc_tail, r->sam.sc_tail_cap);
    }
    if (len) SDEV_CHK(r->sam.sdev.text(r->sam.sdev.obj, slot, at, r->sam.sc_tail, len), "the carry could not be fetched: ");
    r->sam.sc_tail_len = len;
    if (!r->sam.sz_reason[0]) snprintf(r->sam.sz_reason, sizeof r->sam.sz_reason, "handed over at byte %zu of the file: %s", c->coff, c->why);
    if (r->cm.f) fclose(r->cm.f);
    const int fd = dup(r->sam.sam_fd);
    if (fd < 0 || lseek(fd, (off_t)c->coff, SEEK_SET) < 0 || !(r->cm.f = samz_fopen(gzdopen(fd, "rb")))) die("SAM input: cannot read on from byte %zu", c->coff);
    for (size_t left = c->skip_before; left;) {                      /* what is left of the header */
        uint8_t junk[4096];
        const size_t got = fread(junk, 1, left < sizeof junk ? left : sizeof junk, r->cm.f);
        if (!got) break;
        left -= got;
    }
    r->sam.sz_on = 0;
    r->sam.sz_prev_slot = -1;
    r->sam.sc[0].bgzf = r->sam.sc[1].bgzf = r->sam.sc[0].handover = r->sam.sc[1].handover = 0;
    r->sam.sc_stop = r->sam.sc_open = 0;
    r->sam.sc_fill = r->sam.sc_take = 0;
    if (pthread_create(&r->sam.sc_thread, NULL, sam_chunk_thread, r) != 0) die("cannot start the SAM read-ahead thread");
}

/* the device has parsed the open chunk whole (n_hard == 0): its records are handed out from the device's arrays */
static void sam_take_result(aln_reader *r, const itx_samtext_result *res)
{
    r->sam.sc_host = 0;
    r->sam.sc_nrec = res->n_rec;
    r->sam.sc_next = 0;
    r->sam.sc_lines = res->n_lines;
    r->sam.sc_flags = res->flags;
    r->sam.st_dev_chunks++;
    r->sam.st_dev_bytes += res->consumed;
    r->sam.st_ms += res->kernel_ms;
}

/* a chunk the device has inflated becomes the one being consumed. 1: it is open; 0: it held nothing, or the file was handed over:
 * the caller looks for the next chunk */
static int sam_bgzf_open(aln_reader *r, int k, struct sam_chunk *c)
{
    if (c->handover) {                                               /* nothing begun: the carry lies where the chunk before left it */
        sam_hand_over(r, c, r->sam.sz_prev_slot, r->sam.sz_prev_at, r->sam.sz_prev_slot >= 0 ? r->sam.sz_prev_tail : 0);
        return 0;
    }
    itx_samtext_result res;
    itx_samtext_bgzf_info_t zi;
    const double t0 = now_s();
    SDEV_CHK(r->sam.sdev.parse_end(r->sam.sdev.obj, k, &res), "parse failed: ");
    r->sam.st_wait += now_s() - t0;
    c->begun = 0;
    SDEV_CHK(r->sam.sdev.bgzf_info(r->sam.sdev.obj, k, &zi), "");
    if (zi.n_bad) {                                                  /* its text begins with the carry, whatever the members gave */
        snprintf(c->why, sizeof c->why, "member %llu from there on does not inflate on the device", (unsigned long long)zi.first_bad);
        sam_hand_over(r, c, k, 0, (size_t)zi.carry_len);
        return 0;
    }
    if (res.consumed + zi.tail_len != zi.text_len || (c->final && zi.tail_len))
        die("SAM text on the device: %llu of %llu bytes consumed", (unsigned long long)res.consumed, (unsigned long long)zi.text_len);
    r->sam.sz_prev_slot = k;
    r->sam.sz_prev_at = (size_t)res.consumed;
    r->sam.sz_prev_tail = (size_t)zi.tail_len;
    r->sam.sz_dev_chunks++;
    r->sam.sz_comp_bytes += c->clen;
    r->sam.sz_infl_bytes += c->utot;
    r->sam.sz_inflate_ms += zi.inflate_ms;
    if (res.n_hard == 0) {
        sam_take_result(r, &res);
    } else {                                                         /* the host takes the consumed text line by line: it fetches it */
        sam_host_reason(r, "line %lld is spelt in a way the device does not model", r->sam.n_lines + (long long)res.first_hard_line + 1);
        sam_buf_need(r, c, (size_t)res.consumed + 1, 0);
        if (res.consumed) SDEV_CHK(r->sam.sdev.text(r->sam.sdev.obj, k, 0, c->buf, (size_t)res.consumed), "the text could not be fetched: ");
        c->len = (size_t)res.consumed;
    }
    if (r->sam.sc_host ? c->len == 0 : res.n_rec == 0) {                 /* (a chunk inside the header, a chunk that ends before its first newline) */
        sam_chunk_close(r);
        return 0;
    }
    return 1;
}

/* the next chunk becomes the one being consumed: 0 at the end of the input */
static int sam_chunk_open(aln_reader *r)
{
    for (;;) {
        if (r->sam.sc_done) return 0;
        pthread_mutex_lock(&r->sam.sc_mu);
        while (r->sam.sc_fill == r->sam.sc_take) pthread_cond_wait(&r->sam.sc_cv, &r->sam.sc_mu);
        pthread_mutex_unlock(&r->sam.sc_mu);
        const int k = (int)(r->sam.sc_take & 1);
        struct sam_chunk *c = &r->sam.sc[k];
        r->sam.sc_open = 1;
        r->sam.sc_host = 1;
        r->sam.sc_pos = 0;
        if (c->bgzf) {
            if (sam_bgzf_open(r, k, c)) return 1;
            continue;
        }
        if (c->len == 0) {                                           /* nothing but the end of the file */
            sam_chunk_close(r);
            continue;
        }
        if (c->begun) {
            itx_samtext_result res;
            const double t0 = now_s();
            SDEV_CHK(r->sam.sdev.parse_end(r->sam.sdev.obj, k, &res), "parse failed: ");
            r->sam.st_wait += now_s() - t0;
            c->begun = 0;
            if (res.n_hard == 0) {
                if (res.consumed != c->len) die("SAM text on the device: %llu of %zu bytes consumed", (unsigned long long)res.consumed, c->len);
                sam_take_result(r, &res);
                if (res.n_rec == 0) {
                    sam_chunk_close(r);
                    continue;
                }
            } else {
                sam_host_reason(r, "line %lld is spelt in a way the device does not model", r->sam.n_lines + (long long)res.first_hard_line + 1);
            }
        } else if (!r->sam.sdev_on) {
            sam_host_reason(r, "no device object attached");
        } else {
            sam_host_reason(r, "a chunk of %zu bytes, more than the device object holds", c->len);
        }
        return 1;
    }
}

static size_t sam_read_chunked(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa)
{
    size_t n = 0;
    while (n < cap) {
        if (!r->sam.sc_open && !sam_chunk_open(r)) break;
        const int k = (int)(r->sam.sc_take & 1);
        struct sam_chunk *c = &r->sam.sc[k];
        if (r->sam.sc_host) {
            while (n < cap && r->sam.sc_pos < c->len) {
                uint8_t *s = c->buf + r->sam.sc_pos;
                const uint8_t *nl = memchr(s, '\n', c->len - r->sam.sc_pos);
                const size_t ll = nl ? (size_t)(nl - s) : c->len - r->sam.sc_pos;
                r->sam.sc_pos += ll + (nl ? 1 : 0);
                r->sam.n_lines++;
                s[ll] = 0;                                           /* the newline, or the spare byte behind the last line */
                if (sam_take_line(r, (char *)s, (ssize_t)ll, st, &n, side, any_paired, aux_xa) == 2) {
                    if (r->sam.sc_pos >= c->len) sam_chunk_close(r);
                    return n;
                }
            }
            if (r->sam.sc_pos >= c->len) sam_chunk_close(r);
            continue;
        }
        size_t m = (size_t)(r->sam.sc_nrec - r->sam.sc_next);
        if (m > cap - n) m = cap - n;
        const int want_q = side && side->want_qnames, want_a = side && side->want_aux, has_xa = (r->sam.sc_flags & ITX_SAMTEXT_XA) != 0;
        if (r->sam.s_cap < m) {
            r->sam.s_cap = m + m / 4 + 64;
            r->sam.s_off = xrealloc(r->sam.s_off, 4 * r->sam.s_cap);
            r->sam.s_qlen = xrealloc(r->sam.s_qlen, 4 * r->sam.s_cap);
            r->sam.s_xoff = xrealloc(r->sam.s_xoff, 4 * r->sam.s_cap);
            r->sam.s_xlen = xrealloc(r->sam.s_xlen, 4 * r->sam.s_cap);
            r->sam.s_nm = xrealloc(r->sam.s_nm, 4 * r->sam.s_cap);
            r->sam.s_mark = xrealloc(r->sam.s_mark, r->sam.s_cap);
        }
        const int aux = want_a && has_xa;
        const double tp = now_s();
        const int on_dev = c->bgzf;                                  /* the text lies on the device only: the strings are gathered there */
        SDEV_CHK(r->sam.sdev.fetch(r->sam.sdev.obj, k, (size_t)r->sam.sc_next, m, st, n, want_q && !on_dev ? r->sam.s_off : NULL, want_q ? r->sam.s_qlen : NULL,
                                   aux && !on_dev ? r->sam.s_xoff : NULL, aux ? r->sam.s_xlen : NULL, aux ? r->sam.s_nm : NULL, has_xa ? r->sam.s_mark : NULL),
                 "fetch failed: ");
        itx_samtext_strings_out so;
        memset(&so, 0, sizeof so);
        if (on_dev && (want_q || aux)) {
            SDEV_CHK(r->sam.sdev.strings(r->sam.sdev.obj, k, (size_t)r->sam.sc_next, m, (want_q ? 1 : 0) | (aux ? 2 : 0), &so), "the strings could not be gathered: ");
            r->sam.sz_gather_ms += so.kernel_ms;
        }
        int ap = 0, xa = 0;
        const uint8_t *f5 = st->flag5 + n;
        for (size_t i = 0; i < m; i++) ap |= f5[i] & 1;
        if (has_xa)
            for (size_t i = 0; i < m; i++) xa |= r->sam.s_mark[i];
        if (ap) *any_paired = 1;
        if (xa) *aux_xa = 1;
        if (want_q || want_a) {
            const char *text = on_dev ? so.text : (const char *)c->buf;
            const uint32_t *q_at = on_dev ? so.qname_at : r->sam.s_off, *x_at = on_dev ? so.xa_at : r->sam.s_xoff;
#pragma omp parallel for schedule(static)
            for (long i = 0; i < (long)m; i++) {
                if (want_q) side->qname[n + (size_t)i] = xstrndup_bound(text + q_at[i], r->sam.s_qlen[i]);
                if (want_a) {
                    side->xa[n + (size_t)i] = NULL;
                    side->nm[n + (size_t)i] = 0;
                    if (aux && r->sam.s_mark[i]) {
                        side->xa[n + (size_t)i] = xstrndup_bound(text + x_at[i], r->sam.s_xlen[i]);
                        side->nm[n + (size_t)i] = r->sam.s_nm[i];
                    }
                }
            }
        }
        t_parse += now_s() - tp;
        r->sam.sc_next += m;
        n += m;
        if (r->sam.sc_next == r->sam.sc_nrec) {
            r->sam.n_lines += (long long)r->sam.sc_lines;
            sam_chunk_close(r);
        }
    }
    return n;
}


/* stops the chunk reader, prints the SAM timing lines, frees what the SAM side holds */
void sam_close(aln_reader *r)
{
    if (!r->cm.is_sam) return;
    if (r->sam.sc_on) {
        sam_thread_stop(r);
        for (int k = 0; k < 2; k++) {
            struct sam_chunk *c = &r->sam.sc[k];
            sam_buf_release(r, c->buf, c->from_alloc);
            sam_buf_release(r, c->cbuf, c->c_from_alloc);
            free(c->bl);
            free(c->zb);
        }
        if (getenv("ITX_TIMING"))
            fprintf(stderr, "[itx timing] sam: %llu chunks parsed on the device (%llu bytes, %.3f ms in its kernels, host waited %.3f s), %llu by the host (%s)\n", r->sam.st_dev_chunks,
                    r->sam.st_dev_bytes, r->sam.st_ms, r->sam.st_wait, r->sam.st_host_chunks, r->sam.st_host_chunks ? r->sam.st_reason : "none");
        free(r->sam.sc_tail);
        free(r->sam.s_off);
        free(r->sam.s_qlen);
        free(r->sam.s_xoff);
        free(r->sam.s_xlen);
        free(r->sam.s_nm);
        free(r->sam.s_mark);
        pthread_mutex_destroy(&r->sam.sc_mu);
        pthread_cond_destroy(&r->sam.sc_cv);
    }
    if (getenv("ITX_TIMING")) {
        if (!r->sam.sz_gz)
            fprintf(stderr, "[itx timing] sam gz: not compressed\n");
        else
            fprintf(stderr, "[itx timing] sam gz: %llu chunks inflated on the device (%llu -> %llu bytes, %.3f ms in the decoder, %.3f ms gathering strings), %llu by the host (%s)\n",
                    r->sam.sz_dev_chunks, r->sam.sz_comp_bytes, r->sam.sz_infl_bytes, r->sam.sz_inflate_ms, r->sam.sz_gather_ms, r->sam.sz_host_chunks,
                    r->sam.sz_reason[0] ? r->sam.sz_reason : r->sam.sc_on ? "none" : "read line by line");
    }
    if (r->sam.sam_fd >= 0) close(r->sam.sam_fd);
    free(r->sam.line);
}

size_t sam_read_batch(aln_reader *r, itx_staging *st, size_t cap, aln_side *side, int *any_paired, int *aux_xa)
{
    if (side) side->has_strings = 1;
    if (!r->sam.sc_on && (r->sam.sdev_on || getenv("ITX_SAM_CHUNK"))) sam_chunks_start(r);
    if (r->sam.sc_on) return sam_read_chunked(r, st, cap, side, any_paired, aux_xa);
    size_t n = 0;
    while (n < cap) {
        ssize_t len;
        if (r->sam.pending_len >= 0) {
            len = r->sam.pending_len;
            r->sam.pending_len = -1;
        } else {
            len = getline(&r->sam.line, &r->sam.line_cap, r->cm.f);
            if (len < 0) break;
            r->sam.n_lines++;
        }
        if (sam_take_line(r, r->sam.line, len, st, &n, side, any_paired, aux_xa) == 2) break;
    }
    return n;
}
