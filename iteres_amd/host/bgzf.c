/* bgzf.c — what a BGZF member looks like, and nothing that knows a reader: the member's frame, its inflation, the index of
 * the members in a run of bytes, a plain sequential reader for small amounts of data, and on top of that the search for the
 * point where a share of a BAM file may begin. Block framing follows samtools 0.1.18 as vendored by the reference
 * (bgzf.c:401-411,471-565). */
#define _GNU_SOURCE
#define ALN_PRIV_NO_READER
#include "aln_priv.h"

#include <dlfcn.h>
#include <unistd.h>
#include <zlib.h>

/* bgzf.c:401-411 check_header: gzip member with exactly one 6-byte extra field "BC" */
int bgzf_header_ok(const uint8_t *h)
{
    return h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4) && (h[10] | h[11] << 8) == 6 && h[12] == 'B' && h[13] == 'C' &&
           (h[14] | h[15] << 8) == 2;
}

/* the header part of the frame: the bytes the member at h[0, 18) takes (BSIZE + 1), 0 when that is no member's header */
size_t bgzf_member_size(const uint8_t *h)
{
    if (!bgzf_header_ok(h)) return 0;
    const size_t bsize = (size_t)(h[16] | h[17] << 8) + 1;
    return bsize < 26 ? 0 : bsize;
}

/* The member at the front of p[0, n) (bgzf.c:401-411 header check, BSIZE, the ISIZE trailer): 1 it is complete, *csize bytes
 * that inflate to *usize; 0 incomplete: only more bytes can tell; -1 not a member, or damaged. */
int bgzf_member(const uint8_t *p, size_t n, size_t *csize, size_t *usize)
{
    if (n < 18) return 0;
    const size_t bsize = bgzf_member_size(p);
    if (!bsize) return -1;
    if (bsize > n) return 0;
    const size_t us = rd_u32(p + bsize - 4);
    if (us > BGZF_MAX) return -1;
    *csize = bsize;
    *usize = us;
    return 1;
}

/* The frame from the writing side (filter -b: the header of the emitted BAM; the records' members are made on the device by
 * the same frame, csrc/itx_bgzfmember.h): 18 bytes bgzf_header_ok accepts with BSIZE = size - 1, raw DEFLATE, CRC-32, ISIZE.
 * At most 0xff00 bytes go into a member, as samtools cuts them, so that a member fits 64 KiB whatever zlib makes of it. */
int bgzf_write_members(FILE *f, const uint8_t *bytes, size_t len)
{
    enum { CHUNK = 0xff00 };
    uint8_t out[18 + CHUNK + 1024 + 8];
    for (size_t at = 0; at < len; at += CHUNK) {
        const size_t n = len - at < CHUNK ? len - at : CHUNK;
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return -1;
        zs.next_in = (Bytef *)(bytes + at);
        zs.avail_in = (uInt)n;
        zs.next_out = out + 18;
        zs.avail_out = CHUNK + 1024;
        const int rc = deflate(&zs, Z_FINISH);
        const size_t z = zs.total_out;
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) return -1;
        const size_t size = 18 + z + 8;
        const uLong crc = crc32(crc32(0L, NULL, 0), bytes + at, (uInt)n);
        static const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
        memcpy(out, head, 16);
        out[16] = (uint8_t)(size - 1);
        out[17] = (uint8_t)((size - 1) >> 8);
        for (int i = 0; i < 4; i++) {
            out[18 + z + i] = (uint8_t)(crc >> (8 * i));
            out[22 + z + i] = (uint8_t)(n >> (8 * i));
        }
        if (size - 1 > 0xffff || fwrite(out, 1, size, f) != size) return -1;
    }
    return 0;
}

/* the empty member every BAM ends with (bgzf.c of samtools: 28 bytes) */
int bgzf_write_eof(FILE *f)
{
    static const uint8_t eof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return fwrite(eof, 1, sizeof eof, f) == sizeof eof ? 0 : -1;
}

/* Raw DEFLATE of one block. libdeflate, when the system has it (dlopen, no build-time dependency), inflates two to three
 * times faster than zlib's inflate(); both are lossless decoders of the same stream, so the bytes are the same.
 * ITX_NO_LIBDEFLATE=1 keeps zlib. */
typedef struct libdeflate_decompressor ld_dec;
static ld_dec *(*ld_alloc)(void);
static int (*ld_inflate)(ld_dec *, const void *, size_t, void *, size_t, size_t *);
static int ld_state;                         /* 0 not probed, 1 in use, -1 unavailable */
void ld_probe(void)
{
    if (ld_state) return;
    ld_state = -1;
    if (getenv("ITX_NO_LIBDEFLATE")) return;
    void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    ld_alloc = (ld_dec * (*)(void)) dlsym(h, "libdeflate_alloc_decompressor");
    ld_inflate = (int (*)(ld_dec *, const void *, size_t, void *, size_t, size_t *))dlsym(h, "libdeflate_deflate_decompress");
    if (ld_alloc && ld_inflate) ld_state = 1;
}

int inflate_block(const uint8_t *src, size_t csize, uint8_t *dst, size_t usize)
{
    if (ld_state == 1) {
        static __thread ld_dec *d;
        if (!d) d = ld_alloc();
        size_t got = 0;
        if (d && ld_inflate(d, src + 18, csize - 18 - 8, dst, usize, &got) == 0 && got == usize) return 0;
        /* anything unexpected: let zlib have the last word */
    }
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    zs.next_in = (Bytef *)(src + 18);
    zs.avail_in = (uInt)(csize - 18 - 8);
    zs.next_out = dst;
    zs.avail_out = (uInt)usize;
    if (inflateInit2(&zs, -15) != Z_OK) return -1;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    return (rc == Z_STREAM_END && zs.total_out == usize) ? 0 : -1;
}

const char *inflater_name(void) { return ld_state == 1 ? "libdeflate" : "zlib"; }

/* The complete BGZF blocks of the raw bytes at hand, buf[0, len), into *blk (grown as needed);
 * *poff = compressed bytes they take, *putot = bytes they inflate to. At most max_blocks blocks / max_utot inflated bytes
 * are taken (*pcapped: more complete blocks may follow in what is at hand). */
size_t index_blocks(const uint8_t *buf, size_t len, struct blk **blk, size_t *blk_cap, size_t max_blocks, size_t max_utot, size_t *poff,
                    size_t *putot, int *pdamaged, int *pcapped)
{
    *pcapped = 0;
    struct blk *bl = *blk;
    size_t nb = 0, off = 0, utot = 0, bsize = 0, usize = 0;
    *pdamaged = 0;
    for (;;) {
        const int st = bgzf_member(buf + off, len - off, &bsize, &usize);
        if (st == 0) break;                                     /* incomplete: wait for more input */
        if (st < 0) {
            *pdamaged = 1;
            break;
        }
        if (nb == max_blocks || utot + usize > max_utot) {      /* enough for one go: the rest stays for the next */
            *pcapped = 1;
            break;
        }
        if (nb == *blk_cap) {
            *blk_cap = *blk_cap ? *blk_cap * 2 : 4096;
            bl = *blk = xrealloc(bl, sizeof *bl * *blk_cap);
        }
        bl[nb++] = (struct blk){off, bsize, utot, usize};
        utot += usize;
        off += bsize;
    }
    *poff = off;
    *putot = utot;
    return nb;
}

/* ---- a plain sequential BGZF reader on the host (pread + one block at a time): the header of a file whose records this
 * reader takes only a share of, and the search for the share's boundaries. Small amounts of data: no threads. */

/* inflates the next block behind u[len): 0 done, 1 end of file (or a block cut short by it), -1 not a block / damaged */
static int hz_block(hz_t *z)
{
    uint8_t h[18];
    if (z->off + 18 > z->size) return 1;
    if (pread(z->fd, h, 18, (off_t)z->off) != 18) return -1;
    const size_t bsize = bgzf_member_size(h);
    if (!bsize) return -1;
    if (z->off + bsize > z->size) return 1;
    uint8_t *c = xmalloc(bsize + 16);
    size_t csize = 0, usize = 0;                               /* csize: bsize again */
    if (pread(z->fd, c, bsize, (off_t)z->off) != (ssize_t)bsize || bgzf_member(c, bsize, &csize, &usize) != 1) {
        free(c);
        return -1;
    }
    if (z->len + usize + 64 > z->cap) {
        z->cap = (z->len + usize) * 2 + BGZF_MAX;
        z->u = xrealloc(z->u, z->cap);
    }
    if (usize && inflate_block(c, bsize, z->u + z->len, usize) != 0) {
        free(c);
        return -1;
    }
    free(c);
    if (z->nb == z->bcap) {
        z->bcap = z->bcap ? z->bcap * 2 : 64;
        z->b = xrealloc(z->b, sizeof *z->b * z->bcap);
    }
    z->b[z->nb++] = (struct blk){z->off, bsize, z->len, usize};
    z->len += usize;
    z->off += bsize;
    return 0;
}

size_t hz_read(hz_t *z, void *dst, size_t n)
{
    while (z->len - z->pos < n)
        if (hz_block(z) != 0) break;
    size_t k = z->len - z->pos;
    if (k > n) k = n;
    if (k) memcpy(dst, z->u + z->pos, k);
    z->pos += k;
    return k;
}

void hz_free(hz_t *z)
{
    free(z->u);
    free(z->b);
    memset(z, 0, sizeof *z);
}

/* Where a share of the file may begin: a point at or after compressed byte `at` where a BAM record starts, as (file offset
 * of a BGZF block, inflated bytes into that block — fewer than the block holds, size of that block). Two ranks that
 * call this with the same arguments get the same point, which is all that the split needs: any true record start will do.
 * It is a GUESS (a block header whose BSIZE chain leads to more headers; 8 well-formed records in a row): the rank whose
 * share ENDS there verifies it — its own chain of records, which starts at a known record start, has to arrive exactly
 * there — and the job falls back to one rank when a boundary does not hold.
 * Returns 1 with the point; 0 when the file ends without one (nothing starts behind `at`: the share before runs to the
 * end); -1 when the search had to be given up (no block header within reach, damaged blocks, or the chain of a candidate
 * still undecided after GIVE_UP inflated bytes — records of megabytes): the caller must not trust ANY share then. A chain
 * that runs out of inflated bytes is never a reason to reject a candidate: more blocks are inflated until it is decided
 * (with a fixed margin instead, true starts were rejected once eight records no longer fit into it — long reads — and a
 * boundary that fails on one side while a later one holds made two ranks count the same records). */
int find_split(int fd, size_t fsize, size_t at, int n_targets, size_t *pB, size_t *pc, size_t *pcsize)
{
    if (at >= fsize) return 0;
    const size_t span = fsize - at < (4u << 16) + 64 ? fsize - at : (4u << 16) + 64;
    uint8_t *buf = xmalloc(span + 32);
    memset(buf, 0, span + 32);
    size_t have = 0;
    while (have < span) {
        const ssize_t k = pread(fd, buf + have, span - have, (off_t)(at + have));
        if (k <= 0) break;
        have += (size_t)k;
    }
    size_t B = SIZE_MAX;
    for (size_t p = 0; p + 18 <= have && p <= (1u << 16); p++) {
        if (!bgzf_header_ok(buf + p)) continue;
        size_t q = p;
        int ok = 1;
        for (int k = 0; k < 3; k++) {
            if (at + q == fsize) break;                              /* the chain ends with the file */
            const size_t bsize = q + 18 <= have ? bgzf_member_size(buf + q) : 0;
            if (!bsize || at + q + bsize > fsize) {
                ok = 0;
                break;
            }
            q += bsize;
        }
        if (ok) {
            B = at + p;
            break;
        }
    }
    free(buf);
    if (B == SIZE_MAX) return at + have >= fsize && have <= (1u << 16) ? 0 : -1;     /* the last bytes of a file hold no block start: fine; no header in 64 KiB: not a BGZF file here */
    enum { K = 8, GIVE_UP = 64u << 20 };
    hz_t z;
    memset(&z, 0, sizeof z);
    z.fd = fd;
    z.off = B;
    z.size = fsize;
    size_t c = 0, found = SIZE_MAX;
    int at_end = 0, gave_up = 0;
    while (found == SIZE_MAX) {
        if (!at_end) {
            int st = 0;
            for (int i = 0; i < 4 && st == 0; i++) st = hz_block(&z);
            if (st < 0) {                                            /* a damaged block: nothing behind it can be vouched for */
                gave_up = 1;
                break;
            }
            at_end = st != 0;
        }
        int undecided = 0;
        for (; c < z.len && found == SIZE_MAX; c++) {
            size_t a = c;
            int k = 0, why = 1;
            while (k < K) {
                size_t step = 0;
                why = record_or_short(z.u, a, z.len, n_targets, &step);
                if (why != 1) break;
                a += step;
                k++;
            }
            if (k == K || (k > 0 && at_end && a == z.len)) {
                found = c;
            } else if (why < 0 && !at_end) {
                undecided = 1;                                       /* this candidate needs more bytes: come back to it */
                break;
            }
        }
        if (found != SIZE_MAX) break;
        if (at_end) break;                                           /* every byte looked at: no record starts here */
        if (undecided && z.len > GIVE_UP) {
            gave_up = 1;
            break;
        }
    }
    int ok = gave_up ? -1 : 0;
    if (found != SIZE_MAX) {
        /* as (block, offset inside it): the block that holds that byte */
        for (size_t i = 0; i < z.nb; i++)
            if (z.b[i].usize && found >= z.b[i].uoff && found < z.b[i].uoff + z.b[i].usize) {
                *pB = z.b[i].coff;
                *pc = found - z.b[i].uoff;
                *pcsize = z.b[i].csize;
                ok = 1;
                break;
            }
    }
    hz_free(&z);
    return ok;
}
