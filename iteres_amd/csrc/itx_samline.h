/* itx_samline.h — one line of SAM text turned into one record of the engine's arrays: the rule of `iteres stat|filter -S`
 * (bam_import.c:237-470 of samtools 0.1.18 as far as the record loop reads the result), stated once for the device
 * (csrc/itx_samtext.hip, over LDS and over global memory) and for the host build the tests hold against the host reader's own
 * parser, host/samio.c sam_take_line (tests/samline_host.cpp). Valid C and C++.
 *
 * The function models only the PLAIN spelling of every field; whatever else the host parser accepts — through strtol's
 * prefixes, signs and blanks, the flag letters of samtools 0.1.x, a warning or an abort it prints — is called HARD and the
 * host has to look: the values of a hard line are not to be used.
 *
 *   FLAG     plain `0` or [1-9][0-9]{0,8}                      hard: empty, a leading 0 with more behind it, anything but digits, > 9 digits
 *   RNAME    `*` -> -1, else the caller's lookup               hard: the lookup does not know the name (warning / abort of sam_read1)
 *   POS, MAPQ, PNEXT   first byte a digit -> the leading run of digits (POS, PNEXT minus 1; MAPQ cut to 8 bits), else -1 / 0 / -1
 *                                                              hard: a run of more than 9 digits
 *   TLEN     an optional `-`, the run of digits; none -> 0     hard: a run of more than 9 digits
 *   CIGAR    first byte `*` with flag bit 0x4 set; or items of 1-9 digits and one byte: M, D, N in either case add to the end
 *            (u32 wrap-around), every other byte counts as an operation just the same
 *                                                              hard: `*` on a mapped record, an item without digits, digits up to the end
 *   SEQ      `*` -> 0, else its length
 *   optional fields   the first that starts with `XA:` and the first that starts with `NM:`. XA's value: the bytes behind `XA:Z:` /
 *            `XA:H:` up to the next tab — empty for another type byte, or when fewer than 5 bytes are left up to the END OF THE LINE.
 *            NM: `NM:i:`, an optional `-`, 1-9 digits; not of the form `NM:i:` (or fewer than 5 bytes left in the line) -> 0
 *                                                              hard: `NM:i:` followed by anything else, when the record carries XA too
 *   the line at least 11 tab-separated fields                  hard: fewer fields, a NUL byte, an empty line
 *
 *   tmpend = n_cigar ? end : pos + l_qseq, in u32 arithmetic.
 *
 * The caller cuts the line: terminator excluded, every trailing '\r' stripped (itx_sam_strip).
 *
 * ITX_SAMLINE_DEFINE(FN, PTR, LOOKUP) defines
 *     void FN(PTR p, uint32_t len, const void *names, ItxSamRec *r)
 * over a byte source of pointer type PTR (`const uint8_t *`, or the same in another address space);
 * LOOKUP(names, p, n) gives the reference id of the n bytes at p, or a negative value when the header lacks the name. */
#ifndef ITX_SAMLINE_H
#define ITX_SAMLINE_H
#include <stdint.h>

#ifndef ITX_SAM_FN
#ifdef __HIPCC__
#define ITX_SAM_FN static __host__ __device__ inline
#else
#define ITX_SAM_FN static inline
#endif
#endif

typedef struct ItxSamRec {
    int32_t tid, pos, tmpend, mpos, isize, nm;
    uint32_t flag;                 /* the raw value: ITX_FLAG5 and the PAIRED bit both derive from it */
    uint32_t qname_len;            /* the read name is the line's first qname_len bytes */
    uint32_t xa_off, xa_len;       /* the XA value, offset from the line's first byte (has_xa; a length of 0: the empty string) */
    uint8_t mapq, has_xa, hard;
} ItxSamRec;

/* the length of a line without its trailing '\r's (the '\n' already excluded) */
#define ITX_SAM_STRIP(p, len)                                   \
    do {                                                        \
        while ((len) > 0 && (p)[(len) - 1] == '\r') (len)--;    \
    } while (0)

#define ITX_SAM_ISDIG(c) ((uint32_t)(c) - 48u < 10u)
/* the run of digits at k (stops at `e`): value into v (meaningful up to 9 digits), count into nd; k ends behind the run */
#define ITX_SAM_RUN(p, k, e, v, nd)                                \
    do {                                                           \
        (v) = 0;                                                   \
        (nd) = 0;                                                  \
        while ((k) < (e) && ITX_SAM_ISDIG((p)[k])) {               \
            (v) = (v) * 10u + ((uint32_t)(p)[k] - 48u);            \
            (nd)++;                                                \
            (k)++;                                                 \
        }                                                          \
    } while (0)
/* field [a, e): e at the next tab or at the line's end; a NUL byte makes the line hard */
#define ITX_SAM_FIELD(p, a, e, len, hard)                          \
    do {                                                           \
        (e) = (a);                                                 \
        while ((e) < (len) && (p)[e] != '\t') {                    \
            if ((p)[e] == 0) (hard) = 1;                           \
            (e)++;                                                 \
        }                                                          \
    } while (0)
/* the field behind [a, e), which has to exist */
#define ITX_SAM_NEXT(p, a, e, len, hard, r)                        \
    do {                                                           \
        if ((e) >= (len)) {                                        \
            (r)->hard = 1;                                         \
            return;                                                \
        }                                                          \
        (a) = (e) + 1u;                                            \
        ITX_SAM_FIELD(p, a, e, len, hard);                         \
    } while (0)

#define ITX_SAMLINE_DEFINE(FN, PTR, LOOKUP)                                                                                 \
    ITX_SAM_FN void FN(PTR p, uint32_t len, const void *names, ItxSamRec *r)                                                \
    {                                                                                                                       \
        uint32_t a = 0, e, k, v, nd, hard = 0;                                                                              \
        r->tid = -1; r->pos = -1; r->tmpend = -1; r->mpos = -1; r->isize = 0; r->nm = 0;                                    \
        r->flag = 0; r->qname_len = 0; r->xa_off = 0; r->xa_len = 0; r->mapq = 0; r->has_xa = 0; r->hard = 0;               \
        if (len == 0) {                                                                                                     \
            r->hard = 1;                                                                                                    \
            return;                                                                                                         \
        }                                                                                                                   \
        ITX_SAM_FIELD(p, a, e, len, hard);                                             /* QNAME */                          \
        r->qname_len = e;                                                                                                   \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* FLAG */                           \
        k = a;                                                                                                              \
        ITX_SAM_RUN(p, k, e, v, nd);                                                                                        \
        if (nd == 0 || nd > 9u || k != e || (p[a] == '0' && nd > 1u)) hard = 1;                                             \
        const uint32_t flag = v;                                                                                            \
        r->flag = flag;                                                                                                     \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* RNAME */                          \
        if (!(e - a == 1u && p[a] == '*')) {                                                                                \
            const int64_t t = hard ? -1 : (int64_t)LOOKUP(names, p + a, e - a);                                             \
            if (t < 0) hard = 1;                                                                                            \
            r->tid = (int32_t)t;                                                                                            \
        }                                                                                                                   \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* POS */                            \
        k = a;                                                                                                              \
        ITX_SAM_RUN(p, k, e, v, nd);                                                                                        \
        if (nd > 9u) hard = 1;                                                                                              \
        const uint32_t pos = nd ? v - 1u : 0xffffffffu;                                                                     \
        r->pos = (int32_t)pos;                                                                                              \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* MAPQ */                           \
        k = a;                                                                                                              \
        ITX_SAM_RUN(p, k, e, v, nd);                                                                                        \
        if (nd > 9u) hard = 1;                                                                                              \
        r->mapq = (uint8_t)v;                                                                                               \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* CIGAR */                          \
        uint32_t end = pos, n_cigar = 0;                                                                                    \
        if (e > a && p[a] == '*') {                                                                                         \
            if (!(flag & 4u)) hard = 1;                                                                                     \
        } else {                                                                                                            \
            k = a;                                                                                                          \
            while (k < e) {                                                                                                 \
                ITX_SAM_RUN(p, k, e, v, nd);                                                                                \
                if (nd == 0 || nd > 9u || k == e) {                                                                         \
                    hard = 1;                                                                                               \
                    break;                                                                                                  \
                }                                                                                                           \
                const uint32_t op = (uint32_t)p[k] & ~32u;                             /* M D N and m d n */                \
                if (op == 'M' || op == 'D' || op == 'N') end += v;                                                          \
                n_cigar++;                                                                                                  \
                k++;                                                                                                        \
            }                                                                                                               \
        }                                                                                                                   \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* RNEXT */                          \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* PNEXT */                          \
        k = a;                                                                                                              \
        ITX_SAM_RUN(p, k, e, v, nd);                                                                                        \
        if (nd > 9u) hard = 1;                                                                                              \
        r->mpos = nd ? (int32_t)(v - 1u) : -1;                                                                              \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* TLEN */                           \
        k = a;                                                                                                              \
        const uint32_t neg = k < e && p[k] == '-';                                                                          \
        k += neg;                                                                                                           \
        ITX_SAM_RUN(p, k, e, v, nd);                                                                                        \
        if (nd > 9u) hard = 1;                                                                                              \
        r->isize = neg ? -(int32_t)v : (int32_t)v;                                                                          \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* SEQ */                            \
        const uint32_t l_qseq = (e - a == 1u && p[a] == '*') ? 0u : e - a;                                                  \
        r->tmpend = (int32_t)(n_cigar ? end : pos + l_qseq);                                                                \
        ITX_SAM_NEXT(p, a, e, len, hard, r);                                           /* QUAL */                           \
        uint32_t have_nm = 0, nm_hard = 0;                                                                                  \
        while (e < len) {                                                              /* the optional fields */            \
            a = e + 1u;                                                                                                     \
            ITX_SAM_FIELD(p, a, e, len, hard);                                                                              \
            if (a + 3u > len || p[a + 2u] != ':') continue;                                                                 \
            if (!r->has_xa && p[a] == 'X' && p[a + 1u] == 'A') {                                                            \
                r->has_xa = 1;                                                                                              \
                r->xa_off = a + 3u;                                                                                         \
                if (len - a >= 5u && (p[a + 3u] == 'Z' || p[a + 3u] == 'H') && p[a + 4u] == ':') {                          \
                    r->xa_off = a + 5u;                                                                                     \
                    r->xa_len = e - (a + 5u);                                                                               \
                }                                                                                                           \
            } else if (!have_nm && p[a] == 'N' && p[a + 1u] == 'M') {                                                       \
                have_nm = 1;                                                                                                \
                if (len - a >= 5u && p[a + 3u] == 'i' && p[a + 4u] == ':') {                                                \
                    k = a + 5u;                                                                                             \
                    const uint32_t nneg = k < e && p[k] == '-';                                                             \
                    k += nneg;                                                                                              \
                    ITX_SAM_RUN(p, k, e, v, nd);                                                                            \
                    if (nd == 0 || nd > 9u) nm_hard = 1;                                                                    \
                    r->nm = nneg ? -(int32_t)v : (int32_t)v;                                                                \
                }                                                                                                           \
            }                                                                                                               \
        }                                                                                                                   \
        if (r->has_xa && nm_hard) hard = 1;                                                                                 \
        r->hard = (uint8_t)hard;                                                                                            \
    }

#endif
