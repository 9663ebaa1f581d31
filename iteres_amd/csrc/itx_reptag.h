// itx_reptag.h — the tags of `iteres filter -b -a` (an extension): what a counted record carries about the table row it was counted
// for, stated once for the device (csrc/itx_bamout.hip), for the host route (host/stream.c, the C build) and for the host build the
// tests hold against a Python restatement (tests/reptag_host.cpp). Plain C over bytes and integers, valid as C and as C++.
//
//   record   the annotated record is the input record (rec points at its block_size field, rec_len = 4 + block_size bytes) with
//            the tag bytes behind it and block_size, its first four bytes, increased by their number. Nothing else changes: bin,
//            l_read_name, CIGAR, SEQ, QUAL and the aux bytes the record has stay as they are, ZN / ZC / ZF / ZS / ZE among them
//            (the input's aux bytes are not looked at; the new tags follow the old ones).
//   tags     'Z','N','Z', repName,   0        the three strings: columns 5, 6 and 7 of the row's .loci line
//            'Z','C','Z', repClass,  0
//            'Z','F','Z', repFamily, 0
//            'Z','S','I', genoStart  as uint32, little-endian: column 2 of the .loci line
//            'Z','E','I', genoEnd    as uint32, little-endian: column 3
//            26 bytes and the three names. Both integers always have type I, so the length is a function of the row alone: the
//            measure pass needs no look at the values. (Z? tags are the ones SAM v1 reserves for local use.)
//   pieces   itx_reptag_write lays bytes [from, to) of the annotated record at dst: itx_pack_tile (itx_textpack.h) asks for a record
//            in pieces wherever an LDS window or the tile's range cuts it, and a cut may fall anywhere — inside the patched
//            block_size, the original bytes, a key, a name or an integer. Only dst[0 .. to - from) is written.
#pragma once
#include <stdint.h>

#ifndef ITX_REPTAG_FN
#ifdef __HIPCC__
#define ITX_REPTAG_FN static __host__ __device__ inline
#else
#define ITX_REPTAG_FN static inline
#endif
#endif

#if defined(__clang__)
#define ITX_REPTAG_BYTE_LOOP _Pragma("clang loop vectorize(disable) unroll(disable)")  /* pieces start anywhere: byte loops stay byte loops */
#else
#define ITX_REPTAG_BYTE_LOOP
#endif

#define ITX_REPTAG_FIXED 26u             /* five keys of 3 bytes, three NULs, two integers */
#define ITX_REPTAG_MAX_NAME 65535u       /* a name of 2^16 bytes or more is refused where the names are taken */

/* the chosen row: its names (not NUL-terminated: pointer and length) and its coordinates */
typedef struct ItxRepTag {
    const uint8_t *rep, *cla, *fam;
    uint32_t rep_len, cla_len, fam_len;
    uint32_t start, end;
} ItxRepTag;

ITX_REPTAG_FN uint32_t itx_reptag_len(const ItxRepTag *t) { return ITX_REPTAG_FIXED + t->rep_len + t->cla_len + t->fam_len; }

/* the part of [from, to) inside the segment [sb, sb + sl), whose bytes are src[0 .. sl) */
ITX_REPTAG_FN void itx_reptag_bytes(uint8_t *dst, uint32_t from, uint32_t to, uint32_t sb, const uint8_t *src, uint32_t sl)
{
    const uint32_t a = from > sb ? from : sb, b = to < sb + sl ? to : sb + sl;
    uint32_t k;
    ITX_REPTAG_BYTE_LOOP
    for (k = a; k < b; k++) dst[k - from] = src[k - sb];
}

/* the same for a segment of n <= 4 bytes: the low n bytes of v, little-endian */
ITX_REPTAG_FN void itx_reptag_word(uint8_t *dst, uint32_t from, uint32_t to, uint32_t sb, uint32_t v, uint32_t n)
{
    const uint32_t a = from > sb ? from : sb, b = to < sb + n ? to : sb + n;
    uint32_t k;
    ITX_REPTAG_BYTE_LOOP
    for (k = a; k < b; k++) dst[k - from] = (uint8_t)(v >> (8u * (k - sb)));
}

#define ITX_REPTAG_KEY(c, type) ((uint32_t)'Z' | (uint32_t)(c) << 8 | (uint32_t)(type) << 16)

/* one string tag at `at`; returns where the next tag starts */
ITX_REPTAG_FN uint32_t itx_reptag_string(uint8_t *dst, uint32_t from, uint32_t to, uint32_t at, char c, const uint8_t *name, uint32_t n)
{
    itx_reptag_word(dst, from, to, at, ITX_REPTAG_KEY(c, 'Z'), 3u);
    itx_reptag_bytes(dst, from, to, at + 3u, name, n);
    itx_reptag_word(dst, from, to, at + 3u + n, 0u, 1u);
    return at + 4u + n;
}

ITX_REPTAG_FN uint32_t itx_reptag_integer(uint8_t *dst, uint32_t from, uint32_t to, uint32_t at, char c, uint32_t v)
{
    itx_reptag_word(dst, from, to, at, ITX_REPTAG_KEY(c, 'I'), 3u);
    itx_reptag_word(dst, from, to, at + 3u, v, 4u);
    return at + 7u;
}

/* bytes [from, to) of the annotated record into dst[0 .. to - from); from <= to <= rec_len + itx_reptag_len(t). The caller has
 * checked that rec_len + itx_reptag_len(t) fits the record's 32 bits (csrc/itx_bamout.hip: below BO_MAX_RECORD). */
ITX_REPTAG_FN void itx_reptag_write(const uint8_t *rec, uint32_t rec_len, const ItxRepTag *t, uint32_t from, uint32_t to, uint8_t *dst)
{
    uint32_t at = rec_len;
    if (from >= to) return;
    if (from < 4u) itx_reptag_word(dst, from, to, 0u, rec_len - 4u + itx_reptag_len(t), 4u);
    if (from < rec_len) itx_reptag_bytes(dst, from, to, 4u, rec + 4, rec_len - 4u);
    if (to <= rec_len) return;
    at = itx_reptag_string(dst, from, to, at, 'N', t->rep, t->rep_len);
    at = itx_reptag_string(dst, from, to, at, 'C', t->cla, t->cla_len);
    at = itx_reptag_string(dst, from, to, at, 'F', t->fam, t->fam_len);
    at = itx_reptag_integer(dst, from, to, at, 'S', t->start);
    (void)itx_reptag_integer(dst, from, to, at, 'E', t->end);
}
