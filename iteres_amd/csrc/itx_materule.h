// itx_materule.h — the mates of `iteres filter -b -s -m` (an extension), stated once for the device (csrc/itx_bamout_mates.hip), for
// the host route (itx_bamout_mates_append_host, same file) and for the host build the tests hold against a Python restatement
// (tests/materule_host.cpp, tests/matecase.py). Plain C over raw BAM record bytes, valid as C and as C++.
//
// A record is given as `rec`, which points at its block_size field, and `len`, the bytes that are there: 4 + block_size for a whole
// record. Only min(len, 4 + block_size) bytes are ever read. Offsets from rec: tid 4, pos 8, l_read_name 12, flag 18, mtid 24,
// mpos 28, the name 36 (l_read_name bytes, the NUL among them).
//
//   wanted(r)     a counted record wants a mate iff its fixed part is there, PAIRED (0x1) is set and MUNMAP (0x8) is clear. Without -T
//                 such a counted record is a READ1 counted as a pair (csrc/itx_derive.h); a read counted as a single end because its
//                 mate is unmapped wants nothing.
//   candidate(c)  PAIRED set and READ1 (0x40) clear; UNMAP (0x4), MUNMAP (0x8), 0x100 and 0x800 clear; tid >= 0 and pos >= 0; the
//                 record is whole: fixed part, l_read_name >= 1 and the name inside block_size. A candidate is never a counted record
//                 without -T, so the counted set and the mates are disjoint.
//   match(r, c)   c.tid == r.mtid, c.pos == r.mpos, and the names are equal in length and in every byte.
//   key           of a candidate (tid, pos, h32(name)), of a wanted record (mtid, mpos, h32(name)); h32 is 32-bit FNV-1a over the
//                 name's bytes without the NUL. Keys only bring records together: the verdict is match(), never the hash.
//   chosen        of several candidates that match one wanted record the first in stream order; a candidate several wanted records
//                 choose is written once (under -a with the tags of the earliest of them in stream order).
//   order         the -s order (csrc/itx_bamsortrule.h); among equal keys the counted records first in input order, then the mates in
//                 input order.
//   walk          itx_mate_next steps over the whole records of a host-route window, as itx_bamout_mates_append_host takes them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef ITX_MATE_FN
#ifdef __HIPCC__
#define ITX_MATE_FN static __host__ __device__ inline
#else
#define ITX_MATE_FN static inline
#endif
#endif

#define ITX_MATE_PAIRED 0x1u
#define ITX_MATE_UNMAP 0x4u
#define ITX_MATE_MUNMAP 0x8u
#define ITX_MATE_READ1 0x40u
#define ITX_MATE_SECONDARY 0x100u
#define ITX_MATE_SUPPLEMENTARY 0x800u
#define ITX_MATE_FIXED 36u               /* block_size and the 32 bytes behind it */
#define ITX_MATE_MAX_RECORD 0x40000000u  /* a record of a gibibyte is nobody's (csrc/itx_bamout_priv.h BO_MAX_RECORD) */

typedef struct ItxMateKey {
    uint32_t tid, pos, h32;              /* tid and pos as the unsigned words they are stored as: -1 sorts behind every reference */
} ItxMateKey;

ITX_MATE_FN uint32_t itx_mate_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* the bytes of the record that may be read: min(len, 4 + block_size); 0 when not even block_size is there */
ITX_MATE_FN uint32_t itx_mate_avail(const uint8_t *rec, uint32_t len)
{
    uint32_t bs;
    if (len < 4u) return 0u;
    bs = itx_mate_u32(rec);
    return bs < len - 4u ? 4u + bs : len;
}

ITX_MATE_FN int itx_mate_fixed(const uint8_t *rec, uint32_t len) { return itx_mate_avail(rec, len) >= ITX_MATE_FIXED; }

/* fixed part, l_read_name >= 1, the name inside the record */
ITX_MATE_FN int itx_mate_whole(const uint8_t *rec, uint32_t len)
{
    const uint32_t avail = itx_mate_avail(rec, len);
    if (avail < ITX_MATE_FIXED) return 0;
    return rec[12] >= 1u && (uint32_t)rec[12] <= avail - ITX_MATE_FIXED;
}

ITX_MATE_FN uint32_t itx_mate_flag(const uint8_t *rec) { return (uint32_t)rec[18] | (uint32_t)rec[19] << 8; }

ITX_MATE_FN int itx_mate_wanted(const uint8_t *rec, uint32_t len)
{
    uint32_t f;
    if (!itx_mate_fixed(rec, len)) return 0;
    f = itx_mate_flag(rec);
    return (f & ITX_MATE_PAIRED) != 0u && (f & ITX_MATE_MUNMAP) == 0u;
}

ITX_MATE_FN int itx_mate_candidate(const uint8_t *rec, uint32_t len)
{
    uint32_t f;
    if (!itx_mate_whole(rec, len)) return 0;
    f = itx_mate_flag(rec);
    if ((f & ITX_MATE_PAIRED) == 0u || (f & ITX_MATE_READ1) != 0u) return 0;
    if (f & (ITX_MATE_UNMAP | ITX_MATE_MUNMAP | ITX_MATE_SECONDARY | ITX_MATE_SUPPLEMENTARY)) return 0;
    return (int32_t)itx_mate_u32(rec + 4) >= 0 && (int32_t)itx_mate_u32(rec + 8) >= 0;
}

/* 32-bit FNV-1a over the n bytes of a name (the NUL is not among them) */
ITX_MATE_FN uint32_t itx_mate_h32(const uint8_t *name, uint32_t n)
{
    uint32_t h = 2166136261u, k;
    for (k = 0; k < n; k++) h = (h ^ name[k]) * 16777619u;
    return h;
}

/* the key of a candidate; the record is whole */
ITX_MATE_FN ItxMateKey itx_mate_key_candidate(const uint8_t *rec)
{
    ItxMateKey k;
    k.tid = itx_mate_u32(rec + 4);
    k.pos = itx_mate_u32(rec + 8);
    k.h32 = itx_mate_h32(rec + ITX_MATE_FIXED, (uint32_t)rec[12] - 1u);
    return k;
}

/* the key a wanted record looks its mate up by; the record is whole */
ITX_MATE_FN ItxMateKey itx_mate_key_wanted(const uint8_t *rec)
{
    ItxMateKey k;
    k.tid = itx_mate_u32(rec + 24);
    k.pos = itx_mate_u32(rec + 28);
    k.h32 = itx_mate_h32(rec + ITX_MATE_FIXED, (uint32_t)rec[12] - 1u);
    return k;
}

/* -1, 0, 1: keys ascend by tid, then pos, then h32, each as an unsigned word (the order the radix passes leave) */
ITX_MATE_FN int itx_mate_key_cmp(const ItxMateKey *a, const ItxMateKey *b)
{
    if (a->tid != b->tid) return a->tid < b->tid ? -1 : 1;
    if (a->pos != b->pos) return a->pos < b->pos ? -1 : 1;
    if (a->h32 != b->h32) return a->h32 < b->h32 ? -1 : 1;
    return 0;
}

/* candidate c is the mate wanted record r names; 0 when either is not whole */
ITX_MATE_FN int itx_mate_match(const uint8_t *r, uint32_t r_len, const uint8_t *c, uint32_t c_len)
{
    uint32_t k, n;
    if (!itx_mate_whole(r, r_len) || !itx_mate_whole(c, c_len)) return 0;
    if (itx_mate_u32(c + 4) != itx_mate_u32(r + 24) || itx_mate_u32(c + 8) != itx_mate_u32(r + 28)) return 0;
    if (c[12] != r[12]) return 0;
    n = (uint32_t)r[12] - 1u;
    for (k = 0; k < n; k++)
        if (c[ITX_MATE_FIXED + k] != r[ITX_MATE_FIXED + k]) return 0;
    return 1;
}

/* The walk over a host-route window: bytes[at .. len) starts with a whole record (block_size, then block_size bytes, below a
 * gibibyte): 0 and *next is where the one behind it starts; else 1 (the bytes are not whole records). at < len. */
ITX_MATE_FN int itx_mate_next(const uint8_t *bytes, size_t len, size_t at, size_t *next)
{
    uint32_t bs;
    if (len - at < 4u) return 1;
    bs = itx_mate_u32(bytes + at);
    if (bs >= ITX_MATE_MAX_RECORD || (size_t)bs > len - at - 4u) return 1;
    *next = at + 4u + (size_t)bs;
    return 0;
}
