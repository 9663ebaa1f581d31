// itx_auxwalk.h — the walk over a BAM record's optional fields, as the reference walks them (cussamtools/bam_aux.c:28-48
// bam_aux_get with __skip_tag, bam.h:754-760 bam_aux_type2size), and the two readings of a found tag (bam_aux.c:159-170
// bam_aux2i, 199-206 bam_aux2Z). Stated once, for the device (csrc/itx_bamwin.hip k_parse, csrc/itx_xaveto.hip, csrc/itx_bedline.h)
// and for the host program (host/aln_priv.h; gcc, C11). tests/auxmodel.py is the literal restatement the suite holds it to.
//
// The reference's walk is not the SAM specification's. After the two name bytes it upper-cases the type byte and then:
//   Z, H        skips to behind the NUL
//   B           skips 5 + size(subtype) * count, the subtype byte taken AS IT IS: c C A 1, s S 2, i I f 4, anything else 0
//   otherwise   skips size(upper-cased type): C A 1, S 2, I 4 and 0 for everything else — among them F and D, because the size
//               table knows only the lower-case f. Behind a float, a double or a tag of an unknown type the walk therefore
//               goes on INSIDE the value: its bytes are read as the next tags' names and types.
// Where the reference would read a byte at or past the record's end (the second name byte, the type byte of a tag it skips,
// a string without its NUL, an array header, an array with a negative count) its answer depends on what lies behind the
// record in its buffer. There the walk here stops and the tag counts as not found; a value or a string that would run past
// the end reads as 0 or as empty. Nothing outside [s, end) is ever read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef ITX_AUX_FN
#ifdef __HIPCC__
#define ITX_AUX_FN static __host__ __device__ inline
#else
#define ITX_AUX_FN static inline
#endif
#endif

#define ITX_AUX_TAG(a, b) ((uint32_t)(uint8_t)(a) << 8 | (uint32_t)(uint8_t)(b))

// Where a record's optional fields lie: p points at the record's block_len. Returns 0 when there are none (bam1_aux at or
// behind the record's end).
ITX_AUX_FN int itx_aux_bounds(const uint8_t *p, const uint8_t **s, const uint8_t **end)
{
    const uint32_t block_len = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    const uint32_t dlen = block_len - 32u;
    const uint32_t l_qname = p[12], n_cigar = (uint32_t)p[16] | (uint32_t)p[17] << 8;
    const int32_t l_qseq = (int32_t)((uint32_t)p[20] | (uint32_t)p[21] << 8 | (uint32_t)p[22] << 16 | (uint32_t)p[23] << 24);
    const uint64_t ql = l_qseq > 0 ? (uint64_t)l_qseq : 0;
    const uint64_t off = (uint64_t)l_qname + 4ull * n_cigar + (ql + 1) / 2 + ql;
    *s = p + 36 + (off < dlen ? off : dlen);
    *end = p + 36 + dlen;
    return off < dlen;
}

// bam_aux_get for up to two tags in one pass (both walks of the reference visit the same positions): *a / *b become the TYPE
// byte's position of the first tag named ta / tb (ITX_AUX_TAG), or NULL. b == NULL: only ta is looked for. A found position
// may be `end` itself (the name's two bytes are the record's last): read it through itx_aux_int / itx_aux_str only.
ITX_AUX_FN void itx_aux_find(const uint8_t *s, const uint8_t *end, uint32_t ta, const uint8_t **a, uint32_t tb, const uint8_t **b)
{
    *a = NULL;
    if (b) *b = NULL;
    while (s < end) {
        if (end - s < 2) return;                                    // s[1] lies outside
        const uint32_t x = (uint32_t)s[0] << 8 | s[1];
        s += 2;
        if (x == ta && !*a) {
            *a = s;
            if (!b || *b) return;
        }
        if (b && x == tb && !*b) {
            *b = s;
            if (*a) return;
        }
        if (s >= end) return;                                       // the type byte lies outside
        uint32_t type = *s++;
        if (type >= 'a' && type <= 'z') type -= 32u;
        if (type == 'Z' || type == 'H') {
            while (s < end && *s) ++s;
            if (s >= end) return;                                   // no NUL inside the record
            ++s;
        } else if (type == 'B') {
            if (end - s < 5) return;                                // the array's header lies outside
            const uint32_t sub = s[0];
            const int32_t cnt = (int32_t)((uint32_t)s[1] | (uint32_t)s[2] << 8 | (uint32_t)s[3] << 16 | (uint32_t)s[4] << 24);
            if (cnt < 0) return;                                    // the reference steps backwards
            const uint32_t esz = (sub == 'c' || sub == 'C' || sub == 'A') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            const uint64_t adv = 5ull + (uint64_t)esz * (uint32_t)cnt;
            if (adv >= (uint64_t)(end - s)) return;                 // the loop's own end: nothing more inside the record
            s += adv;
        } else {
            const uint32_t adv = (type == 'C' || type == 'A') ? 1u : type == 'S' ? 2u : type == 'I' ? 4u : 0u;
            if (adv >= (size_t)(end - s)) return;                   // the loop's own end
            s += adv;
        }
    }
}

// bam_aux2i of a found tag (t: its type byte, or NULL): c C s S i I, 0 for every other type
ITX_AUX_FN int32_t itx_aux_int(const uint8_t *t, const uint8_t *end)
{
    if (!t || t >= end) return 0;
    const uint32_t type = *t++;
    const size_t left = (size_t)(end - t);
    if (type == 'c' && left >= 1) return (int32_t)(int8_t)t[0];
    if (type == 'C' && left >= 1) return (int32_t)t[0];
    if (type == 's' && left >= 2) return (int32_t)(int16_t)(uint16_t)((uint32_t)t[0] | (uint32_t)t[1] << 8);
    if (type == 'S' && left >= 2) return (int32_t)((uint32_t)t[0] | (uint32_t)t[1] << 8);
    if ((type == 'i' || type == 'I') && left >= 4) return (int32_t)((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24);
    return 0;
}

// bam_aux2Z of a found tag: the string's first byte and, in *len, its length. A tag of a type other than Z / H has no string
// (the reference crashes on it), one whose NUL lies outside the record is undefined there: both read as empty, *len = 0,
// and the position returned is then just a valid one to add 0 bytes to.
ITX_AUX_FN const uint8_t *itx_aux_str(const uint8_t *t, const uint8_t *end, uint32_t *len)
{
    *len = 0;
    if (!t || t >= end || (*t != 'Z' && *t != 'H')) return end;
    const uint8_t *z = t + 1;
    while (z < end && *z) ++z;
    if (z >= end) return end;
    *len = (uint32_t)(z - (t + 1));
    return t + 1;
}
