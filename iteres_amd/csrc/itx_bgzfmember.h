// itx_bgzfmember.h — one BGZF member (the gzip member of SAM/BAM files: RFC 1952 with the 6-byte "BC" extra field) made of a
// payload of at most ITX_BAMOUT_PAYLOAD bytes, by one wave on a GPU or by one "lane" on the host. The writer of `filter -b`
// (itx_bamout_members.hip) calls it per payload; tests/bgzfmember_host.cpp is the host build the device's bytes are held to.
//
// The member:
//   [0, 18)          1f 8b 08 04, mtime 0, XFL 0, OS 255, XLEN 6, 'B' 'C', SLEN 2, BSIZE = size - 1
//   [18, size - 8)   raw DEFLATE: what itxd_deflate (itx_deflate_core.h) writes without its 2-byte zlib head and its Adler sum.
//                    The core is called on out + 16, so that its head falls on bytes 16, 17 and its Adler sum on the 4 bytes
//                    behind the DEFLATE bytes; the frame's header and trailer are written over both afterwards.
//   [size - 8, size) CRC-32 of the payload, ISIZE = its length
// so size = (the zlib stream's size) + 20, at most n + 31, and BSIZE < 65536 for every n <= ITXD_MAX_IN.
//
// CRC-32 (the reflected 0xedb88320 of gzip), lane-parallel: lane l takes the CRC of the contiguous slice l of ceil(n / lanes)
// bytes. The CRC of a concatenation A B is crc(A) * x^(8 |B|) + crc(B) in GF(2)[x] modulo the polynomial (the pre- and
// post-conditioning cancel: zlib's crc32_combine is this rule), so every lane multiplies its slice's CRC by x^(8 * bytes behind
// the slice) and the member's CRC is the XOR of the lanes' terms. An empty slice's term is 0.
//
// The member's bytes are a pure function of the payload's bytes: the same for every number of lanes, on host and device.
// Hooks: those of itx_deflate_core.h, defined by the including file before this one.
#pragma once
#include "itx_deflate_core.h"

// Payload bytes per member. The encoder's workspace is 4 bytes of LDS per payload byte (the input, a length and a 2-byte distance
// per position) plus ~13.5 KB that do not depend on it (hash heads, code tables): 144 KB at 32768, 79 KB at 16384, 46 KB at 8192,
// 30 KB at 4096. A CU has 160 KB, and the parse is serial on one lane per member, so the encoder's rate follows the members in
// flight per CU: 1, 2, 3, 5. Measured on 1.43 GB of BAM records: 935 ms at 16384, 657 ms at 8192, for 1 % more output
// (a member's 26 bytes of frame, ~100 bytes of code tables and a window that starts empty, twice as often). Below 8192 the fixed
// part is half of the workspace and frame and tables 3 % of the payload: not tried. A multiple of 16: payloads start on vectors.
#define ITX_BAMOUT_PAYLOAD 8192u
#define ITX_BGZF_MEMBER_CAP(n) (ITXD_OUT_CAP(n) + 24u)      // room a member of n payload bytes may be built in (a multiple of 4)

#define ITX_CRC_POLY 0xedb88320u

// a * b modulo the polynomial; bit 31 is x^0 (the reflected form the CRC register has)
ITXD_FN uint32_t itx_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ ITX_CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 * len) modulo the polynomial, by squaring
ITXD_FN uint32_t itx_crc_xpow8(uint32_t len)
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;                  // 1, x^8
    for (; len; len >>= 1) {
        if (len & 1u) r = itx_crc_mul(r, sq);
        sq = itx_crc_mul(sq, sq);
    }
    return r;
}

// the CRC-32 of bytes [from, to) of `in` (little-endian words, as itxd_ws::in)
ITXD_FN uint32_t itx_crc32_slice(const uint32_t *in, uint32_t from, uint32_t to)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = from; i < to; i++) {
        c ^= itxd_byte(in, i);
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ ITX_CRC_POLY : c >> 1;
    }
    return ~c;
}

// lane `lane` of nl: its term of the CRC-32 of in[0, n); the XOR of all nl terms is the CRC
ITXD_FN uint32_t itx_crc32_term(const uint32_t *in, uint32_t n, uint32_t lane, uint32_t nl)
{
    const uint32_t per = (n + nl - 1u) / nl;
    const uint32_t from = lane * per < n ? lane * per : n, to = from + per < n ? from + per : n;
    if (from == to) return 0u;
    return itx_crc_mul(itx_crc32_slice(in, from, to), itx_crc_xpow8(n - to));
}

// The whole member: n (<= ITXD_MAX_IN) payload bytes in w.in -> the member at out (room: ITX_BGZF_MEMBER_CAP(n)); returns its size
// to every lane.
ITXD_FN uint32_t itx_bgzf_member(const itxd_ws &w, uint32_t n, uint8_t *out, uint32_t lane, uint32_t nl)
{
    const uint32_t term = itx_crc32_term(w.in, n, lane, nl);
    const uint32_t size = itxd_deflate(w, n, out + 16, lane, nl) + 20u;
    w.red[lane] = term;                                            // (the core is through with its Adler sums)
    ITXD_SYNC();
    if (lane == 0) {
        uint32_t crc = 0;
        for (uint32_t l = 0; l < nl; l++) crc ^= (uint32_t)w.red[l];
        static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int i = 0; i < 16; i++) out[i] = head[i];
        out[16] = (uint8_t)(size - 1u);
        out[17] = (uint8_t)((size - 1u) >> 8);
        uint8_t *t = out + size - 8u;
        for (int i = 0; i < 4; i++) {
            t[i] = (uint8_t)(crc >> (8 * i));
            t[4 + i] = (uint8_t)(n >> (8 * i));
        }
    }
    ITXD_SYNC();
    return size;
}
