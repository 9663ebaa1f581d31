// itx_bgzflevels.h — the levels of a BGZF member of `filter -b -l` (itx_bamout_members.hip calls it per payload; tests/bgzflevels_host.cpp
// is the host build the device's bytes are held to). The frame, the CRC-32 and ISIZE are itx_bgzfmember.h's at every level; what
// differs is the DEFLATE block between them:
//   level 6   itx_bgzf_member, unchanged: the default, and the only level without -l
//   level 0   one stored block: 18 bytes of header, 01, LEN, NLEN, the n payload bytes, CRC-32, ISIZE: n + 31 bytes
//   level 1   itxf_block (itx_deflate_fast.h): a dynamic-Huffman block whose parse is cut into slices of 128 positions that the
//             lanes take independently; stored whenever that is not larger, so a member never exceeds n + 31 bytes
// Levels 0 and 1 build the whole member in the staging area (itxf_ws::stage, ITXF_STAGE_WORDS(n, 18) words) and store it to `out`
// in whole words, a word per lane: `out` is 4-byte aligned and has room for ITX_BGZF_MEMBER_CAP(n) bytes, as for level 6. The
// bytes behind the member in its last word are zero.
// The member's bytes are a pure function of the payload's bytes and the level, for any number of lanes, on host and device.
// Hooks: those of itx_deflate_fast.h, defined by the including file before this one.
#pragma once
#include "itx_bgzfmember.h"
#include "itx_deflate_fast.h"

#define ITX_BGZF_LEAD 18u                                          // bytes of a member in front of its DEFLATE block
#define ITX_BGZF_LEVEL_OK(l) ((l) == 0 || (l) == 1 || (l) == 6)

// The whole member at `level` (0, 1 or 6; the same for every lane): n (<= ITXD_MAX_IN) payload bytes in w.d.in -> the member at
// out; returns its size to every lane.
ITXD_FN uint32_t itx_bgzf_member_level(const itxf_ws &w, uint32_t n, uint8_t *out, uint32_t lane, uint32_t nl, uint32_t level)
{
    if (level == 6u) return itx_bgzf_member(w.d, n, out, lane, nl);
    w.d.red[lane] = itx_crc32_term(w.d.in, n, lane, nl);          // (read behind the block's barriers)
    const uint32_t size = (level == 1u ? itxf_block(w, n, ITX_BGZF_LEAD, lane, nl) : itxf_stored(w, n, ITX_BGZF_LEAD, lane, nl)) + 26u;
    if (lane == 0) {
        uint32_t crc = 0;
        for (uint32_t l = 0; l < nl; l++) crc ^= (uint32_t)w.d.red[l];
        static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        uint8_t *o = (uint8_t *)w.stage;
        for (int i = 0; i < 16; i++) o[i] = head[i];
        o[16] = (uint8_t)(size - 1u);
        o[17] = (uint8_t)((size - 1u) >> 8);
        uint8_t *t = o + size - 8u;
        for (int i = 0; i < 4; i++) {
            t[i] = (uint8_t)(crc >> (8 * i));
            t[4 + i] = (uint8_t)(n >> (8 * i));
        }
    }
    ITXD_SYNC();
    uint32_t *o32 = (uint32_t *)out;
    for (uint32_t i = lane; i < (size + 3u) / 4u; i += nl) o32[i] = w.stage[i];
    ITXD_SYNC();
    return size;
}
