// itx_deflate_fast.h — one final DEFLATE block (RFC 1951) of at most 32 KiB of input in which every stage uses the whole wave: the
// fast level of the BAM's members (itx_bgzflevels.h). It stands on itx_deflate_core.h and takes from it, unchanged, the workspace
// (itxd_ws), the match finder (itxd_matches), the symbol rules (itxd_lsym / itxd_dsym), the code construction (itxd_huff /
// itxd_rle) and the header's bit writer. What differs is the parse: the core's runs on lane 0 over all positions, twice (greedy
// with a lazy step, matches extended to 258); this one is cut into slices that lanes take independently.
//
// The rule:
//   1. matches: itxd_matches, as it is.
//   2. the parse, in fixed slices of ITXF_SLICE (128) positions: slice s covers [128 s, min(128 s + 128, n)) and lane s % lanes
//      takes it. Greedy from the slice's first position: the position's match is taken, cut so that it ends inside the slice; a
//      cut that leaves fewer than ITXD_MINM bytes makes a literal. No lazy step, no match longer than ITXD_CAP. Distances reach
//      back across slices freely: the window is the whole input. The slice is a constant of the rule, not the lane count, which
//      is what makes 1 lane and 64 lanes write the same bytes.
//   3. frequencies: every lane adds its slices' symbols into the shared fq[] (an atomic add: sums do not depend on order) and its
//      extra bits into one shared total.
//   4. codes: itxd_huff / itxd_rle as they are; lane 0 writes the block header.
//   5. bits: every lane measures its slices under the codes, an exclusive sum gives every slice its first bit behind the block
//      header, and every lane writes its slices' bits there. The block is built in a zeroed staging area in LDS, so two slices
//      that share a word combine by an atomic OR; the caller stores the staging area to memory in whole words. The end-of-block
//      symbol follows the last slice.
//   6. a stored block is written whenever the Huffman block is not smaller: a block never exceeds n + 5 bytes.
// The walk over a slice runs three times (count, measure, write); nothing is a lane-0 loop over positions.
// The block's bytes are a pure function of the input bytes, for any number of lanes, on host and device.
//
// Hooks, beside the core's: ITXD_AADD(p, v) and ITXD_AOR(p, v), an atomic add and an atomic OR on a uint32_t in LDS (plain
// operations for one lane on the host). The device's are in itx_deflate_device.h with the core's; a host build defines them
// only when it includes this header.
#pragma once
#include "itx_deflate_core.h"

#if !defined(ITXD_AADD) || !defined(ITXD_AOR)
#error "define ITXD_AADD and ITXD_AOR before including this file"
#endif

#define ITXF_SLICE 128u                                            // positions per slice of the parse
#define ITXF_SLICES(n) (((uint32_t)(n) + ITXF_SLICE - 1u) / ITXF_SLICE)
// words of staging area for `lead` bytes, a block of n input bytes (at most n + 5) and 8 bytes behind it
#define ITXF_STAGE_WORDS(n, lead) (((uint32_t)(lead) + (uint32_t)(n) + 13u + 3u) / 4u)

// the core's workspace and what the fast block needs beside it
struct itxf_ws {
    itxd_ws d;
    uint32_t *stage;    // ITXF_STAGE_WORDS(n, lead): the block in the making. It may be d.head's memory (the hash heads are dead
                        // when it is first written), which is where the device build puts it.
    uint32_t *sbits;    // ITXF_SLICES(n) + 1: every slice's bit length, then its first bit
};

// the symbols of positions [from, to), greedy, matches cut at `to`: lit(byte) or mat(length, distance) per symbol
template <class LIT, class MAT>
ITXD_FN void itxf_walk(const itxd_ws &w, uint32_t from, uint32_t to, LIT lit, MAT mat)
{
    for (uint32_t p = from; p < to;) {
        uint32_t L = w.ml[p];
        if (L > to - p) L = to - p;
        if (L < ITXD_MINM) {
            lit(itxd_byte(w.in, p));
            p++;
        } else {
            mat(L, (uint32_t)w.md[p]);
            p += L;
        }
    }
}

// bits into the staging area from any bit on: whole words leave with an atomic OR (a slice's first and last word are shared)
struct itxf_bits {
    uint32_t *st;
    uint32_t wi;
    uint64_t acc;
    uint32_t nb;        // < 32 between calls
};

ITXD_FN void itxf_put(itxf_bits &b, uint32_t v, uint32_t n)         // n <= 32
{
    b.acc |= (uint64_t)v << b.nb;
    b.nb += n;
    if (b.nb >= 32u) {
        ITXD_AOR(&b.st[b.wi], (uint32_t)b.acc);
        b.wi++;
        b.acc >>= 32;
        b.nb -= 32u;
    }
}

ITXD_FN void itxf_flush(itxf_bits &b)
{
    if (b.nb) ITXD_AOR(&b.st[b.wi], (uint32_t)b.acc);
}

// A stored block of the n bytes in w.d.in at byte `lead` of the staging area: 01, LEN, NLEN, the bytes (copied a word per lane).
// Zeroes the area first; returns n + 5 to every lane.
ITXD_FN uint32_t itxf_stored(const itxf_ws &x, uint32_t n, uint32_t lead, uint32_t lane, uint32_t nl)
{
    const uint32_t at = lead + 5u;                                 // the first payload byte
    const uint32_t k0 = (at + 3u) / 4u, k1 = (at + n + 3u) / 4u;   // the words that start inside the payload
    for (uint32_t i = lane; i < ITXF_STAGE_WORDS(n, lead); i += nl) x.stage[i] = 0;
    ITXD_SYNC();
    for (uint32_t k = k0 + lane; k < k1; k += nl) x.stage[k] = itxd_ld32(x.d.in, 4u * k - at);      // (in[] is zero beyond n)
    if (lane == 0) {
        uint8_t *o = (uint8_t *)x.stage;
        o[lead] = 1;
        o[lead + 1u] = (uint8_t)n;
        o[lead + 2u] = (uint8_t)(n >> 8);
        o[lead + 3u] = (uint8_t)~n;
        o[lead + 4u] = (uint8_t)(~n >> 8);
        for (uint32_t i = 0; at + i < 4u * k0 && i < n; i++) o[at + i] = (uint8_t)itxd_byte(x.d.in, i);
    }
    ITXD_SYNC();
    return n + 5u;
}

// The block of the n (<= ITXD_MAX_IN) bytes in w.d.in at byte `lead` of the staging area; returns its size in bytes to every lane.
// The staging area is zero wherever the block did not write.
ITXD_FN uint32_t itxf_block(const itxf_ws &x, uint32_t n, uint32_t lead, uint32_t lane, uint32_t nl)
{
    const itxd_ws &w = x.d;
    const uint32_t S = ITXF_SLICES(n);
    for (uint32_t s = lane; s < ITXD_NSYM; s += nl) w.fq[s] = 0;
    if (lane == 0) w.misc[1] = 0;
    itxd_matches(w, n, lane, nl);                                  // (its barriers order the zeroes above)
    for (uint32_t i = lane; i < ITXF_STAGE_WORDS(n, lead); i += nl) x.stage[i] = 0;
    // 3. frequencies
    {
        uint32_t ebits = 0;
        for (uint32_t s = lane; s < S; s += nl) {
            const uint32_t from = s * ITXF_SLICE, to = from + ITXF_SLICE < n ? from + ITXF_SLICE : n;
            itxf_walk(
                w, from, to, [&](uint32_t c) { ITXD_AADD(&w.fq[c], 1u); },
                [&](uint32_t L, uint32_t D) {
                    uint32_t ls, le, lv, ds, de, dv;
                    itxd_lsym(L, ls, le, lv);
                    itxd_dsym(D, ds, de, dv);
                    ITXD_AADD(&w.fq[ls], 1u);
                    ITXD_AADD(&w.fq[286u + ds], 1u);
                    ebits += le + de;
                });
        }
        if (ebits) ITXD_AADD(&w.misc[1], ebits);
    }
    ITXD_SYNC();
    // 4. codes (the core's steps around itxd_huff, for this parse)
    if (lane == 0) {
        w.fq[256]++;                                               // end of block
        uint32_t nlit = 0, ndist = 0;                              // every code gets at least two symbols, as in the core
        for (uint32_t s = 0; s < 286u; s++) nlit += w.fq[s] != 0;
        for (uint32_t s = 286u; s < 316u; s++) ndist += w.fq[s] != 0;
        if (nlit < 2) w.fq[0] += w.fq[0] ? 0u : 1u;
        if (ndist < 2) {
            if (!w.fq[286]) w.fq[286] = 1;
            else w.fq[287] = 1;
        }
    }
    ITXD_SYNC();
    itxd_huff(w, w.fq, 286u, 15u, w.len, w.code, lane, nl);
    itxd_huff(w, w.fq + 286, 30u, 15u, w.len + 286, w.code + 286, lane, nl);
    if (lane == 0) {
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257u && !w.len[hlit - 1]) hlit--;
        while (hdist > 1u && !w.len[286u + hdist - 1]) hdist--;
        for (int s = 0; s < 20; s++) w.clfq[s] = 0;
        itxd_bits nob = {nullptr, 0, 0, 0};
        w.misc[2] = itxd_rle(w, hlit, hdist, true, nob);
        uint32_t ncl = 0;
        for (int s = 0; s < 19; s++) ncl += w.clfq[s] != 0;
        if (ncl < 2) w.clfq[w.clfq[0] ? 1 : 0] = 1;
        w.misc[3] = hlit;
        w.misc[4] = hdist;
    }
    ITXD_SYNC();
    itxd_huff(w, w.clfq, 19u, 7u, w.cllen, w.clcode, lane, nl);
    if (lane == 0) {
        static const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const uint32_t hlit = w.misc[3], hdist = w.misc[4];
        uint32_t hclen = 19;
        while (hclen > 4u && !w.cllen[ord[hclen - 1]]) hclen--;
        uint64_t bits = 3u + 14u + 3u * hclen + w.misc[1] + w.misc[2];
        for (int s = 0; s < 19; s++) bits += (uint64_t)w.clfq[s] * w.cllen[s];
        for (uint32_t s = 0; s < 316u; s++) bits += (uint64_t)w.fq[s] * w.len[s];
        const uint32_t dyn = (uint32_t)((bits + 7u) / 8u), stored = 5u + n;
        w.misc[5] = dyn < stored ? 0u : 1u;                       // (the core's estimate and the core's rule)
        if (dyn < stored) {
            // the block header, bytewise into the zeroed area; its last, partial byte too: the first slice ORs into the rest of it
            itxd_bits b = {(uint8_t *)x.stage + lead, 0, 0, 0};
            itxd_put(b, 1, 1);
            itxd_put(b, 2, 2);
            itxd_put(b, hlit - 257u, 5);
            itxd_put(b, hdist - 1u, 5);
            itxd_put(b, hclen - 4u, 4);
            for (uint32_t i = 0; i < hclen; i++) itxd_put(b, w.cllen[ord[i]], 3);
            itxd_rle(w, hlit, hdist, false, b);
            if (b.nb) b.out[b.pos] = (uint8_t)b.acc;
            w.misc[6] = 8u * (lead + b.pos) + b.nb;               // the first slice's first bit
        }
    }
    ITXD_SYNC();
    if (w.misc[5]) return itxf_stored(x, n, lead, lane, nl);       // 6. (the same for every lane)
    // 5. every slice's length, its place, its bits
    for (uint32_t s = lane; s < S; s += nl) {
        const uint32_t from = s * ITXF_SLICE, to = from + ITXF_SLICE < n ? from + ITXF_SLICE : n;
        uint32_t bits = 0;
        itxf_walk(
            w, from, to, [&](uint32_t c) { bits += w.len[c]; },
            [&](uint32_t L, uint32_t D) {
                uint32_t ls, le, lv, ds, de, dv;
                itxd_lsym(L, ls, le, lv);
                itxd_dsym(D, ds, de, dv);
                bits += w.len[ls] + le + w.len[286u + ds] + de;
            });
        x.sbits[s] = bits;
    }
    ITXD_SYNC();
    if (lane == 0) {                                               // (a sum over slices, not positions: 64 of them in a BAM payload)
        uint32_t at = w.misc[6];
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t b = x.sbits[s];
            x.sbits[s] = at;
            at += b;
        }
        x.sbits[S] = at;
    }
    ITXD_SYNC();
    for (uint32_t s = lane; s < S; s += nl) {
        const uint32_t from = s * ITXF_SLICE, to = from + ITXF_SLICE < n ? from + ITXF_SLICE : n;
        itxf_bits b = {x.stage, x.sbits[s] >> 5, 0, x.sbits[s] & 31u};
        itxf_walk(
            w, from, to, [&](uint32_t c) { itxf_put(b, w.code[c], w.len[c]); },
            [&](uint32_t L, uint32_t D) {
                uint32_t ls, le, lv, ds, de, dv;
                itxd_lsym(L, ls, le, lv);
                itxd_dsym(D, ds, de, dv);
                itxf_put(b, w.code[ls] | lv << w.len[ls], w.len[ls] + le);                       // <= 15 + 5 bits
                itxf_put(b, w.code[286u + ds] | dv << w.len[286u + ds], w.len[286u + ds] + de);  // <= 15 + 13 bits
            });
        itxf_flush(b);
    }
    if (lane == 0) {
        itxf_bits b = {x.stage, x.sbits[S] >> 5, 0, x.sbits[S] & 31u};
        itxf_put(b, w.code[256], w.len[256]);
        itxf_flush(b);
        // (what was written, not the estimate: that counts the symbols a code was given only to have two)
        w.misc[7] = (x.sbits[S] + w.len[256] - 8u * lead + 7u) / 8u;
    }
    ITXD_SYNC();
    return w.misc[7];
}
