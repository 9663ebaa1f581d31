// itx_deflate_core.h — a zlib stream (RFC 1950 around one RFC 1951 block) of at most 32 KiB of input, made by one
// wave on a GPU, or by one "lane" on the host.
//
// What it replaces: zlib's compress() of the bigWig data sections and zoom blocks (host/bigwig.c z_compress). A bigWig is tens
// of thousands of independent blocks of <= 32 KiB, each inside one DEFLATE window, so one wave takes one block and the
// blocks need nothing from each other.
//
// The block's shape:
//   1. match finding, lane-parallel: every position p gets its best match among a few candidates: the fixed distances
//      1, 4, 8 and 32 (byte runs, runs of equal floats, and the 32-byte records of a zoom block) and the last earlier
//      position with the same hash of its first 3 bytes. The hash heads advance one chunk of 64 positions at a time: position p sees the
//      heads as they stood after the chunk before its own, and a head keeps the LARGEST position that hashed there
//      (an atomic max: what it holds does not depend on the order of the lanes). Lengths are measured up to ITXD_CAP.
//   2. the parse, serial (lane 0): greedy with one step of lazy evaluation, as zlib's deflate_slow; a match that reached
//      ITXD_CAP is extended there to its full length (<= 258). It runs twice: once to count symbol frequencies, once to
//      write the bits.
//   3. one dynamic-Huffman block with code lengths limited to 15 (7 for the code-length code): a lane-parallel rank sort
//      of the used symbols, then the in-place minimum-redundancy construction of Moffat and Katajainen and the usual
//      Kraft-sum repair of over-long codes. A stored block is written instead whenever it is not larger.
//   4. Adler-32 as a lane-parallel sum of b[i] and (n - i) * b[i].
// The output bytes are a pure function of the input bytes, and the host and device builds give the same bytes.
//
// Hooks the including file defines: ITXD_FN (function attributes), ITXD_SYNC() (a barrier of the block's lanes: the
// wave's workgroup on the device, nothing on the host), ITXD_AMAX(p, v) (atomic max of a uint32 in LDS), ITXD_CTZ(x).
// Device code includes itx_deflate_device.h, which defines them and has the workspace as an LDS struct.
#pragma once
#include <stdint.h>

#ifndef ITXD_FN
#error "define the ITXD_* hooks before including this file"
#endif

#define ITXD_MAX_IN 32768u                 // input bytes per block (one DEFLATE window)
#define ITXD_CAP 32u                       // match lengths measured in the parallel pass
#define ITXD_MINM 3u                       // shortest match taken
#define ITXD_HMASK 0xffffffu                // the hash covers 3 bytes
#define ITXD_HBITS 11u                     // hash heads: 2^11 of them
#define ITXD_CHUNK 64u                     // positions per step of the hash heads
#define ITXD_NSYM 320u                     // 286 literal/length + 30 distance symbols (+ pad); 19 code-length symbols reuse it
#define ITXD_OUT_CAP(n) ((((uint32_t)(n) + 16u) + 3u) & ~3u)   // output room per block: a stored block is n + 11 bytes

// LDS (device) or plain arrays (host) a block works in; `in` holds the input as little-endian words, zero beyond n,
// at least n / 4 + 3 words
struct itxd_ws {
    uint32_t *in;
    uint32_t *head;     // 1 << ITXD_HBITS
    uint8_t *ml;        // per position: best match length (0: none)
    uint16_t *md;       // per position: its distance
    uint32_t *fq;       // ITXD_NSYM: symbol counts (litlen 0..285, dist 286..315)
    uint32_t *key;      // ITXD_NSYM: sort keys, then the Huffman construction's array
    uint16_t *srt;      // ITXD_NSYM: used symbols by increasing frequency
    uint8_t *len;       // ITXD_NSYM: code lengths (litlen 0..285, dist 286..315)
    uint16_t *code;     // ITXD_NSYM: bit-reversed canonical codes
    uint32_t *clfq;     // 19 + 1
    uint8_t *cllen;     // 19 + 1
    uint16_t *clcode;   // 19 + 1
    uint64_t *red;      // 2 x lanes: Adler partial sums
    uint32_t *misc;     // 16 shared scalars
};

ITXD_FN uint32_t itxd_ld32(const uint32_t *in, uint32_t i)
{
    const uint32_t w = i >> 2, sh = (i & 3u) * 8u;
    const uint32_t a = in[w];
    return sh ? (a >> sh) | (in[w + 1] << (32u - sh)) : a;
}

ITXD_FN uint32_t itxd_byte(const uint32_t *in, uint32_t i) { return (in[i >> 2] >> ((i & 3u) * 8u)) & 255u; }

// matching bytes of positions p and c (c < p) from byte k on, at most lim in all
ITXD_FN uint32_t itxd_cmp(const uint32_t *in, uint32_t p, uint32_t c, uint32_t k, uint32_t lim)
{
    while (k < lim) {
        const uint32_t x = itxd_ld32(in, p + k) ^ itxd_ld32(in, c + k);
        if (x) {
            k += ITXD_CTZ(x) >> 3;
            break;
        }
        k += 4;
    }
    return k < lim ? k : lim;
}

ITXD_FN uint32_t itxd_hash(const uint32_t *in, uint32_t p) { return ((itxd_ld32(in, p) & ITXD_HMASK) * 2654435761u) >> (32u - ITXD_HBITS); }

// 1. best match per position
ITXD_FN void itxd_matches(const itxd_ws &w, uint32_t n, uint32_t lane, uint32_t nl)
{
    for (uint32_t i = lane; i < (1u << ITXD_HBITS); i += nl) w.head[i] = 0;
    ITXD_SYNC();
    for (uint32_t base = 0; base < n; base += ITXD_CHUNK) {
        const uint32_t end = base + ITXD_CHUNK < n ? base + ITXD_CHUNK : n;
        for (uint32_t p = base + lane; p < end; p += nl) {
            const uint32_t left = n - p, lim = left < ITXD_CAP ? left : ITXD_CAP;
            uint32_t best = 0, bd = 0;
            if (lim >= ITXD_MINM) {
                const uint32_t fixed[4] = {1u, 4u, 8u, 32u};
                for (int j = 0; j < 4; j++) {
                    const uint32_t d = fixed[j];
                    if (d > p) break;
                    const uint32_t l = itxd_cmp(w.in, p, p - d, 0, lim);
                    if (l > best) {
                        best = l;
                        bd = d;
                    }
                }
                const uint32_t h = w.head[itxd_hash(w.in, p)];
                if (h && best < lim) {
                    const uint32_t c = h - 1u;
                    const uint32_t l = itxd_cmp(w.in, p, c, 0, lim);
                    if (l > best) {
                        best = l;
                        bd = p - c;
                    }
                }
            }
            w.ml[p] = (uint8_t)(best >= ITXD_MINM ? best : 0u);
            w.md[p] = (uint16_t)bd;
        }
        ITXD_SYNC();
        for (uint32_t p = base + lane; p < end; p += nl)
            if (n - p >= ITXD_MINM) ITXD_AMAX(&w.head[itxd_hash(w.in, p)], p + 1u);
        ITXD_SYNC();
    }
}

// length 3..258 -> symbol 257..285, extra bits and their value
ITXD_FN void itxd_lsym(uint32_t L, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    const uint32_t x = L - 3u;
    if (L == 258u) {
        sym = 285u; eb = 0; ev = 0;
    } else if (x < 8u) {
        sym = 257u + x; eb = 0; ev = 0;
    } else {
        const uint32_t e = (31u - (uint32_t)__builtin_clz(x)) - 2u;
        sym = 257u + 4u * (e + 1u) + ((x >> e) & 3u);
        eb = e;
        ev = x & ((1u << e) - 1u);
    }
}

// distance 1..32768 -> symbol 0..29, extra bits and their value
ITXD_FN void itxd_dsym(uint32_t D, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    const uint32_t d = D - 1u;
    if (d < 4u) {
        sym = d; eb = 0; ev = 0;
    } else {
        const uint32_t e = (31u - (uint32_t)__builtin_clz(d)) - 1u;
        sym = 2u * (e + 1u) + ((d >> e) & 1u);
        eb = e;
        ev = d & ((1u << e) - 1u);
    }
}

struct itxd_bits {
    uint8_t *out;
    uint32_t pos;
    uint64_t acc;
    uint32_t nb;
};

ITXD_FN void itxd_put(itxd_bits &b, uint32_t v, uint32_t n)
{
    b.acc |= (uint64_t)v << b.nb;
    b.nb += n;
    while (b.nb >= 8u) {
        b.out[b.pos++] = (uint8_t)b.acc;
        b.acc >>= 8;
        b.nb -= 8u;
    }
}

ITXD_FN void itxd_align(itxd_bits &b)
{
    if (b.nb) itxd_put(b, 0, 8u - b.nb);
}

// 2. the parse. count: fq[] and the extra bits (returned); else: the symbols' bits into b
ITXD_FN uint32_t itxd_parse(const itxd_ws &w, uint32_t n, bool count, itxd_bits &b)
{
    uint32_t ebits = 0, p = 0;
    while (p < n) {
        const uint32_t l = w.ml[p];
        bool lit = l < ITXD_MINM;
        if (!lit && l < ITXD_CAP && p + 1u < n && w.ml[p + 1u] > l) lit = true;
        if (lit) {
            const uint32_t s = itxd_byte(w.in, p);
            if (count) w.fq[s]++;
            else itxd_put(b, w.code[s], w.len[s]);
            p++;
            continue;
        }
        const uint32_t d = w.md[p];
        uint32_t L = l;
        if (l == ITXD_CAP) {
            const uint32_t left = n - p;
            L = itxd_cmp(w.in, p, p - d, ITXD_CAP, left < 258u ? left : 258u);
        }
        uint32_t ls, le, lv, ds, de, dv;
        itxd_lsym(L, ls, le, lv);
        itxd_dsym(d, ds, de, dv);
        if (count) {
            w.fq[ls]++;
            w.fq[286u + ds]++;
            ebits += le + de;
        } else {
            itxd_put(b, w.code[ls], w.len[ls]);
            if (le) itxd_put(b, lv, le);
            itxd_put(b, w.code[286u + ds], w.len[286u + ds]);
            if (de) itxd_put(b, dv, de);
        }
        p += L;
    }
    return ebits;
}

ITXD_FN uint32_t itxd_rev(uint32_t c, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; i++) {
        r = (r << 1) | (c & 1u);
        c >>= 1;
    }
    return r;
}

// 3. code lengths (<= maxb) and codes of the nsym symbols fq[0..nsym) into len[] / code[]; every lane takes part
ITXD_FN void itxd_huff(const itxd_ws &w, uint32_t *fq, uint32_t nsym, uint32_t maxb, uint8_t *len, uint16_t *code, uint32_t lane,
                       uint32_t nl)
{
    // rank sort of the used symbols by (frequency, symbol): srt[0] is the rarest
    for (uint32_t s = lane; s < nsym; s += nl) {
        if (!fq[s]) continue;
        const uint64_t ks = (uint64_t)fq[s] << 9 | s;
        uint32_t r = 0;
        for (uint32_t t = 0; t < nsym; t++)
            if (fq[t] && ((uint64_t)fq[t] << 9 | t) < ks) r++;
        w.srt[r] = (uint16_t)s;
    }
    ITXD_SYNC();
    if (lane == 0) {
        uint32_t nu = 0;
        for (uint32_t s = 0; s < nsym; s++) {
            len[s] = 0;
            if (fq[s]) nu++;
        }
        uint32_t *A = w.key;
        for (uint32_t i = 0; i < nu; i++) A[i] = fq[w.srt[i]];
        // Moffat & Katajainen, in place: A[i] becomes the depth of the i-th rarest symbol
        if (nu == 1) {
            A[0] = 1;
        } else if (nu > 1) {
            A[0] += A[1];
            uint32_t root = 0, leaf = 2;
            for (uint32_t next = 1; next < nu - 1; next++) {
                if (leaf >= nu || A[root] < A[leaf]) {
                    A[next] = A[root];
                    A[root++] = next;
                } else {
                    A[next] = A[leaf++];
                }
                if (leaf >= nu || (root < next && A[root] < A[leaf])) {
                    A[next] += A[root];
                    A[root++] = next;
                } else {
                    A[next] += A[leaf++];
                }
            }
            A[nu - 2] = 0;
            for (int next = (int)nu - 3; next >= 0; next--) A[next] = A[A[next]] + 1u;
            int avbl = 1, used = 0, dpth = 0, root2 = (int)nu - 2, next = (int)nu - 1;
            while (avbl > 0) {
                while (root2 >= 0 && (int)A[root2] == dpth) {
                    used++;
                    root2--;
                }
                while (avbl > used) {
                    A[next--] = (uint32_t)dpth;
                    avbl--;
                }
                avbl = 2 * used;
                dpth++;
                used = 0;
            }
        }
        // codes longer than maxb: fold them in and repair the Kraft sum
        uint32_t num[33];
        for (int i = 0; i < 33; i++) num[i] = 0;
        for (uint32_t i = 0; i < nu; i++) num[A[i] < 32u ? A[i] : 32u]++;
        if (nu > 1) {
            for (uint32_t i = maxb + 1; i <= 32u; i++) num[maxb] += num[i];
            uint32_t total = 0;
            for (uint32_t i = maxb; i > 0; i--) total += num[i] << (maxb - i);
            while (total != (1u << maxb)) {
                num[maxb]--;
                for (uint32_t i = maxb - 1; i > 0; i--)
                    if (num[i]) {
                        num[i]--;
                        num[i + 1] += 2;
                        break;
                    }
                total--;
            }
        }
        uint32_t j = nu;
        for (uint32_t i = 1; i <= maxb; i++)
            for (uint32_t l = num[i]; l > 0; l--) len[w.srt[--j]] = (uint8_t)i;
        // canonical codes, bit-reversed for the LSB-first stream
        uint32_t bl[16], nc[16];
        for (int i = 0; i < 16; i++) bl[i] = 0;
        for (uint32_t s = 0; s < nsym; s++) bl[len[s]]++;
        bl[0] = 0;
        uint32_t c = 0;
        for (int i = 1; i < 16; i++) {
            c = (c + bl[i - 1]) << 1;
            nc[i] = c;
        }
        for (uint32_t s = 0; s < nsym; s++)
            code[s] = len[s] ? (uint16_t)itxd_rev(nc[len[s]]++, len[s]) : (uint16_t)0;
    }
    ITXD_SYNC();
}

// the code lengths of the header, run-length coded (RFC 1951 3.2.7). count: clfq[] and the extra bits; else: the bits
ITXD_FN uint32_t itxd_rle(const itxd_ws &w, uint32_t hlit, uint32_t hdist, bool count, itxd_bits &b)
{
    const uint32_t T = hlit + hdist;
    uint32_t i = 0, eb = 0;
    auto L = [&](uint32_t k) -> uint32_t { return k < hlit ? w.len[k] : w.len[286u + k - hlit]; };
    auto sym = [&](uint32_t s, uint32_t v, uint32_t n) {
        if (count) {
            w.clfq[s]++;
            eb += n;
        } else {
            itxd_put(b, w.clcode[s], w.cllen[s]);
            if (n) itxd_put(b, v, n);
        }
    };
    while (i < T) {
        const uint32_t v = L(i);
        uint32_t r = 1;
        while (i + r < T && L(i + r) == v) r++;
        i += r;
        if (v == 0) {
            while (r >= 11u) {
                const uint32_t k = r < 138u ? r : 138u;
                sym(18, k - 11u, 7);
                r -= k;
            }
            if (r >= 3u) {
                sym(17, r - 3u, 3);
                r = 0;
            }
            while (r) {
                sym(0, 0, 0);
                r--;
            }
        } else {
            sym(v, 0, 0);
            r--;
            while (r >= 3u) {
                const uint32_t k = r < 6u ? r : 6u;
                sym(16, k - 3u, 2);
                r -= k;
            }
            while (r) {
                sym(v, 0, 0);
                r--;
            }
        }
    }
    return eb;
}

// The whole block: n (<= ITXD_MAX_IN) bytes in w.in -> a zlib stream at out (room: ITXD_OUT_CAP(n)); returns its size to
// every lane.
ITXD_FN uint32_t itxd_deflate(const itxd_ws &w, uint32_t n, uint8_t *out, uint32_t lane, uint32_t nl)
{
    // 4. Adler-32
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t i = lane; i < n; i += nl) {
        const uint32_t v = itxd_byte(w.in, i);
        s1 += v;
        s2 += (uint64_t)(n - i) * v;
    }
    w.red[2 * lane] = s1;
    w.red[2 * lane + 1] = s2;
    for (uint32_t s = lane; s < ITXD_NSYM; s += nl) w.fq[s] = 0;
    ITXD_SYNC();
    itxd_matches(w, n, lane, nl);
    if (lane == 0) {
        uint64_t a = 0, bsum = 0;
        for (uint32_t l = 0; l < nl; l++) {
            a += w.red[2 * l];
            bsum += w.red[2 * l + 1];
        }
        w.misc[0] = (uint32_t)((1u + a) % 65521u) | (uint32_t)((n + bsum) % 65521u) << 16;
        itxd_bits nob = {nullptr, 0, 0, 0};
        w.misc[1] = itxd_parse(w, n, true, nob);
        w.fq[256]++;                                              // end of block
        // every code gets at least two symbols: a one-symbol code is incomplete, which inflaters need not accept
        uint32_t nlit = 0, ndist = 0;
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
        itxd_bits b = {out, 0, 0, 0};
        itxd_put(b, 0x78, 8);
        itxd_put(b, 0x9c, 8);
        if (dyn < stored) {
            itxd_put(b, 1, 1);
            itxd_put(b, 2, 2);
            itxd_put(b, hlit - 257u, 5);
            itxd_put(b, hdist - 1u, 5);
            itxd_put(b, hclen - 4u, 4);
            for (uint32_t i = 0; i < hclen; i++) itxd_put(b, w.cllen[ord[i]], 3);
            itxd_rle(w, hlit, hdist, false, b);
            itxd_parse(w, n, false, b);
            itxd_put(b, w.code[256], w.len[256]);
            itxd_align(b);
            w.misc[5] = 0;
        } else {
            itxd_put(b, 1, 1);
            itxd_put(b, 0, 2);
            itxd_align(b);
            itxd_put(b, n & 0xffffu, 16);
            itxd_put(b, ~n & 0xffffu, 16);
            w.misc[5] = 1;
        }
        w.misc[6] = b.pos;
    }
    ITXD_SYNC();
    uint32_t pos = w.misc[6];
    if (w.misc[5]) {
        for (uint32_t i = lane; i < n; i += nl) out[pos + i] = (uint8_t)itxd_byte(w.in, i);
        pos += n;
    }
    if (lane == 0) {
        const uint32_t ad = w.misc[0];
        out[pos] = (uint8_t)(ad >> 24);
        out[pos + 1] = (uint8_t)(ad >> 16);
        out[pos + 2] = (uint8_t)(ad >> 8);
        out[pos + 3] = (uint8_t)ad;
    }
    ITXD_SYNC();
    return pos + 4u;
}
