// itx_textpack.h — device only: the variable-length pieces of a tile of TILE lanes packed into ONE contiguous range of an output
// (the bed lines of itx_bed.hip, the read names of itx_names.hip on their way into the pool and out of it into the text).
//
// Why the text is staged. The pieces are 20 - 120 bytes at offsets unrelated to anything, so stores from the lanes would be byte
// stores scattered over the output. But the tile's pieces follow one another, so the tile's output is one range [tb, te) known
// from two scans: k_tile_scan2 over the tiles' sums gives tb, itx_tile_offsets gives each lane's place [mb, me) inside it. The
// range is cut into windows of LDS bytes; every lane lays the part of its piece that falls into the window into shared memory
// (the caller's `lay(dst, from, to)` writes bytes [from, to) of the lane's piece at dst, so a piece longer than a window simply
// spans several), and the workgroup stores the window with one 16-byte vector per lane, coalesced.
// Why windows start on 16-byte boundaries of the OUTPUT (win = tb & ~15, then steps of LDS): vector v of the window is then the
// aligned vector at out + win + 16 v, whatever tb is.
// The ragged-vector rule: a vector goes as one uint4 store only where all 16 bytes lie inside [tb, te); the first and the last
// vector of a tile may hold a neighbour tile's bytes, which another workgroup writes, so those two go byte by byte, own bytes only.
// The output must be 16-byte aligned at offset 0; nothing outside [tb, te) is written.
//
// TILE and LDS are template parameters: bed packs 256 lines through 32 KiB, names 256 names through 16 KiB. The scan routines
// (wave_incl_scan_u32, itx_scan_chunk, itx_scan_wg) are in itx_device.h.
// Also here, for blocks that are made apart and packed afterwards (the bigWig blocks, the BAM's members): k_size_scan and
// k_pack_blocks.
#pragma once
#include "itx_device.h"

// exclusive sums over the tiles' sums, two 64-bit columns at once (tile k: tile_sum[2k], tile_sum[2k + 1]), and the two totals;
// one workgroup of ITX_SCAN_WG threads
static __global__ __launch_bounds__(ITX_SCAN_WG) void k_tile_scan2(const unsigned long long *__restrict__ tile_sum, uint32_t nt,
                                                                      unsigned long long *__restrict__ tile_base, unsigned long long *__restrict__ tot)
{
    __shared__ unsigned long long s[2][ITX_SCAN_WG];
    uint64_t lo, hi;
    itx_scan_chunk(nt, &lo, &hi);
    unsigned long long a = 0, b = 0, ta, tb;
    for (uint64_t k = lo; k < hi; k++) {
        a += tile_sum[2 * k];
        b += tile_sum[2 * k + 1];
    }
    unsigned long long ea = itx_scan_wg(a, s[0], &ta), eb = itx_scan_wg(b, s[1], &tb);
    for (uint64_t k = lo; k < hi; k++) {
        const unsigned long long ca = tile_sum[2 * k], cb = tile_sum[2 * k + 1];
        tile_base[2 * k] = ea;
        tile_base[2 * k + 1] = eb;
        ea += ca;
        eb += cb;
    }
    if (threadIdx.x == 0) {
        tot[0] = ta;
        tot[1] = tb;
    }
}

// exclusive sums of n sizes: off[0 .. n], 64 bit (the compressed blocks of a bigWig, the members of a BAM batch, all members of
// a BAM for its index); one workgroup of ITX_SCAN_WG threads, a thread sums a chunk of the sizes when there are more than that
static __global__ __launch_bounds__(ITX_SCAN_WG) void k_size_scan(const uint32_t *__restrict__ size, uint64_t n, uint64_t *__restrict__ off)
{
    __shared__ uint64_t s[ITX_SCAN_WG];
    uint64_t lo, hi;
    itx_scan_chunk(n, &lo, &hi);
    uint64_t a = 0, total;
    for (uint64_t i = lo; i < hi; i++) a += size[i];
    uint64_t e = itx_scan_wg(a, s, &total);
    for (uint64_t i = lo; i < hi; i++) {
        off[i] = e;
        e += size[i];
    }
    if (threadIdx.x == 0) off[n] = total;
}

// the blocks one behind the other: block b's size[b] bytes go to packed + dst_off[b] (k_size_scan's offsets), a workgroup per
// block. src_off: where block b lies in src; null: it lies at b * stride, and a size beyond the stride is cut to it.
static __global__ __launch_bounds__(256) void k_pack_blocks(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, uint32_t stride,
                                                            const uint32_t *__restrict__ size, const uint64_t *__restrict__ dst_off, uint8_t *__restrict__ packed)
{
    const uint64_t b = blockIdx.x;
    const uint8_t *from = src + (src_off ? src_off[b] : b * stride);
    uint8_t *dst = packed + dst_off[b];
    const uint32_t z = src_off || size[b] < stride ? size[b] : stride;
    for (uint32_t i = threadIdx.x; i < z; i += 256) dst[i] = from[i];
}

// where the lane's `len` bytes start inside the tile, and the tile's total: wave scan, then the waves' sums through LDS
// (s_w: TILE / 64 words; every lane calls, the barrier inside also orders whatever the caller put into LDS before)
template <uint32_t TILE>
__device__ __forceinline__ uint32_t itx_tile_offsets(uint32_t len, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t x = wave_incl_scan_u32(len, lane);
    if (lane == 63u) s_w[w] = x;
    __syncthreads();
    uint32_t woff = 0, t = 0;
    for (uint32_t k = 0; k < TILE / 64u; k++) {
        if (k < w) woff += s_w[k];
        t += s_w[k];
    }
    *total = t;
    return woff + (x - len);
}

// the staged window [win, win + LDS) of the output range [tb, te): full vectors where they lie inside the range
template <uint32_t TILE, uint32_t LDS>
__device__ __forceinline__ void itx_store_window(const uint4 *s_buf, uint8_t *__restrict__ out, unsigned long long win, unsigned long long tb, unsigned long long te)
{
    const uint8_t *s_bytes = reinterpret_cast<const uint8_t *>(s_buf);
    for (uint32_t v = threadIdx.x; v < LDS / 16u; v += TILE) {
        const unsigned long long ab = win + 16ull * v;
        if (ab >= te) break;
        if (ab >= tb && ab + 16ull <= te) {
            *reinterpret_cast<uint4 *>(out + ab) = s_buf[v];
        } else {
            for (uint32_t k = 0; k < 16u; k++)
                if (ab + k >= tb && ab + k < te) out[ab + k] = s_bytes[16u * v + k];
        }
    }
}

// the tile's range [tb, te) of `out`, the lane's piece at [mb, me) (empty: nothing to lay); s_buf: LDS bytes of the workgroup
template <uint32_t TILE, uint32_t LDS, class LAY>
__device__ __forceinline__ void itx_pack_tile(uint4 *s_buf, uint8_t *__restrict__ out, unsigned long long tb, unsigned long long te, unsigned long long mb,
                                              unsigned long long me, LAY lay)
{
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(s_buf);
    for (unsigned long long win = tb & ~15ull; win < te; win += LDS) {
        const unsigned long long a = mb > win ? mb : win, b = me < win + LDS ? me : win + LDS;
        if (a < b) lay(s_bytes + (uint32_t)(a - win), (uint32_t)(a - mb), (uint32_t)(b - mb));
        __syncthreads();
        itx_store_window<TILE, LDS>(s_buf, out, win, tb, te);
        __syncthreads();
    }
}
