// itx_samtext.hip — SAM text split and parsed on the device (iteres stat|filter -S): a chunk of text, cut by the host after a
// newline, becomes the per-record arrays the host reader fills otherwise (tid, pos, tmpend, mapq, flag5, mpos, isize) plus, per
// record, where in the text its line, its read name and its XA value lie, so that the host cuts a string out of ITS copy of the
// text only when a side channel wants one. The line rule is csrc/itx_samline.h; a line it calls hard makes the whole chunk the
// host's (warnings, the abort and the line numbers stay the reference's).
//
//   k_sam_count    tiles of 16 KiB: '\n' bytes and NUL bytes per tile
//   k_tile_scan2   (itx_textpack.h) the tiles' first line numbers
//   k_sam_starts   the same tiles again: newline number g at byte o writes line_start[g + 1] = o + 1; the number inside the tile
//                  from ballots and popcounts
//   k_sam_parse    a lane per line: a wave stages the contiguous bytes of its 64 lines in its own LDS window with 16-byte loads
//                  and the lanes parse out of LDS; a wave whose lines do not fit parses the same way out of global memory
//
// A text that arrives as BGZF (itx_samtext_parse_begin_bgzf) is inflated on the device by the decoder's two passes
// (itx_inflate_enqueue, csrc/itx_inflate.hip) into a buffer of the slot; the slot's text is put together from the previous
// chunk's tail and those bytes with device-to-device copies, so the four kernels above see a 16-byte-aligned start whatever
// the tail's length is. The host then has no copy of the text to cut strings out of: itx_samtext_strings gathers them,
//   k_sam_str_measure  a lane per record: the bytes its strings take (name + NUL, XA value + NUL), summed per tile of 256
//   k_tile_scan2       the tiles' places in the packed text
//   k_sam_str_write    a workgroup per tile: the tile's strings are one contiguous range of the output, staged in LDS and stored
//                      with 16-byte vectors (itx_textpack.h)
#include <string.h>

#include <string>
#include <vector>

#include "itx_common.h"
#include "itx_devbuf.h"
#include "itx_samline.h"
#include "itx_textpack.h"

#define SAM_TILE 16384u                 // bytes of text per workgroup of k_sam_count / k_sam_starts
#define SAM_TILE_WG 256u
#define SAM_MAX_CHUNK (256u << 20)      // k_tile_scan2 runs over at most 16 Ki tiles
#define SAM_WAVES 2u                    // waves per workgroup of k_sam_parse
#define SAM_WIN 24576u                  // LDS bytes per wave: 64 lines of 350 bytes (22400) and the 15 bytes before the first one
#define SAM_MIN_LINE 20u                // a line of fewer bytes (newline included) cannot hold 11 fields: lines beyond len / 20 + 2 prove a hard one

struct SamNames {                       // the @SQ names: open addressing over FNV-1a, entry = tid + 1 (0: empty)
    const uint32_t *tab;
    const uint32_t *off;                // name t = pool[off[t] .. off[t + 1])
    const uint8_t *pool;
    uint32_t mask;                      // slots - 1; 0 with tab == nullptr: no names at all
};

struct SamOut {
    int32_t *tid, *pos, *tmpend, *mpos, *isize, *nm;
    uint8_t *mapq, *flag5, *xa_mark;
    uint32_t *line_off, *qname_len, *xa_off, *xa_len;
};

// res[]: what a parse leaves for the host
enum { SAM_R_NHARD = 0, SAM_R_FIRST = 1, SAM_R_FLAGS = 2, SAM_R_LINES = 3, SAM_R_CONSUMED = 4, SAM_R_WORDS = 8 };

typedef const __attribute__((address_space(3))) uint8_t *sam_lds_ptr;

static inline uint32_t sam_fnv_host(const uint8_t *p, size_t n)
{
    uint32_t h = 2166136261u;
    for (size_t k = 0; k < n; k++) h = (h ^ p[k]) * 16777619u;
    return h;
}

template <class P>
__device__ __forceinline__ int64_t sam_lookup(const void *names, P p, uint32_t n)
{
    const SamNames *N = (const SamNames *)names;
    if (!N->tab) return -1;
    uint32_t h = 2166136261u;
    for (uint32_t k = 0; k < n; k++) h = (h ^ (uint32_t)p[k]) * 16777619u;
    for (uint32_t i = h & N->mask;; i = (i + 1u) & N->mask) {
        const uint32_t t = N->tab[i];
        if (!t) return -1;
        const uint32_t o = N->off[t - 1u];
        if (N->off[t] - o != n) continue;
        uint32_t k = 0;
        while (k < n && N->pool[o + k] == (uint8_t)p[k]) k++;
        if (k == n) return (int64_t)(t - 1u);
    }
}

ITX_SAMLINE_DEFINE(sam_line_lds, sam_lds_ptr, sam_lookup)
ITX_SAMLINE_DEFINE(sam_line_global, const uint8_t *, sam_lookup)

// bit b set: byte b of the vector equals c
__device__ __forceinline__ uint32_t sam_match4(uint32_t w, uint32_t c)
{
    const uint32_t x = w ^ (c * 0x01010101u);
    const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);        // 0x80 in every byte that is zero in x
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}
__device__ __forceinline__ uint32_t sam_match16(uint4 v, uint32_t c)
{
    return sam_match4(v.x, c) | sam_match4(v.y, c) << 4 | sam_match4(v.z, c) << 8 | sam_match4(v.w, c) << 12;
}

// vector j of thread t of a tile: byte offset of the vector in the text; the vectors of one j are contiguous over the threads
__device__ __forceinline__ uint32_t sam_vec_off(uint32_t tile, uint32_t j) { return tile * SAM_TILE + (j * SAM_TILE_WG + threadIdx.x) * 16u; }
__device__ __forceinline__ uint32_t sam_vec_valid(uint32_t off, uint32_t len) { return len - off >= 16u ? 0xffffu : (1u << (len - off)) - 1u; }

static __global__ __launch_bounds__(SAM_TILE_WG) void k_sam_count(const uint8_t *__restrict__ text, uint32_t len, unsigned long long *__restrict__ tile_sum)
{
    __shared__ uint32_t s_c[2][SAM_TILE_WG / 64u];
    uint32_t nl = 0, nul = 0;
#pragma unroll
    for (uint32_t j = 0; j < SAM_TILE / (16u * SAM_TILE_WG); j++) {
        const uint32_t off = sam_vec_off(blockIdx.x, j);
        if (off < len) {
            const uint4 v = *reinterpret_cast<const uint4 *>(text + off);
            const uint32_t ok = sam_vec_valid(off, len);
            nl += (uint32_t)__popc(sam_match16(v, '\n') & ok);
            nul += (uint32_t)__popc(sam_match16(v, 0u) & ok);
        }
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    nl = wave_incl_scan_u32(nl, lane);
    nul = wave_incl_scan_u32(nul, lane);
    if (lane == 63u) {
        s_c[0][w] = nl;
        s_c[1][w] = nul;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (uint32_t k = 0; k < SAM_TILE_WG / 64u; k++) {
            a += s_c[0][k];
            b += s_c[1][k];
        }
        tile_sum[2u * blockIdx.x] = a;
        tile_sum[2u * blockIdx.x + 1u] = b;
    }
}

// line_start[0 .. cap_lines]: entry g + 1 is written by newline number g (0-based over the whole text) while g + 1 <= cap_lines
static __global__ __launch_bounds__(SAM_TILE_WG) void k_sam_starts(const uint8_t *__restrict__ text, uint32_t len, const unsigned long long *__restrict__ tile_base,
                                                                    uint32_t *__restrict__ line_start, uint32_t cap_lines)
{
    constexpr uint32_t NJ = SAM_TILE / (16u * SAM_TILE_WG), NW = SAM_TILE_WG / 64u;
    __shared__ uint32_t s_seg[NJ * NW];                 // newlines per (j, wave): the segments of the tile in text order
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t m[NJ], pre[NJ];
#pragma unroll
    for (uint32_t j = 0; j < NJ; j++) {
        const uint32_t off = sam_vec_off(blockIdx.x, j);
        m[j] = 0;
        pre[j] = 0;
        if (off < len) m[j] = sam_match16(*reinterpret_cast<const uint4 *>(text + off), '\n') & sam_vec_valid(off, len);
        uint32_t tot = 0;
        if (__ballot(m[j] != 0u)) {
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++) {
                const unsigned long long B = __ballot((m[j] >> b) & 1u);
                pre[j] += (uint32_t)__popcll(B & below);          // newlines in the vectors of the lanes below
                tot += (uint32_t)__popcll(B);
            }
        }
        if (lane == 0) s_seg[j * NW + w] = tot;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = 0;
    const uint32_t base = (uint32_t)tile_base[2u * blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < NJ; j++) {
        if (!m[j]) continue;
        uint32_t g = base + pre[j];
        for (uint32_t k = 0; k < j * NW + w; k++) g += s_seg[k];
        const uint32_t off = sam_vec_off(blockIdx.x, j);
        uint32_t mm = m[j];
        while (mm) {
            const uint32_t b = (uint32_t)__ffs((int)mm) - 1u;
            mm &= mm - 1u;
            if (g + 1u <= cap_lines) line_start[g + 1u] = off + b + 1u;
            g++;
        }
    }
}

static __global__ __launch_bounds__(SAM_WAVES * 64u) void k_sam_parse(const uint8_t *__restrict__ text, uint32_t len, int final, const uint32_t *__restrict__ line_start,
                                                                       const unsigned long long *__restrict__ tot, uint32_t cap_lines, SamNames N, SamOut O,
                                                                       uint32_t *__restrict__ res)
{
    __shared__ uint4 s_win[SAM_WAVES][SAM_WIN / 16u];
    __shared__ uint32_t s_red[SAM_WAVES][4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long n_nl = tot[0];
    const bool over = n_nl >= cap_lines;                                  // as many newlines as the arrays hold lines: a hard chunk (itx_samtext_parse_end)
    const uint32_t n_term = over ? cap_lines : (uint32_t)n_nl;            // lines that end in a newline
    const uint32_t last_start = over ? len : line_start[n_term];
    const uint32_t n_lines = n_term + ((final && !over && last_start < len) ? 1u : 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        res[SAM_R_LINES] = n_lines;
        res[SAM_R_CONSUMED] = (final || over) ? len : last_start;
    }
    uint32_t n_hard = 0, first_hard = 0x7fffffffu, flags = 0;
    uint4 *win = s_win[w];
    const uint32_t n_groups = (n_lines + 63u) / 64u;
    for (uint32_t g = blockIdx.x * SAM_WAVES + w; g < n_groups; g += gridDim.x * SAM_WAVES) {
        const uint32_t i = g * 64u + lane;
        const bool act = i < n_lines;
        const uint32_t s = act ? line_start[i] : 0u;
        uint32_t e = act ? (i < n_term ? line_start[i + 1u] - 1u : len) : 0u;
        const uint32_t n_act = n_lines - g * 64u < 64u ? n_lines - g * 64u : 64u;
        const uint32_t b0 = (uint32_t)__shfl((int)s, 0, 64) & ~15u, b1 = (uint32_t)__shfl((int)e, (int)(n_act - 1u), 64);
        const bool in_lds = b1 - b0 <= SAM_WIN;                            // wave-uniform
        if (in_lds) {
            const uint4 *src = reinterpret_cast<const uint4 *>(text + b0);
            for (uint32_t v = lane; 16u * v < b1 - b0; v += 64u) win[v] = src[v];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        ItxSamRec r;
        uint32_t n = e - s;
        if (in_lds) {
            sam_lds_ptr p = (sam_lds_ptr)win + (s - b0);
            ITX_SAM_STRIP(p, n);
            if (act) sam_line_lds(p, n, &N, &r);
        } else {
            const uint8_t *p = text + s;
            ITX_SAM_STRIP(p, n);
            if (act) sam_line_global(p, n, &N, &r);
        }
        __builtin_amdgcn_wave_barrier();                                   // the window is rewritten by the next group
        if (!act) continue;
        O.tid[i] = r.tid;
        O.pos[i] = r.pos;
        O.tmpend[i] = r.tmpend;
        O.mapq[i] = r.mapq;
        O.flag5[i] = ITX_FLAG5(r.flag);
        O.mpos[i] = r.mpos;
        O.isize[i] = r.isize;
        O.nm[i] = r.nm;
        O.xa_mark[i] = r.has_xa;
        O.line_off[i] = s;
        O.qname_len[i] = r.qname_len;
        O.xa_off[i] = s + r.xa_off;
        O.xa_len[i] = r.xa_len;
        if (r.hard) {
            n_hard++;
            if (i < first_hard) first_hard = i;
        } else {
            flags |= (r.flag & 1u) | (r.has_xa ? 2u : 0u);
        }
    }
    // one reduction per wave, one atomic per workgroup and value
    const uint32_t wh = wave_incl_scan_u32(n_hard, lane);
    const int32_t wf = wave_min_i32((int32_t)first_hard);
    const uint32_t wfl = (__ballot(flags & 1u) ? 1u : 0u) | (__ballot(flags & 2u) ? 2u : 0u);
    if (lane == 63u) {
        s_red[w][0] = wh;
        s_red[w][1] = (uint32_t)wf;
        s_red[w][2] = wfl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0x7fffffffu, c = 0;
        for (uint32_t k = 0; k < SAM_WAVES; k++) {
            a += s_red[k][0];
            b = s_red[k][1] < b ? s_red[k][1] : b;
            c |= s_red[k][2];
        }
        if (a) {
            atomicAdd(&res[SAM_R_NHARD], a);
            atomicMin(&res[SAM_R_FIRST], b);
        }
        if (c) atomicOr(&res[SAM_R_FLAGS], c);
    }
}

// ---- the string gather ----------------------------------------------------------------------------------------------------------
#define SAM_STR_TILE 256u               // records per workgroup
#define SAM_STR_LDS 16384u              // bytes staged at a time: a tile of names (256 x 20-40 bytes) and its few XA values in one window
#define SAM_STR_NONE 0xffffffffu
#define SAM_STR_GUARD 16u               // bytes behind the packed text that travel with it (set before the write, nothing writes them)

// the piece of record i: its name and a NUL (want & 1), then its XA value and a NUL (want & 2, a record that carries XA).
// The strings are disjoint slices of a text of at most SAM_MAX_CHUNK bytes: a tile's sum, and every offset, fits 32 bits.
__device__ __forceinline__ uint32_t sam_str_len(const SamOut &O, uint32_t i, int want, uint32_t *ql1, uint32_t *xl1)
{
    *ql1 = (want & 1) ? O.qname_len[i] + 1u : 0u;
    *xl1 = ((want & 2) && O.xa_mark[i]) ? O.xa_len[i] + 1u : 0u;
    return *ql1 + *xl1;
}

static __global__ __launch_bounds__(SAM_STR_TILE) void k_sam_str_measure(SamOut O, uint32_t first, uint32_t n, int want, unsigned long long *__restrict__ tile_sum)
{
    __shared__ uint32_t s_w[SAM_STR_TILE / 64u];
    const uint32_t j = blockIdx.x * SAM_STR_TILE + threadIdx.x;
    uint32_t ql1 = 0, xl1 = 0, total = 0;
    const uint32_t len = j < n ? sam_str_len(O, first + j, want, &ql1, &xl1) : 0u;
    (void)itx_tile_offsets<SAM_STR_TILE>(len, s_w, &total);
    if (threadIdx.x == 0) {
        tile_sum[2u * blockIdx.x] = total;
        tile_sum[2u * blockIdx.x + 1u] = 0;
    }
}

static __global__ __launch_bounds__(SAM_STR_TILE) void k_sam_str_write(const uint8_t *__restrict__ text, SamOut O, uint32_t first, uint32_t n, int want,
                                                                        const unsigned long long *__restrict__ tile_base, uint8_t *__restrict__ out,
                                                                        uint32_t *__restrict__ qname_at, uint32_t *__restrict__ xa_at)
{
    __shared__ uint4 s_buf[SAM_STR_LDS / 16u];
    __shared__ uint32_t s_w[SAM_STR_TILE / 64u];
    const uint32_t j = blockIdx.x * SAM_STR_TILE + threadIdx.x;
    const bool valid = j < n;
    uint32_t ql1 = 0, xl1 = 0, total = 0;
    const uint32_t len = valid ? sam_str_len(O, first + j, want, &ql1, &xl1) : 0u;
    const uint32_t moff = itx_tile_offsets<SAM_STR_TILE>(len, s_w, &total);
    const unsigned long long tb = tile_base[2u * blockIdx.x], te = tb + total;
    const unsigned long long mb = tb + moff, me = mb + len;
    if (valid) {
        qname_at[j] = ql1 ? (uint32_t)mb : SAM_STR_NONE;
        xa_at[j] = xl1 ? (uint32_t)mb + ql1 : SAM_STR_NONE;
    }
    const uint8_t *qs = text + (ql1 ? O.line_off[first + j] : 0u), *xs = text + (xl1 ? O.xa_off[first + j] : 0u);
    itx_pack_tile<SAM_STR_TILE, SAM_STR_LDS>(s_buf, out, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) {
        // 20-60 bytes at any alignment: a byte loop, as in itx_names.hip
#pragma clang loop vectorize(disable)
        for (uint32_t k = from; k < to; k++) {
            uint8_t c;
            if (k < ql1) c = k + 1u < ql1 ? qs[k] : (uint8_t)0;
            else c = k - ql1 + 1u < xl1 ? xs[k - ql1] : (uint8_t)0;
            dst[k - from] = c;
        }
    });
}

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------
struct SamSlot {
    ItxBuf d_text, d_line_start;
    ItxBuf d_rec;                          // one allocation behind the arrays of `out`
    SamOut out = {};
    ItxBuf d_tot;                          // newlines, NUL bytes
    ItxBuf d_res;
    ItxPin h_res;                          // SAM_R_WORDS words, then the two totals
    ItxEvent ev_copy, ev_k0, ev_k1, ev_done;
    int state = 0;                         // 0 idle, 1 begun, 2 ended: its records can be fetched
    size_t len = 0;
    uint64_t n_rec = 0;
    // a chunk begun by parse_begin_bgzf: its compressed bytes, block list and status bytes, and what they inflate to
    int bgzf = 0;
    ItxBuf d_comp, d_infl, d_status, d_blk;
    ItxPin h_status, h_blk;
    size_t n_blk = 0, carry_len = 0;
    ItxEvent ev_d0, ev_d1;
    double inflate_ms = 0;
};

struct itx_samtext {
    int device = 0;
    size_t max_chunk = 0;
    uint32_t cap_lines = 0;
    unsigned n_blocks = 0;
    SamNames names = {};
    ItxBuf d_tab, d_off, d_pool;
    ItxBuf d_tile_sum, d_tile_base;
    hipStream_t st = nullptr, st_copy = nullptr;
    SamSlot slot[2];
    // BGZF: the decoder's scratch (one chunk's passes at a time: they all run on st), the slot of the stream's previous chunk (-1:
    // the next chunk has no carry), the last text put together on st (a copy into a slot's text on st_copy waits for it)
    ItxBuf d_scr, d_meta;
    int bgzf_prev = -1;
    ItxEvent ev_asm;
    bool asm_recorded = false;
    // the string gather: a stream and buffers of its own, so that it does not queue behind the other slot's parse
    hipStream_t st_str = nullptr;
    ItxEvent ev_s[4];
    ItxBuf d_str_sum, d_str_base, d_str_tot;
    ItxPin h_str_tot;
    ItxBuf d_at, d_str;                    // qname_at[n], then xa_at[n]
    ItxPin h_at, h_str;
};

#define SAM_RC(call)                          \
    do {                                      \
        const int rc__ = (call);              \
        if (rc__ != ITX_OK) return rc__;      \
    } while (0)

// room for `need` elements of `size` bytes, nothing kept (the drop's hipFree waits for whatever still uses the old one)
template <bool PINNED> static int sam_grow(ItxMem<PINNED> &b, size_t need, size_t size)
{
    return need * size <= b.cap ? ITX_OK : itx_mem_need("itx_samtext", b, (need + need / 4 + 64) * size);
}

extern "C" void itx_samtext_destroy(itx_samtext *x)
{
    if (!x) return;
    (void)hipSetDevice(x->device);
    for (hipStream_t st : {x->st, x->st_copy, x->st_str})
        if (st) (void)hipStreamSynchronize(st);
    for (hipStream_t st : {x->st, x->st_copy, x->st_str})
        if (st) (void)hipStreamDestroy(st);
    delete x;
}

static inline size_t sam_up256(size_t n) { return (n + 255) & ~(size_t)255; }

// fills the object; on a non-zero return the caller destroys what there is of it
static int samtext_create(itx_samtext *x, int device, const char *name_bytes, const uint64_t *name_off, int n_targets, size_t max_chunk)
{
    const char *const who = "itx_samtext_create";
    x->device = device;
    ITX_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ITX_HIP(hipGetDeviceProperties(&prop, device));
    x->n_blocks = (unsigned)prop.multiProcessorCount * 3u;                 // three workgroups of 48 KiB LDS per CU
    x->max_chunk = max_chunk;
    x->cap_lines = (uint32_t)(max_chunk / SAM_MIN_LINE + 2);
    if (n_targets > 0) {
        uint32_t slots = 2;
        while (slots < 2u * (uint32_t)n_targets + 1u) slots <<= 1;
        std::vector<uint32_t> tab(slots, 0u), off((size_t)n_targets + 1);
        const uint8_t *nb = (const uint8_t *)name_bytes;
        for (int t = 0; t <= n_targets; t++) off[(size_t)t] = (uint32_t)(name_off[t] - name_off[0]);
        for (int t = 0; t < n_targets; t++) {
            const uint8_t *p = nb + name_off[t];
            const size_t n = (size_t)(name_off[t + 1] - name_off[t]);
            uint32_t i = sam_fnv_host(p, n) & (slots - 1u);
            bool dup = false;
            for (; tab[i]; i = (i + 1u) & (slots - 1u)) {
                const uint32_t u = tab[i] - 1u;
                if (name_off[u + 1] - name_off[u] == n && memcmp(nb + name_off[u], p, n) == 0) {
                    dup = true;                                            // the first occurrence wins a lookup
                    break;
                }
            }
            if (!dup) tab[i] = (uint32_t)t + 1u;
        }
        const size_t pool = (size_t)(name_off[n_targets] - name_off[0]);
        SAM_RC(itx_buf_need(who, x->d_tab, 4 * tab.size()));
        SAM_RC(itx_buf_need(who, x->d_off, 4 * off.size()));
        SAM_RC(itx_buf_need(who, x->d_pool, pool + 16));
        ITX_HIP(hipMemcpy(x->d_tab.p, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice));
        ITX_HIP(hipMemcpy(x->d_off.p, off.data(), 4 * off.size(), hipMemcpyHostToDevice));
        if (pool) ITX_HIP(hipMemcpy(x->d_pool.p, nb + name_off[0], pool, hipMemcpyHostToDevice));
        x->names.tab = x->d_tab.as<uint32_t>();
        x->names.off = x->d_off.as<uint32_t>();
        x->names.pool = x->d_pool.as<uint8_t>();
        x->names.mask = slots - 1u;
    }
    const size_t nt = (max_chunk + SAM_TILE - 1) / SAM_TILE + 1;
    SAM_RC(itx_buf_need(who, x->d_tile_sum, 16 * nt));
    SAM_RC(itx_buf_need(who, x->d_tile_base, 16 * nt));
    ITX_HIP(hipStreamCreateWithFlags(&x->st, hipStreamNonBlocking));
    ITX_HIP(hipStreamCreateWithFlags(&x->st_copy, hipStreamNonBlocking));
    const size_t c = (size_t)x->cap_lines, a4 = sam_up256(4 * c), a1 = sam_up256(c);
    for (auto &s : x->slot) {
        SAM_RC(itx_buf_need(who, s.d_text, sam_up256(max_chunk) + 256));
        SAM_RC(itx_buf_need(who, s.d_line_start, 4 * (c + 2)));
        SAM_RC(itx_buf_need(who, s.d_rec, 10 * a4 + 3 * a1));
        uint8_t *p = s.d_rec.as<uint8_t>();
        int32_t **i32s[6] = {&s.out.tid, &s.out.pos, &s.out.tmpend, &s.out.mpos, &s.out.isize, &s.out.nm};
        for (auto pp : i32s) {
            *pp = (int32_t *)p;
            p += a4;
        }
        uint32_t **u32s[4] = {&s.out.line_off, &s.out.qname_len, &s.out.xa_off, &s.out.xa_len};
        for (auto pp : u32s) {
            *pp = (uint32_t *)p;
            p += a4;
        }
        uint8_t **u8s[3] = {&s.out.mapq, &s.out.flag5, &s.out.xa_mark};
        for (auto pp : u8s) {
            *pp = p;
            p += a1;
        }
        SAM_RC(itx_buf_need(who, s.d_tot, 16));
        SAM_RC(itx_buf_need(who, s.d_res, 4 * SAM_R_WORDS));
        SAM_RC(itx_pin_need(who, s.h_res, 4 * SAM_R_WORDS + 16));
        for (ItxEvent *e : {&s.ev_copy, &s.ev_k0, &s.ev_k1, &s.ev_done, &s.ev_d0, &s.ev_d1}) SAM_RC(itx_event_make(*e));
    }
    ITX_HIP(hipStreamCreateWithFlags(&x->st_str, hipStreamNonBlocking));
    SAM_RC(itx_event_make(x->ev_asm));
    for (auto &e : x->ev_s) SAM_RC(itx_event_make(e));
    SAM_RC(itx_buf_need(who, x->d_str_tot, 16));
    SAM_RC(itx_pin_need(who, x->h_str_tot, 16));
    return ITX_OK;
}

extern "C" int itx_samtext_create(int device, const char *name_bytes, const uint64_t *name_off, int n_targets, size_t max_chunk_bytes, itx_samtext **out)
{
    if (!out || device < 0 || n_targets < 0 || (n_targets && (!name_bytes || !name_off)) || max_chunk_bytes == 0) {
        itx_set_error("itx_samtext_create: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    if (max_chunk_bytes > SAM_MAX_CHUNK || (n_targets && name_off[n_targets] - name_off[0] > 0xffffff00ull)) {
        itx_set_error("itx_samtext_create: chunks of more than %u bytes or names of 4 GiB are not encoded", SAM_MAX_CHUNK);
        return ITX_E_LIMIT;
    }
    for (int t = 0; t < n_targets; t++)
        if (name_off[t + 1] < name_off[t]) {
            itx_set_error("itx_samtext_create: name offsets do not ascend");
            return ITX_E_ARG;
        }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) {
        itx_set_error("itx_samtext_create: no device %d", device);
        return ITX_E_NO_DEVICE;
    }
    itx_samtext *x = new itx_samtext();
    const int rc = samtext_create(x, device, name_bytes, name_off, n_targets, max_chunk_bytes);
    if (rc) {
        itx_samtext_destroy(x);
        return rc;
    }
    *out = x;
    return ITX_OK;
}

static int sam_enqueue_parse(itx_samtext *x, SamSlot &s, size_t len, int final);

extern "C" int itx_samtext_parse_begin(itx_samtext *x, int slot, const void *text, size_t len, int final)
{
    if (!x || slot < 0 || slot > 1 || (len && !text)) {
        itx_set_error("itx_samtext_parse_begin: bad argument");
        return ITX_E_ARG;
    }
    if (len > x->max_chunk) {
        itx_set_error("itx_samtext_parse_begin: %zu bytes exceed the chunk size the object was made for (%zu)", len, x->max_chunk);
        return ITX_E_LIMIT;
    }
    SamSlot &s = x->slot[slot];
    if (s.state == 1) {
        itx_set_error("itx_samtext_parse_begin: the slot's parse has not been ended");
        return ITX_E_STATE;
    }
    ITX_HIP(hipSetDevice(x->device));
    s.state = 0;
    s.len = len;
    s.bgzf = 0;
    if (x->bgzf_prev == slot) x->bgzf_prev = -1;                           // the tail a BGZF chunk left here is overwritten
    if (x->asm_recorded) ITX_HIP(hipStreamWaitEvent(x->st_copy, x->ev_asm, 0));       // ... but not before the chunk that took it has it
    if (len) ITX_HIP(hipMemcpyAsync(s.d_text.as<uint8_t>(), text, len, hipMemcpyHostToDevice, x->st_copy));
    ITX_HIP(hipEventRecord(s.ev_copy, x->st_copy));
    ITX_HIP(hipStreamWaitEvent(x->st, s.ev_copy, 0));
    const int rc = sam_enqueue_parse(x, s, len, final);
    if (rc == ITX_OK) s.state = 1;
    return rc;
}

// the four kernels over the slot's text[0 .. len) and the copies of what they leave, on x->st
static int sam_enqueue_parse(itx_samtext *x, SamSlot &s, size_t len, int final)
{
    const uint8_t *const d_text = s.d_text.as<uint8_t>();
    uint32_t *const d_res = s.d_res.as<uint32_t>(), *const h_res = s.h_res.as<uint32_t>(), *const line_start = s.d_line_start.as<uint32_t>();
    unsigned long long *const d_tot = s.d_tot.as<unsigned long long>(), *const tile_sum = x->d_tile_sum.as<unsigned long long>(),
                             *const tile_base = x->d_tile_base.as<unsigned long long>();
    ITX_HIP(hipEventRecord(s.ev_k0, x->st));
    ITX_HIP(hipMemsetAsync(d_res, 0, 4 * SAM_R_WORDS, x->st));
    ITX_HIP(hipMemsetAsync(d_res + SAM_R_FIRST, 0xff, 4, x->st));
    ITX_HIP(hipMemsetAsync(d_tot, 0, 16, x->st));
    const uint32_t nt = (uint32_t)((len + SAM_TILE - 1) / SAM_TILE);
    if (nt) {
        hipLaunchKernelGGL(k_sam_count, dim3(nt), dim3(SAM_TILE_WG), 0, x->st, d_text, (uint32_t)len, tile_sum);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, x->st, tile_sum, nt, tile_base, d_tot);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_sam_starts, dim3(nt), dim3(SAM_TILE_WG), 0, x->st, d_text, (uint32_t)len, tile_base, line_start, x->cap_lines);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_sam_parse, dim3(x->n_blocks), dim3(SAM_WAVES * 64u), 0, x->st, d_text, (uint32_t)len, final ? 1 : 0, line_start, d_tot, x->cap_lines,
                           x->names, s.out, d_res);
        ITX_HIP(hipGetLastError());
    }
    ITX_HIP(hipEventRecord(s.ev_k1, x->st));
    ITX_HIP(hipMemcpyAsync(h_res, d_res, 4 * SAM_R_WORDS, hipMemcpyDeviceToHost, x->st));
    ITX_HIP(hipMemcpyAsync(h_res + SAM_R_WORDS, d_tot, 16, hipMemcpyDeviceToHost, x->st));
    ITX_HIP(hipEventRecord(s.ev_done, x->st));
    return ITX_OK;
}

// members of the slot's chunk whose status is not 0 (valid once ev_done has passed)
static size_t sam_count_bad(const SamSlot &s, size_t *first)
{
    size_t n = 0;
    for (size_t i = 0; i < s.n_blk; i++)
        if (s.h_status.as<uint8_t>()[i]) {
            if (!n) *first = i;
            n++;
        }
    return n;
}

extern "C" int itx_samtext_parse_begin_bgzf(itx_samtext *x, int slot, const void *comp, size_t comp_len, const itx_bgzf_block *blk, size_t n_blk, size_t skip,
                                            int final)
{
    if (!x || slot < 0 || slot > 1 || !comp || !blk) {
        itx_set_error("itx_samtext_parse_begin_bgzf: bad argument");
        return ITX_E_ARG;
    }
    if (comp_len > 0xfffffff0u || n_blk > 0x7fffffffu) {
        itx_set_error("itx_samtext_parse_begin_bgzf: %zu bytes in %zu members are more than the decoder encodes", comp_len, n_blk);
        return ITX_E_LIMIT;
    }
    size_t total = 0;                                                      // what the decoder assumes about every member (itx_inflate_bgzf)
    for (size_t i = 0; i < n_blk; i++) {
        const itx_bgzf_block &b = blk[i];
        if ((size_t)b.coff + b.csize > comp_len || b.csize < 26u || b.uoff != total || b.usize > 65536u) {
            itx_set_error("itx_samtext_parse_begin_bgzf: block %zu does not fit its buffers", i);
            return ITX_E_ARG;
        }
        total += b.usize;
    }
    if (total > x->max_chunk + 65536u) {
        itx_set_error("itx_samtext_parse_begin_bgzf: the members inflate to %zu bytes, the object was made for %zu + 64 KiB", total, x->max_chunk);
        return ITX_E_LIMIT;
    }
    SamSlot &s = x->slot[slot];
    if (s.state == 1) {
        itx_set_error("itx_samtext_parse_begin_bgzf: the slot's parse has not been ended");
        return ITX_E_STATE;
    }
    size_t unused = 0;
    int prev = x->bgzf_prev;
    if (prev == slot) {                                                    // (ended: its status bytes are here)
        if (sam_count_bad(s, &unused) == 0) {
            itx_set_error("itx_samtext_parse_begin_bgzf: the stream's previous chunk lies in this slot");
            return ITX_E_STATE;
        }
        prev = x->bgzf_prev = -1;
    }
    ITX_HIP(hipSetDevice(x->device));
    SAM_RC(sam_grow(s.d_comp, comp_len + 64, 1));
    SAM_RC(sam_grow(s.d_infl, x->max_chunk + 65536u + 64, 1));
    SAM_RC(sam_grow(s.d_status, n_blk + 1, 1));
    SAM_RC(sam_grow(s.h_blk, n_blk + 1, sizeof *blk));
    SAM_RC(sam_grow(s.h_status, n_blk + 1, 1));
    SAM_RC(sam_grow(s.d_blk, n_blk + 1, sizeof *blk));
    SAM_RC(sam_grow(x->d_scr, itx_inflate_scratch_bytes(n_blk), 1));
    SAM_RC(sam_grow(x->d_meta, 3 * n_blk, 4));
    itx_bgzf_block *const h_blk = s.h_blk.as<itx_bgzf_block>(), *const d_blk = s.d_blk.as<itx_bgzf_block>();
    uint8_t *const h_status = s.h_status.as<uint8_t>(), *const d_status = s.d_status.as<uint8_t>();
    uint8_t *const d_comp = s.d_comp.as<uint8_t>(), *const d_infl = s.d_infl.as<uint8_t>(), *const d_text = s.d_text.as<uint8_t>();
    s.state = 0;
    s.n_blk = 0;
    // 1. the compressed bytes cross the link on the copy stream, both passes of the decoder run behind them
    memcpy(h_blk, blk, n_blk * sizeof *blk);
    memset(h_status, 0xff, n_blk);
    if (n_blk) ITX_HIP(hipMemcpyAsync(d_blk, h_blk, n_blk * sizeof *blk, hipMemcpyHostToDevice, x->st_copy));
    if (comp_len) ITX_HIP(hipMemcpyAsync(d_comp, comp, comp_len, hipMemcpyHostToDevice, x->st_copy));
    ITX_HIP(hipEventRecord(s.ev_copy, x->st_copy));
    ITX_HIP(hipStreamWaitEvent(x->st, s.ev_copy, 0));
    ITX_HIP(hipEventRecord(s.ev_d0, x->st));
    SAM_RC(itx_inflate_enqueue(x->st, d_comp, d_blk, (uint32_t)n_blk, d_infl, d_status, x->d_scr.as<uint8_t>(), x->d_meta.as<uint32_t>()));
    ITX_HIP(hipEventRecord(s.ev_d1, x->st));
    if (n_blk) ITX_HIP(hipMemcpyAsync(h_status, d_status, n_blk, hipMemcpyDeviceToHost, x->st));
    // 2. where the previous chunk's parse stopped: its tail is this text's front
    size_t carry = 0, carry_at = 0;
    if (prev >= 0) {
        const SamSlot &p = x->slot[prev];
        ITX_HIP(hipEventSynchronize(p.ev_done));
        carry_at = p.len ? p.h_res.as<uint32_t>()[SAM_R_CONSUMED] : 0;
        carry = sam_count_bad(p, &unused) || carry_at > p.len ? 0 : p.len - carry_at;
    }
    x->bgzf_prev = -1;
    const size_t from = skip < total ? skip : total, len = carry + (total - from);
    if (len > x->max_chunk) {
        ITX_HIP(hipStreamSynchronize(x->st_copy));                         // comp is the caller's again
        itx_set_error("itx_samtext_parse_begin_bgzf: a text of %zu bytes (%zu of them the chunk before's tail) exceeds the chunk size the object was made for (%zu)",
                      len, carry, x->max_chunk);
        return ITX_E_LIMIT;
    }
    // 3. the text, put together on the device
    if (carry) ITX_HIP(hipMemcpyAsync(d_text, x->slot[prev].d_text.as<uint8_t>() + carry_at, carry, hipMemcpyDeviceToDevice, x->st));
    if (total > from) ITX_HIP(hipMemcpyAsync(d_text + carry, d_infl + from, total - from, hipMemcpyDeviceToDevice, x->st));
    ITX_HIP(hipEventRecord(x->ev_asm, x->st));
    x->asm_recorded = true;
    // 4. the parse
    s.len = len;
    s.bgzf = 1;
    s.n_blk = n_blk;
    s.carry_len = carry;
    SAM_RC(sam_enqueue_parse(x, s, len, final));
    s.state = 1;
    if (!final) x->bgzf_prev = slot;
    return ITX_OK;
}

extern "C" int itx_samtext_parse_end(itx_samtext *x, int slot, itx_samtext_result *res)
{
    if (!x || slot < 0 || slot > 1 || !res) {
        itx_set_error("itx_samtext_parse_end: bad argument");
        return ITX_E_ARG;
    }
    SamSlot &s = x->slot[slot];
    if (s.state != 1) {
        itx_set_error("itx_samtext_parse_end: no parse has been begun in the slot");
        return ITX_E_STATE;
    }
    ITX_HIP(hipSetDevice(x->device));
    ITX_HIP(hipEventSynchronize(s.ev_done));
    const uint32_t *const h_res = s.h_res.as<uint32_t>();
    float ms = 0;
    ITX_HIP(hipEventElapsedTime(&ms, s.ev_k0, s.ev_k1));
    unsigned long long tot[2];
    memcpy(tot, h_res + SAM_R_WORDS, 16);
    memset(res, 0, sizeof *res);
    res->n_lines = h_res[SAM_R_LINES];
    res->consumed = s.len ? h_res[SAM_R_CONSUMED] : 0;
    res->n_hard = h_res[SAM_R_NHARD];
    res->first_hard_line = h_res[SAM_R_FIRST] >= 0x7fffffffu ? 0 : h_res[SAM_R_FIRST];
    if (tot[0] >= x->cap_lines) {                  // as many lines as the arrays hold, or more: one of them is too short for 11 fields
        if (!res->n_hard) res->first_hard_line = x->cap_lines;
        res->n_hard++;
    }
    res->flags = (int)(h_res[SAM_R_FLAGS] | (tot[1] ? ITX_SAMTEXT_NUL : 0));
    res->n_rec = res->n_hard ? 0 : res->n_lines;
    res->kernel_ms = ms;
    if (s.bgzf) {
        size_t first = 0;
        if (sam_count_bad(s, &first)) res->n_rec = 0;                      // the text is not the file's: nothing of it is handed out
        float dms = 0;
        ITX_HIP(hipEventElapsedTime(&dms, s.ev_d0, s.ev_d1));
        s.inflate_ms = dms;
    }
    s.n_rec = res->n_rec;
    s.state = 2;
    return ITX_OK;
}

extern "C" int itx_samtext_bgzf_info(itx_samtext *x, int slot, itx_samtext_bgzf_info_t *out)
{
    if (!x || slot < 0 || slot > 1 || !out) {
        itx_set_error("itx_samtext_bgzf_info: bad argument");
        return ITX_E_ARG;
    }
    const SamSlot &s = x->slot[slot];
    if (s.state != 2 || !s.bgzf) {
        itx_set_error("itx_samtext_bgzf_info: the slot holds no parsed BGZF chunk");
        return ITX_E_STATE;
    }
    memset(out, 0, sizeof *out);
    size_t first = 0;
    const size_t consumed = s.len ? s.h_res.as<uint32_t>()[SAM_R_CONSUMED] : 0;
    out->text_len = s.len;
    out->carry_len = s.carry_len;
    out->tail_len = s.len - consumed;
    out->n_bad = sam_count_bad(s, &first);
    out->first_bad = first;
    out->inflate_ms = s.inflate_ms;
    return ITX_OK;
}

extern "C" int itx_samtext_text(itx_samtext *x, int slot, size_t off, void *dst, size_t len)
{
    if (!x || slot < 0 || slot > 1 || (len && !dst)) {
        itx_set_error("itx_samtext_text: bad argument");
        return ITX_E_ARG;
    }
    const SamSlot &s = x->slot[slot];
    if (s.state != 2) {
        itx_set_error("itx_samtext_text: the slot holds no parsed chunk");
        return ITX_E_STATE;
    }
    if (off > s.len || len > s.len - off) {
        itx_set_error("itx_samtext_text: bytes %zu + %zu of %zu", off, len, s.len);
        return ITX_E_ARG;
    }
    if (!len) return ITX_OK;
    ITX_HIP(hipSetDevice(x->device));
    ITX_HIP(hipMemcpyAsync(dst, s.d_text.as<uint8_t>() + off, len, hipMemcpyDeviceToHost, x->st_str));
    ITX_HIP(hipStreamSynchronize(x->st_str));
    return ITX_OK;
}

extern "C" int itx_samtext_strings(itx_samtext *x, int slot, size_t first, size_t n, int want, itx_samtext_strings_out *out)
{
    if (!x || slot < 0 || slot > 1 || !out || want < 1 || want > 3) {
        itx_set_error("itx_samtext_strings: bad argument");
        return ITX_E_ARG;
    }
    const SamSlot &s = x->slot[slot];
    if (s.state != 2) {
        itx_set_error("itx_samtext_strings: the slot holds no parsed chunk");
        return ITX_E_STATE;
    }
    if (first > s.n_rec || n > s.n_rec - first) {
        itx_set_error("itx_samtext_strings: records %zu + %zu of %llu", first, n, (unsigned long long)s.n_rec);
        return ITX_E_ARG;
    }
    memset(out, 0, sizeof *out);
    if (!n) return ITX_OK;
    ITX_HIP(hipSetDevice(x->device));
    const uint32_t nt = (uint32_t)((n + SAM_STR_TILE - 1) / SAM_STR_TILE);
    SAM_RC(sam_grow(x->d_str_sum, 2 * (size_t)nt, 8));
    SAM_RC(sam_grow(x->d_str_base, 2 * (size_t)nt, 8));
    SAM_RC(sam_grow(x->d_at, 2 * n, 4));
    SAM_RC(sam_grow(x->h_at, 2 * n, 4));
    unsigned long long *const d_sum = x->d_str_sum.as<unsigned long long>(), *const d_base = x->d_str_base.as<unsigned long long>(),
                             *const d_tot = x->d_str_tot.as<unsigned long long>(), *const h_tot = x->h_str_tot.as<unsigned long long>();
    uint32_t *const d_at = x->d_at.as<uint32_t>(), *const h_at = x->h_at.as<uint32_t>();
    hipStream_t st = x->st_str;
    ITX_HIP(hipEventRecord(x->ev_s[0], st));
    hipLaunchKernelGGL(k_sam_str_measure, dim3(nt), dim3(SAM_STR_TILE), 0, st, s.out, (uint32_t)first, (uint32_t)n, want, d_sum);
    ITX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, d_sum, nt, d_base, d_tot);
    ITX_HIP(hipGetLastError());
    ITX_HIP(hipEventRecord(x->ev_s[1], st));
    ITX_HIP(hipMemcpyAsync(h_tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    ITX_HIP(hipStreamSynchronize(st));                                     // the total is all the host waits for before the write
    const size_t total = (size_t)h_tot[0];
    if (total > s.len + n) {                                               // disjoint slices of the text and a NUL each: cannot be more
        itx_set_error("itx_samtext_strings: %zu bytes of strings out of a text of %zu", total, s.len);
        return ITX_E_STATE;
    }
    SAM_RC(sam_grow(x->d_str, total + SAM_STR_GUARD + 16, 1));
    SAM_RC(sam_grow(x->h_str, total + SAM_STR_GUARD, 1));
    ITX_HIP(hipMemsetAsync(x->d_str.as<uint8_t>() + total, 0xa5, SAM_STR_GUARD, st));
    ITX_HIP(hipEventRecord(x->ev_s[2], st));
    hipLaunchKernelGGL(k_sam_str_write, dim3(nt), dim3(SAM_STR_TILE), 0, st, s.d_text.as<uint8_t>(), s.out, (uint32_t)first, (uint32_t)n, want, d_base,
                       x->d_str.as<uint8_t>(), d_at, d_at + n);
    ITX_HIP(hipGetLastError());
    ITX_HIP(hipEventRecord(x->ev_s[3], st));
    ITX_HIP(hipMemcpyAsync(x->h_str.as<uint8_t>(), x->d_str.as<uint8_t>(), total + SAM_STR_GUARD, hipMemcpyDeviceToHost, st));
    ITX_HIP(hipMemcpyAsync(h_at, d_at, 8 * n, hipMemcpyDeviceToHost, st));
    ITX_HIP(hipStreamSynchronize(st));
    float a = 0, b = 0;
    ITX_HIP(hipEventElapsedTime(&a, x->ev_s[0], x->ev_s[1]));
    ITX_HIP(hipEventElapsedTime(&b, x->ev_s[2], x->ev_s[3]));
    out->text = x->h_str.as<const char>();
    out->text_len = total;
    out->qname_at = h_at;
    out->xa_at = h_at + n;
    out->kernel_ms = (double)a + (double)b;
    return ITX_OK;
}

extern "C" int itx_samtext_fetch(itx_samtext *x, int slot, size_t first, size_t n, const itx_staging *dst, size_t dst_at, uint32_t *line_off, uint32_t *qname_len,
                                 uint32_t *xa_off, uint32_t *xa_len, int32_t *nm, uint8_t *xa_mark)
{
    if (!x || slot < 0 || slot > 1 || !dst || !dst->tid || !dst->pos || !dst->tmpend || !dst->mapq || !dst->flag5 || dst_at > dst->capacity ||
        n > dst->capacity - dst_at) {
        itx_set_error("itx_samtext_fetch: bad argument");
        return ITX_E_ARG;
    }
    SamSlot &s = x->slot[slot];
    if (s.state != 2) {
        itx_set_error("itx_samtext_fetch: the slot holds no parsed chunk");
        return ITX_E_STATE;
    }
    if (first > s.n_rec || n > s.n_rec - first) {
        itx_set_error("itx_samtext_fetch: records %zu + %zu of %llu", first, n, (unsigned long long)s.n_rec);
        return ITX_E_ARG;
    }
    if (!n) return ITX_OK;
    ITX_HIP(hipSetDevice(x->device));
    const SamOut &o = s.out;
    struct {
        void *to;
        const void *from;
        size_t size;
    } c[13] = {{dst->tid ? dst->tid + dst_at : nullptr, o.tid + first, 4}, {dst->pos + dst_at, o.pos + first, 4}, {dst->tmpend + dst_at, o.tmpend + first, 4},
               {dst->mapq + dst_at, o.mapq + first, 1}, {dst->flag5 + dst_at, o.flag5 + first, 1},
               {dst->mpos ? dst->mpos + dst_at : nullptr, o.mpos + first, 4}, {dst->isize ? dst->isize + dst_at : nullptr, o.isize + first, 4},
               {line_off, o.line_off + first, 4}, {qname_len, o.qname_len + first, 4}, {xa_off, o.xa_off + first, 4}, {xa_len, o.xa_len + first, 4},
               {nm, o.nm + first, 4}, {xa_mark, o.xa_mark + first, 1}};
    for (auto &k : c)
        if (k.to) ITX_HIP(hipMemcpyAsync(k.to, k.from, k.size * n, hipMemcpyDeviceToHost, x->st_copy));
    ITX_HIP(hipStreamSynchronize(x->st_copy));
    return ITX_OK;
}
