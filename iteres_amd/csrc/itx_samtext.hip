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
#include <string.h>

#include <string>
#include <vector>

#include "itx_common.h"
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

// ---- the C ABI ----------------------------------------------------------------------------------------------------------------
struct SamSlot {
    uint8_t *d_text = nullptr;
    uint32_t *d_line_start = nullptr;
    void *d_rec = nullptr;                 // one allocation behind the arrays of `out`
    SamOut out = {};
    unsigned long long *d_tot = nullptr;   // newlines, NUL bytes
    uint32_t *d_res = nullptr;
    uint32_t *h_res = nullptr;             // page-locked: SAM_R_WORDS words, then the two totals
    hipEvent_t ev_copy = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_done = nullptr;
    int state = 0;                         // 0 idle, 1 begun, 2 ended: its records can be fetched
    size_t len = 0;
    uint64_t n_rec = 0;
};

struct itx_samtext {
    int device = 0;
    size_t max_chunk = 0;
    uint32_t cap_lines = 0;
    unsigned n_blocks = 0;
    SamNames names = {};
    void *d_tab = nullptr, *d_off = nullptr, *d_pool = nullptr;
    unsigned long long *d_tile_sum = nullptr, *d_tile_base = nullptr;
    hipStream_t st = nullptr, st_copy = nullptr;
    SamSlot slot[2];
};

extern "C" void itx_samtext_destroy(itx_samtext *x)
{
    if (!x) return;
    (void)hipSetDevice(x->device);
    if (x->st) (void)hipStreamSynchronize(x->st);
    if (x->st_copy) (void)hipStreamSynchronize(x->st_copy);
    for (auto &s : x->slot) {
        (void)hipFree(s.d_text);
        (void)hipFree(s.d_line_start);
        (void)hipFree(s.d_rec);
        (void)hipFree(s.d_tot);
        (void)hipFree(s.d_res);
        if (s.h_res) (void)hipHostFree(s.h_res);
        hipEvent_t *ev[4] = {&s.ev_copy, &s.ev_k0, &s.ev_k1, &s.ev_done};
        for (auto e : ev)
            if (*e) (void)hipEventDestroy(*e);
    }
    (void)hipFree(x->d_tab);
    (void)hipFree(x->d_off);
    (void)hipFree(x->d_pool);
    (void)hipFree(x->d_tile_sum);
    (void)hipFree(x->d_tile_base);
    if (x->st) (void)hipStreamDestroy(x->st);
    if (x->st_copy) (void)hipStreamDestroy(x->st_copy);
    delete x;
}

static inline size_t sam_up256(size_t n) { return (n + 255) & ~(size_t)255; }

// fills the object; on a non-zero return the caller destroys what there is of it
static int samtext_create(itx_samtext *x, int device, const char *name_bytes, const uint64_t *name_off, int n_targets, size_t max_chunk)
{
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
        ITX_HIP(hipMalloc(&x->d_tab, 4 * tab.size()));
        ITX_HIP(hipMalloc(&x->d_off, 4 * off.size()));
        ITX_HIP(hipMalloc(&x->d_pool, pool + 16));
        ITX_HIP(hipMemcpy(x->d_tab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice));
        ITX_HIP(hipMemcpy(x->d_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice));
        if (pool) ITX_HIP(hipMemcpy(x->d_pool, nb + name_off[0], pool, hipMemcpyHostToDevice));
        x->names.tab = (const uint32_t *)x->d_tab;
        x->names.off = (const uint32_t *)x->d_off;
        x->names.pool = (const uint8_t *)x->d_pool;
        x->names.mask = slots - 1u;
    }
    const size_t nt = (max_chunk + SAM_TILE - 1) / SAM_TILE + 1;
    ITX_HIP(hipMalloc((void **)&x->d_tile_sum, 16 * nt));
    ITX_HIP(hipMalloc((void **)&x->d_tile_base, 16 * nt));
    ITX_HIP(hipStreamCreateWithFlags(&x->st, hipStreamNonBlocking));
    ITX_HIP(hipStreamCreateWithFlags(&x->st_copy, hipStreamNonBlocking));
    const size_t c = (size_t)x->cap_lines, a4 = sam_up256(4 * c), a1 = sam_up256(c);
    for (auto &s : x->slot) {
        ITX_HIP(hipMalloc((void **)&s.d_text, sam_up256(max_chunk) + 256));
        ITX_HIP(hipMalloc((void **)&s.d_line_start, 4 * (c + 2)));
        ITX_HIP(hipMalloc(&s.d_rec, 10 * a4 + 3 * a1));
        uint8_t *p = (uint8_t *)s.d_rec;
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
        ITX_HIP(hipMalloc((void **)&s.d_tot, 16));
        ITX_HIP(hipMalloc((void **)&s.d_res, 4 * SAM_R_WORDS));
        ITX_HIP(hipHostMalloc((void **)&s.h_res, 4 * SAM_R_WORDS + 16, hipHostMallocDefault));
        hipEvent_t *ev[4] = {&s.ev_copy, &s.ev_k0, &s.ev_k1, &s.ev_done};
        for (auto e : ev) ITX_HIP(hipEventCreate(e));
    }
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
    if (len) ITX_HIP(hipMemcpyAsync(s.d_text, text, len, hipMemcpyHostToDevice, x->st_copy));
    ITX_HIP(hipEventRecord(s.ev_copy, x->st_copy));
    ITX_HIP(hipStreamWaitEvent(x->st, s.ev_copy, 0));
    ITX_HIP(hipEventRecord(s.ev_k0, x->st));
    ITX_HIP(hipMemsetAsync(s.d_res, 0, 4 * SAM_R_WORDS, x->st));
    ITX_HIP(hipMemsetAsync(s.d_res + SAM_R_FIRST, 0xff, 4, x->st));
    ITX_HIP(hipMemsetAsync(s.d_tot, 0, 16, x->st));
    const uint32_t nt = (uint32_t)((len + SAM_TILE - 1) / SAM_TILE);
    if (nt) {
        hipLaunchKernelGGL(k_sam_count, dim3(nt), dim3(SAM_TILE_WG), 0, x->st, s.d_text, (uint32_t)len, x->d_tile_sum);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, x->st, x->d_tile_sum, nt, x->d_tile_base, s.d_tot);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_sam_starts, dim3(nt), dim3(SAM_TILE_WG), 0, x->st, s.d_text, (uint32_t)len, x->d_tile_base, s.d_line_start, x->cap_lines);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_sam_parse, dim3(x->n_blocks), dim3(SAM_WAVES * 64u), 0, x->st, s.d_text, (uint32_t)len, final ? 1 : 0, s.d_line_start, s.d_tot, x->cap_lines,
                           x->names, s.out, s.d_res);
        ITX_HIP(hipGetLastError());
    }
    ITX_HIP(hipEventRecord(s.ev_k1, x->st));
    ITX_HIP(hipMemcpyAsync(s.h_res, s.d_res, 4 * SAM_R_WORDS, hipMemcpyDeviceToHost, x->st));
    ITX_HIP(hipMemcpyAsync(s.h_res + SAM_R_WORDS, s.d_tot, 16, hipMemcpyDeviceToHost, x->st));
    ITX_HIP(hipEventRecord(s.ev_done, x->st));
    s.state = 1;
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
    float ms = 0;
    ITX_HIP(hipEventElapsedTime(&ms, s.ev_k0, s.ev_k1));
    unsigned long long tot[2];
    memcpy(tot, s.h_res + SAM_R_WORDS, 16);
    memset(res, 0, sizeof *res);
    res->n_lines = s.h_res[SAM_R_LINES];
    res->consumed = s.len ? s.h_res[SAM_R_CONSUMED] : 0;
    res->n_hard = s.h_res[SAM_R_NHARD];
    res->first_hard_line = s.h_res[SAM_R_FIRST] >= 0x7fffffffu ? 0 : s.h_res[SAM_R_FIRST];
    if (tot[0] >= x->cap_lines) {                  // as many lines as the arrays hold, or more: one of them is too short for 11 fields
        if (!res->n_hard) res->first_hard_line = x->cap_lines;
        res->n_hard++;
    }
    res->flags = (int)(s.h_res[SAM_R_FLAGS] | (tot[1] ? ITX_SAMTEXT_NUL : 0));
    res->n_rec = res->n_hard ? 0 : res->n_lines;
    res->kernel_ms = ms;
    s.n_rec = res->n_rec;
    s.state = 2;
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
