// itx_bamout.hip — the BAM of `iteres filter -b` (an extension: the reference has no such output) built where the records lie:
// every record of a batch that chose a table row goes, block_size and bytes unchanged and in file order, into one stream of
// payload bytes in HBM; every ITX_BAMOUT_PAYLOAD bytes of that stream become one BGZF member (itx_bgzfmember.h), and only the
// members, compressed and packed, cross the link back. The header's members and the EOF marker are the host's (bamout.c).
//
// per batch (records in device memory, the chosen rows in d_hit_row):
//   k_bo_measure   one lane per record: 4 + block_size for a record with hit_row >= 0, else 0. A tile of BO_TILE records adds up
//                  its bytes (64 bit) and its records.
//   k_tile_scan2   (itx_textpack.h) exclusive sums over the tiles, one workgroup; the totals are all the host waits for: they
//                  say how many whole payloads the stream now holds, and every buffer is sized before anything is written.
//   k_bo_gather    one workgroup per tile: the tile's records are ONE contiguous range of the stream, behind what the call before
//                  left over; staged in LDS a window at a time and stored with 16-byte vectors (itx_textpack.h says why and how).
//   k_bo_member    one wave per whole payload: the payload into LDS, itx_bgzf_member into the member's slot (a fixed stride).
//                  After itx_bamout_set_level (filter -b -l) k_bo_member_stored (level 0) or k_bo_member_fast (level 1) stands in
//                  its place (itx_bgzflevels.h), in the same launch shape; nothing behind it knows the level.
//   k_bo_scan      exclusive sums of the member sizes, one workgroup     } written as k_bw_scan / k_bw_gather of itx_bigwig.hip
//   k_bo_pack      the members one behind the other                       }
//   then the stream's rest, less than one payload, moves to its front (device to device), and the packed total to the host.
// itx_bamout_collect hands a batch's members out: it waits for that batch's kernels only (the next batch's are queued behind them
// and go on), copies the packed bytes on the copy stream into one of two page-locked buffers, and the host writes them to the file
// while the next batch's kernels run — the bed route's arrangement.
// What the host route counted joins the same stream in stream order (itx_bamout_append_host), so the file is one ordered stream
// whatever route a window took. itx_bamout_finish makes the last, short payload a member.
// With itx_bamout_index_enable (filter -b -i) the stream's .bai index is collected beside it and made at the end
// (csrc/itx_bamidx.hip): an entry per counted record behind every gather, every batch's member sizes behind those before.
//
// With itx_bamout_sort_enable (filter -b -s) the stream is held whole instead of being cut: every gather appends to it, and one lane
// per record appends {tid, pos << 1 | reverse, where the record lies, its length} to a pool (k_bs_entries; the rule is
// csrc/itx_bamsortrule.h). After the last batch itx_bamout_sort_next sorts (key, index) pairs with itx_radixsort.h, by the low key
// and then by tid, stable, and replays the records in sorted order a round of at most batch_capacity at a time through the path
// above: k_bs_lengths lays the round's lengths and 64-bit offsets out in sorted order, k_tile_scan2, then k_bo_gather reads the held
// stream (scattered, a record each) and writes the payload stream (coalesced), then members, scan and pack as for any batch.
//
// With itx_bamout_annotate_enable (filter -b -a) a counted record leaves with the tags of its row behind it (csrc/itx_reptag.h):
// k_bo_measure<true> adds the tags' length, a function of the row alone, k_bo_gather<uint32_t, true> lays the record with
// itx_reptag_write in place of the byte copy. Everything behind the gather sees a longer record: the members, the index's chunks, the
// held stream of -s (annotated at the first gather; the replay copies byte for byte). Without the call the <false> instantiations run.
//
// Every buffer that grows (bo_reserve, bs_reserve) grows by the two-phase rule of itx_devbuf.h; the sort's passes are itx_sort_run's.
//
// Byte and integer work. k_bo_member is bound by the encoder's serial parse (one lane per member); ITX_BAMOUT_PAYLOAD is chosen
// for that (itx_bgzfmember.h). No kernel uses scratch (DESIGN.md has the figures).
#include "itx_bamidx.h"
#include "itx_bamsortrule.h"
#include "itx_devbuf.h"
#include "itx_radixsort.h"
#include "itx_reptag.h"
#include "itx_textpack.h"

#include <stdlib.h>
#include <string.h>

#define ITXD_FN __device__ static inline
#define ITXD_SYNC() __syncthreads()
#define ITXD_AMAX(p, v) atomicMax((p), (v))
#define ITXD_CTZ(x) ((uint32_t)__builtin_ctz(x))
#define ITXD_AADD(p, v) ((void)atomicAdd((p), (v)))
#define ITXD_AOR(p, v) ((void)atomicOr((p), (v)))
#include "itx_bgzflevels.h"

typedef unsigned long long ull;

#define BO_TILE 256u                 // records per workgroup (measure, gather)
#define BO_LDS 32768u                // bytes staged at a time: a tile of short reads (256 x ~120 bytes) in one window
#define BO_P ITX_BAMOUT_PAYLOAD
#define BO_STRIDE ITX_BGZF_MEMBER_CAP(BO_P)      // bytes between two members' slots (a multiple of 4)
#define BO_MAX_RECORD 0x40000000u    // a record of a gibibyte is nobody's: the decoder's windows hold less
#define BO_TOT_BYTES 64u             // a batch's totals: bytes, records, records too long; -a: rows outside the table, tag bytes

static_assert(BO_P % 16u == 0 && BO_P <= ITXD_MAX_IN, "the payload: at most one DEFLATE window, whole 16-byte vectors");
static_assert(BO_TILE == ITX_BAMIDX_TILE && BO_P == ITX_BAMIDX_PAYLOAD, "the index (itx_bamidx.hip) places records by the gather's tiles and payloads");

// ---- filter -b -a: the table's rows and names as the kernels read them (one allocation, itx_bamout_annotate_enable)
struct BoAnn {
    const uint32_t *rows;            // per row: start, end, rep, cla, fam
    const ull *rep_off, *cla_off, *fam_off;
    const uint8_t *rep, *cla, *fam;  // the name pools: name i of a pool is bytes [off[i], off[i + 1])
    uint32_t n_rows;
};
#define BO_ROW_WORDS 5u

__device__ __forceinline__ ItxRepTag bo_row_tag(const BoAnn &a, uint32_t row)
{
    const uint32_t *r = a.rows + (size_t)BO_ROW_WORDS * row;
    ItxRepTag t;
    t.start = r[0];
    t.end = r[1];
    const ull r0 = a.rep_off[r[2]], c0 = a.cla_off[r[3]], f0 = a.fam_off[r[4]];
    t.rep = a.rep + r0;
    t.rep_len = (uint32_t)(a.rep_off[r[2] + 1u] - r0);
    t.cla = a.cla + c0;
    t.cla_len = (uint32_t)(a.cla_off[r[3] + 1u] - c0);
    t.fam = a.fam + f0;
    t.fam_len = (uint32_t)(a.fam_off[r[4] + 1u] - f0);
    return t;
}

// ANN: the record's length includes the tags of its row (a row outside the table counts as bad, as a record too long does)
template <bool ANN>
__global__ __launch_bounds__(BO_TILE) void k_bo_measure(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, const int32_t *__restrict__ hit_row,
                                                         uint32_t n, uint32_t *__restrict__ len_out, ull *__restrict__ tile_sum, ull *__restrict__ tot, BoAnn ann)
{
    __shared__ ull s_sum[ANN ? 3 : 2];                                     // bytes, records; ANN: and the tag bytes among them
    if (threadIdx.x < (ANN ? 3 : 2)) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    bool bad = false, bad_row = false;
    if (i < n) {
        uint32_t len = 0;
        if (hit_row[i] >= 0) {
            const uint8_t *p = u + rec_off[i];
            const uint32_t bs = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            bad = bs >= BO_MAX_RECORD;
            uint32_t tag = 0;
            if constexpr (ANN) {
                bad_row = (uint32_t)hit_row[i] >= ann.n_rows;
                if (!bad && !bad_row) {
                    const ItxRepTag t = bo_row_tag(ann, (uint32_t)hit_row[i]);
                    tag = itx_reptag_len(&t);                              // (below 2^18: three names below 2^16 each)
                    bad = bs + tag >= BO_MAX_RECORD;
                }
            }
            if (!bad && !bad_row) {
                len = 4u + bs + tag;
                atomicAdd(&s_sum[0], (ull)len);
                atomicAdd(&s_sum[1], 1ull);
                if constexpr (ANN) atomicAdd(&s_sum[2], (ull)tag);
            }
        }
        len_out[i] = len;
    }
    const ull badm = __ballot(bad);
    if ((threadIdx.x & 63u) == 0 && badm) atomicAdd(&tot[2], (ull)__popcll(badm));
    if constexpr (ANN) {
        const ull rowm = __ballot(bad_row);
        if ((threadIdx.x & 63u) == 0 && rowm) atomicAdd(&tot[3], (ull)__popcll(rowm));
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
    if constexpr (ANN) {
        if (threadIdx.x == 2 && s_sum[2]) atomicAdd(&tot[4], s_sum[2]);
    }
}

// OFF: uint32_t offsets into a window; 64-bit offsets into the held stream (the replay of filter -b -s)
// ANN: len_in are annotated lengths and the record is laid with its row's tags behind it (hit_row and ann are read only then)
template <class OFF, bool ANN>
__global__ __launch_bounds__(BO_TILE) void k_bo_gather(const uint8_t *__restrict__ u, const OFF *__restrict__ rec_off, uint32_t n,
                                                        const uint32_t *__restrict__ len_in, const ull *__restrict__ tile_base, ull base, uint8_t *__restrict__ pay,
                                                        const int32_t *__restrict__ hit_row, BoAnn ann)
{
    __shared__ uint4 s_buf[BO_LDS / 16u];
    __shared__ uint32_t s_w[BO_TILE / 64u];
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0;
    const uint32_t moff = itx_tile_offsets<BO_TILE>(len, s_w, &total);
    const ull tb = base + tile_base[2u * blockIdx.x], te = tb + total;
    const ull mb = tb + moff, me = mb + len;
    const uint8_t *src = len ? u + rec_off[i] : u;
    if constexpr (ANN) {
        // the measure pass has checked the row; the names are a few cached bytes per lane, read where they are laid
        ItxRepTag t = {};
        if (len) t = bo_row_tag(ann, (uint32_t)hit_row[i]);
        const uint32_t rec_len = len - (len ? itx_reptag_len(&t) : 0u);
        itx_pack_tile<BO_TILE, BO_LDS>(s_buf, pay, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) { itx_reptag_write(src, rec_len, &t, from, to, dst); });
    } else {
        itx_pack_tile<BO_TILE, BO_LDS>(s_buf, pay, tb, te, mb, me, [=](uint8_t *dst, uint32_t from, uint32_t to) {
            // a record starts wherever the one before it ended: kept a byte loop (names' gather says why)
#pragma clang loop vectorize(disable)
            for (uint32_t k = from; k < to; k++) dst[k - from] = src[k];
        });
    }
}

// ---- filter -b -s: what is collected during the pass and the order of the replay
struct BoSortEnt {
    uint32_t tid, low;               // the high and the low sort key (itx_bamsortrule.h)
    ull off;                         // the record's first byte in the held stream
    uint32_t len, pad;               // 4 + block_size
};
static_assert(sizeof(BoSortEnt) == 24, "BoSortEnt");

// behind a batch's gather: one entry per counted record (len != 0). Its place in the held stream comes from the gather's own tile
// bases and itx_tile_offsets, its place in the pool from the tile's record count the same way (k_bi_entries' arrangement).
// flag[0] counts the records that cannot be sorted, flag[1] is the highest tid seen; a workgroup adds to them once.
__global__ __launch_bounds__(BO_TILE) void k_bs_entries(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, uint32_t n, const uint32_t *__restrict__ len_in,
                                                         const ull *__restrict__ tile_base, ull stream_at, ull ent_at, BoSortEnt *__restrict__ ent, uint32_t *__restrict__ flag)
{
    __shared__ uint32_t s_w[BO_TILE / 64u], s_c[BO_TILE / 64u], s_f[2];
    if (threadIdx.x < 2) s_f[threadIdx.x] = 0;                             // (the barriers of itx_tile_offsets order this)
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0, count = 0;
    const uint32_t moff = itx_tile_offsets<BO_TILE>(len, s_w, &total);
    const uint32_t rank = itx_tile_offsets<BO_TILE>(len ? 1u : 0u, s_c, &count);
    if (len) {
        ItxBamSortKey k;
        // (under -a `len` is the annotated length while the bytes here are the source record's: the fields lie inside the shorter)
        const uint8_t *p = u + rec_off[i];
        const uint32_t src_len = 4u + itx_bamsort_u32(p);
        const int bad = itx_bamsort_key(p, src_len < len ? src_len : len, &k);
        BoSortEnt e;
        e.tid = itx_bamsort_high(&k);
        e.low = itx_bamsort_low(&k);
        e.off = stream_at + tile_base[2u * blockIdx.x] + moff;
        e.len = len;
        e.pad = 0;
        ent[ent_at + tile_base[2u * blockIdx.x + 1u] + rank] = e;
        if (bad) atomicAdd(&s_f[0], 1u);
        else atomicMax(&s_f[1], e.tid);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_f[0]) atomicAdd(&flag[0], s_f[0]);
        if (s_f[1]) atomicMax(&flag[1], s_f[1]);
    }
}

// the pairs the radix sort moves: (low key, the entry's number); after the passes over the low key the key becomes the entry's tid
__global__ __launch_bounds__(256) void k_bs_keys(const BoSortEnt *__restrict__ ent, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = make_uint2(ent[i].low, i);
}

__global__ __launch_bounds__(256) void k_bs_rekey(const BoSortEnt *__restrict__ ent, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i].x = ent[keys[i].y].tid;
}

// one round of the replay, records sorted[0 .. n): their lengths and where they lie in the held stream, laid out in sorted order
// for the gather; a tile's bytes (64 bit) and records as k_bo_measure leaves them
__global__ __launch_bounds__(BO_TILE) void k_bs_lengths(const uint2 *__restrict__ sorted, const BoSortEnt *__restrict__ ent, uint32_t n, uint32_t *__restrict__ len_out,
                                                         ull *__restrict__ off_out, ull *__restrict__ tile_sum)
{
    __shared__ ull s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BO_TILE + threadIdx.x;
    if (i < n) {
        const BoSortEnt e = ent[sorted[i].y];
        len_out[i] = e.len;
        off_out[i] = e.off;
        atomicAdd(&s_sum[0], (ull)e.len);
        atomicAdd(&s_sum[1], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_sum[2u * blockIdx.x + threadIdx.x] = s_sum[threadIdx.x];
}

// LDS of one member's encoder (itxd_ws), for payloads of up to BO_P bytes
struct BoLds {
    uint32_t in[BO_P / 4 + 4];
    uint32_t head[1u << ITXD_HBITS];
    uint16_t md[BO_P];
    uint8_t ml[BO_P];
    uint32_t fq[ITXD_NSYM], key[ITXD_NSYM];
    uint16_t srt[ITXD_NSYM], code[ITXD_NSYM];
    uint8_t len[ITXD_NSYM];
    uint32_t clfq[20];
    uint16_t clcode[20];
    uint8_t cllen[20];
    uint64_t red[128];
    uint32_t misc[16];
};

// one wave per member: payload m is pay[m * BO_P, min((m + 1) * BO_P, total)); pay is 16-byte aligned and BO_P a multiple of 16
__global__ __launch_bounds__(64) void k_bo_member(const uint8_t *__restrict__ pay, ull total, uint8_t *__restrict__ mem, uint32_t *__restrict__ msize)
{
    __shared__ BoLds s;
    const ull at = (ull)blockIdx.x * BO_P;
    const uint32_t lane = threadIdx.x;
    const uint32_t n = total - at < BO_P ? (uint32_t)(total - at) : BO_P;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(pay + at);
    for (uint32_t i = lane; i < BO_P / 4 + 4; i += 64) {
        uint32_t v = 0;
        if (4u * i + 4u <= n) {
            v = src[i];
        } else {
            for (uint32_t k = 0; k < 4u && 4u * i + k < n; k++) v |= (uint32_t)pay[at + 4u * i + k] << (8u * k);      // (the last payload's ragged word)
        }
        s.in[i] = v;
    }
    __syncthreads();
    const itxd_ws w = {s.in, s.head, s.ml, s.md, s.fq, s.key, s.srt, s.len, s.code, s.clfq, s.cllen, s.clcode, s.red, s.misc};
    const uint32_t z = itx_bgzf_member(w, n, mem + (ull)blockIdx.x * BO_STRIDE, lane, 64);
    if (lane == 0) msize[blockIdx.x] = z;
}

// ---- filter -b -l: the other levels of the members (itx_bgzflevels.h), in k_bo_member's launch shape
// payload `m` of the stream into LDS as little-endian words, zero beyond its n bytes; returns n
__device__ static inline uint32_t bo_load_payload(const uint8_t *__restrict__ pay, ull total, uint32_t *in)
{
    const ull at = (ull)blockIdx.x * BO_P;
    const uint32_t n = total - at < BO_P ? (uint32_t)(total - at) : BO_P;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(pay + at);
    for (uint32_t i = threadIdx.x; i < BO_P / 4 + 4; i += 64) {
        uint32_t v = 0;
        if (4u * i + 4u <= n) {
            v = src[i];
        } else {
            for (uint32_t k = 0; k < 4u && 4u * i + k < n; k++) v |= (uint32_t)pay[at + 4u * i + k] << (8u * k);      // (the last payload's ragged word)
        }
        in[i] = v;
    }
    __syncthreads();
    return n;
}

#define BO_STAGE_WORDS ITXF_STAGE_WORDS(BO_P, ITX_BGZF_LEAD)       // a whole member of a full payload, in words
static_assert(4u * BO_STAGE_WORDS <= BO_STRIDE, "a member's whole words fit its slot");

// level 0: the payload behind a stored block's 5 bytes. The workspace is the payload, the member and the CRC's terms.
__global__ __launch_bounds__(64) void k_bo_member_stored(const uint8_t *__restrict__ pay, ull total, uint8_t *__restrict__ mem, uint32_t *__restrict__ msize)
{
    __shared__ uint32_t s_in[BO_P / 4 + 4], s_stage[BO_STAGE_WORDS];
    __shared__ uint64_t s_red[64];
    const uint32_t n = bo_load_payload(pay, total, s_in);
    const itxf_ws w = {{s_in, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s_red, nullptr}, s_stage, nullptr};
    const uint32_t z = itx_bgzf_member_level(w, n, mem + (ull)blockIdx.x * BO_STRIDE, threadIdx.x, 64, 0u);
    if (threadIdx.x == 0) msize[blockIdx.x] = z;
}

// LDS of the fast level's encoder: BoLds with the member's staging area over the hash heads (dead when it is first written), which
// is 32 bytes longer than they are, and the slices' bit counts
struct BoLdsFast {
    uint32_t in[BO_P / 4 + 4];
    uint32_t head[BO_STAGE_WORDS];
    uint16_t md[BO_P];
    uint8_t ml[BO_P];
    uint32_t fq[ITXD_NSYM], key[ITXD_NSYM];
    uint16_t srt[ITXD_NSYM], code[ITXD_NSYM];
    uint8_t len[ITXD_NSYM];
    uint32_t clfq[20];
    uint16_t clcode[20];
    uint8_t cllen[20];
    uint64_t red[128];
    uint32_t misc[16];
    uint32_t sbits[ITXF_SLICES(BO_P) + 1];
};
static_assert(BO_STAGE_WORDS >= (1u << ITXD_HBITS), "the staging area holds the hash heads");
static_assert(3u * sizeof(BoLdsFast) <= 160u * 1024u, "three members in flight per CU, as k_bo_member");

// level 1: every stage of the encoder on all 64 lanes (itx_deflate_fast.h)
__global__ __launch_bounds__(64) void k_bo_member_fast(const uint8_t *__restrict__ pay, ull total, uint8_t *__restrict__ mem, uint32_t *__restrict__ msize)
{
    __shared__ BoLdsFast s;
    const uint32_t n = bo_load_payload(pay, total, s.in);
    const itxf_ws w = {{s.in, s.head, s.ml, s.md, s.fq, s.key, s.srt, s.len, s.code, s.clfq, s.cllen, s.clcode, s.red, s.misc}, s.head, s.sbits};
    const uint32_t z = itx_bgzf_member_level(w, n, mem + (ull)blockIdx.x * BO_STRIDE, threadIdx.x, 64, 1u);
    if (threadIdx.x == 0) msize[blockIdx.x] = z;
}

// exclusive prefix sum of the member sizes: moff[0 .. n] (one workgroup, itx_device.h)
__global__ __launch_bounds__(ITX_SCAN_WG) void k_bo_scan(const uint32_t *__restrict__ msize, uint64_t n, uint64_t *__restrict__ moff)
{
    __shared__ uint64_t s[ITX_SCAN_WG];
    uint64_t lo, hi;
    itx_scan_chunk(n, &lo, &hi);
    uint64_t a = 0, total;
    for (uint64_t i = lo; i < hi; i++) a += msize[i];
    uint64_t e = itx_scan_wg(a, s, &total);
    for (uint64_t i = lo; i < hi; i++) {
        moff[i] = e;
        e += msize[i];
    }
    if (threadIdx.x == 0) moff[n] = total;
}

__global__ __launch_bounds__(256) void k_bo_pack(const uint8_t *__restrict__ mem, const uint32_t *__restrict__ msize, const uint64_t *__restrict__ moff,
                                                 uint8_t *__restrict__ packed)
{
    const uint64_t b = blockIdx.x;
    const uint8_t *src = mem + b * BO_STRIDE;
    uint8_t *dst = packed + moff[b];
    const uint32_t z = msize[b] < BO_STRIDE ? msize[b] : BO_STRIDE;
    for (uint32_t i = threadIdx.x; i < z; i += 256) dst[i] = src[i];
}

// ---- host side
struct bo_slot {                     // one batch's members on their way out
    uint8_t *d_packed, *h_pin;
    size_t cap;                      // bytes of both
    ull *h_total;                    // page-locked: the packed size
    hipEvent_t e0, e1;               // around member + scan + pack; e1 is the batch's "done"
    uint32_t n_mem;
    int busy;
};

struct itx_bamout {
    int device;
    size_t cap;                      // records per batch
    hipStream_t st, cst;             // kernels; the copies to the host
    hipEvent_t ev[5];                // measure: 0 .. 1, gather: 2 .. 3 (3: the batch's records are read); 4: the caller's stream
    int gather_timed;
    int32_t *d_hits;
    uint32_t *d_len;
    ull *d_tile_sum, *d_tile_base, *d_tot, *h_tot;
    uint8_t *d_pay;                  // the payload stream: carry bytes, then the batch's
    size_t pay_cap, carry;
    uint8_t *d_mem;                  // member slots of BO_STRIDE bytes
    uint32_t *d_msize;
    uint64_t *d_moff;
    size_t mem_cap;                  // members
    bo_slot slot[2];
    int head, pending;               // the oldest batch not yet collected; batches not yet collected
    int finished;
    int level, level_set;            // the members' level (itx_bgzflevels.h): 6 unless itx_bamout_set_level chose another
    itx_bamout_stats stats;
    int annotate;                    // filter -b -a (itx_bamout_annotate_enable): d_ann holds the rows and names, ann points into it
    void *d_ann;
    BoAnn ann;
    ull tag_bytes;                   // tag bytes the device batches appended
    itx_bamidx *ix;                  // filter -b -i (itx_bamout_index_enable): the .bai index in the making, else null
    ull stream_base;                 // bytes of the record stream that are members already: d_pay[0] is this byte of the stream
    // filter -b -s (itx_bamout_sort_enable)
    int sort;                        // 0: off; 1: the stream is held (d_pay is the held stream, carry its bytes); 2: it is replayed
    int32_t n_ref;                   // from index_enable, else -1: the highest tid seen says how many passes tid takes
    BoSortEnt *d_sent;               // the pool: an entry per held record, in stream order
    ull n_sent, sent_cap, sent_grows;
    uint32_t *d_sflag, *h_sflag;     // [0] records that cannot be sorted, [1] the highest tid (device batches; h_sflag page-locked)
    ull host_bad;                    // the same of the host route's records
    uint32_t host_maxtid;
    uint8_t *d_held;                 // the replay: the held stream, the pairs in both buffers and where the sorted ones are,
    uint2 *d_k0, *d_k1, *sorted;     // the digit counts, the round's offsets into the held stream
    uint32_t *d_hist;
    ull *d_soff;
    ull sort_done, rounds;           // records replayed; rounds
    hipEvent_t sev[2];               // around the sort
    int sort_timed;
    double sort_ms, replay_ms;
};

extern "C" void itx_bamout_destroy(itx_bamout *bo)
{
    if (!bo) return;
    (void)hipSetDevice(bo->device);
    if (bo->st) (void)hipStreamSynchronize(bo->st);
    if (bo->cst) (void)hipStreamSynchronize(bo->cst);
    for (auto &e : bo->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &s : bo->slot) {
        if (s.e0) (void)hipEventDestroy(s.e0);
        if (s.e1) (void)hipEventDestroy(s.e1);
        (void)hipFree(s.d_packed);
        if (s.h_pin) (void)hipHostFree(s.h_pin);
        if (s.h_total) (void)hipHostFree(s.h_total);
    }
    if (bo->st) (void)hipStreamDestroy(bo->st);
    if (bo->cst) (void)hipStreamDestroy(bo->cst);
    (void)hipFree(bo->d_hits);
    (void)hipFree(bo->d_len);
    (void)hipFree(bo->d_tile_sum);
    (void)hipFree(bo->d_tile_base);
    (void)hipFree(bo->d_tot);
    (void)hipFree(bo->d_pay);
    (void)hipFree(bo->d_mem);
    (void)hipFree(bo->d_msize);
    (void)hipFree(bo->d_moff);
    if (bo->h_tot) (void)hipHostFree(bo->h_tot);
    for (auto &e : bo->sev)
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(bo->d_sent);
    (void)hipFree(bo->d_sflag);
    if (bo->h_sflag) (void)hipHostFree(bo->h_sflag);
    (void)hipFree(bo->d_held);
    (void)hipFree(bo->d_k0);
    (void)hipFree(bo->d_k1);
    (void)hipFree(bo->d_hist);
    (void)hipFree(bo->d_soff);
    (void)hipFree(bo->d_ann);
    itx_bamidx_destroy(bo->ix);
    delete bo;
}

extern "C" int itx_bamout_create(int device, size_t batch_capacity, size_t stream_bytes, itx_bamout **out)
{
    if (!out || batch_capacity == 0 || batch_capacity > 0xffffff00u) {
        itx_set_error("itx_bamout_create: bad argument");
        return ITX_E_ARG;
    }
    *out = nullptr;
    int rc = ITX_OK;
    itx_bamout *bo = new itx_bamout();
    bo->device = device;
    bo->cap = batch_capacity;
    bo->n_ref = -1;
    bo->level = 6;
    const size_t n = batch_capacity + 64, nt = (batch_capacity + BO_TILE - 1) / BO_TILE + 1;
    if (stream_bytes < 4 * (size_t)BO_P) stream_bytes = 4 * (size_t)BO_P;
    bo->pay_cap = stream_bytes;
    ITX_TRY(hipSetDevice(device));
    if (hipMalloc((void **)&bo->d_hits, 4 * n) != hipSuccess || hipMalloc((void **)&bo->d_len, 4 * n) != hipSuccess ||
        hipMalloc((void **)&bo->d_tile_sum, 16 * nt) != hipSuccess || hipMalloc((void **)&bo->d_tile_base, 16 * nt) != hipSuccess ||
        hipMalloc((void **)&bo->d_tot, BO_TOT_BYTES) != hipSuccess || hipMalloc((void **)&bo->d_pay, bo->pay_cap + 16) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_create: no device memory for batches of %zu records and a stream of %zu bytes", batch_capacity, stream_bytes);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipHostMalloc((void **)&bo->h_tot, BO_TOT_BYTES, hipHostMallocDefault));
    ITX_TRY(hipStreamCreateWithFlags(&bo->st, hipStreamNonBlocking));
    ITX_TRY(hipStreamCreateWithFlags(&bo->cst, hipStreamNonBlocking));
    for (auto &e : bo->ev) ITX_TRY(hipEventCreate(&e));
    for (auto &s : bo->slot) {
        ITX_TRY(hipEventCreate(&s.e0));
        ITX_TRY(hipEventCreate(&s.e1));
        ITX_TRY(hipHostMalloc((void **)&s.h_total, 16, hipHostMallocDefault));
    }
out:
    if (rc != ITX_OK) {
        itx_bamout_destroy(bo);
        return rc;
    }
    *out = bo;
    return ITX_OK;
}

extern "C" int32_t *itx_bamout_hits(itx_bamout *bo) { return bo ? bo->d_hits : nullptr; }
extern "C" void *itx_bamout_stream(itx_bamout *bo) { return bo ? (void *)bo->st : nullptr; }

static void bo_read_gather_time(itx_bamout *bo)
{
    if (bo->ix) itx_bamidx_batch_time(bo->ix);
    if (!bo->gather_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, bo->ev[2], bo->ev[3]) == hipSuccess) *(bo->sort == 2 ? &bo->replay_ms : &bo->stats.gather_ms) += (double)ms;
    bo->gather_timed = 0;
}

// filter -b -s: room for n_more more entries in the pool; bo->st is idle. What does not fit leaves the object as it was.
static int bs_reserve(itx_bamout *bo, ull n_more)
{
    const ull want = bo->n_sent + n_more;
    if (want >= 0xfffffffeull) {
        itx_set_error("itx_bamout: %llu records to sort (run without -s)", want);
        return ITX_E_LIMIT;
    }
    if (want <= bo->sent_cap) return ITX_OK;
    const ull cap = want + want / 2 + 1024;
    const bool first = !bo->d_sent;
    ItxGrow g = {(void **)&bo->d_sent, sizeof(BoSortEnt) * bo->n_sent, sizeof(BoSortEnt) * cap};       // the pool alone; its entries are kept
    if (itx_grow_alloc(&g, 1) >= 0) {
        itx_set_error("itx_bamout: no device memory for the sort entries of %llu records (run without -s)", want);
        return ITX_E_NOMEM;
    }
    const int rc = itx_grow_commit(bo->st, &g, 1);
    if (rc != ITX_OK) return rc;
    bo->sent_cap = cap;
    if (!first) bo->sent_grows++;
    return ITX_OK;
}

// Room for a stream of `total` bytes and for the n_mem members made of it next; bo->st is idle when this is called. Every limit is
// checked and every buffer allocated here, before anything is written: what does not fit leaves the object as it was.
static int bo_reserve(itx_bamout *bo, ull total, ull n_mem)
{
    bo_slot *s = &bo->slot[(bo->head + bo->pending) & 1];
    size_t want_pay = 0, want_mem = 0, want_pk = 0;
    if (n_mem > 0x7fffff00ull) {
        itx_set_error("itx_bamout: %llu members in one batch", n_mem);
        return ITX_E_LIMIT;
    }
    if (n_mem && bo->pending == 2) {
        itx_set_error("itx_bamout: two batches wait to be collected (itx_bamout_collect)");
        return ITX_E_STATE;
    }
    if (total > bo->pay_cap) want_pay = (size_t)(total + (total > 2 * (ull)bo->pay_cap ? total / 4 : total));
    if (n_mem > bo->mem_cap) want_mem = (size_t)(n_mem + n_mem / 4 + 16);
    if (n_mem && n_mem * BO_STRIDE > s->cap) want_pk = (size_t)((n_mem + n_mem / 4 + 16) * BO_STRIDE);
    // taken together: the stream, of which the carry is kept; the members' slots, sizes and offsets; the slot's packed buffer and its
    // page-locked twin (the slot is not busy: nothing reads its buffers). Of the last five nothing is kept.
    ItxGrow g[6] = {{(void **)&bo->d_pay, bo->carry, want_pay ? want_pay + 16 : 0},
                    {(void **)&bo->d_mem, 0, want_mem * BO_STRIDE},
                    {(void **)&bo->d_msize, 0, 4 * want_mem},
                    {(void **)&bo->d_moff, 0, want_mem ? 8 * (want_mem + 1) : 0},
                    {(void **)&s->d_packed, 0, want_pk},
                    {(void **)&s->h_pin, 0, want_pk, 1}};
    if (itx_grow_alloc(g, 6) >= 0) {
        itx_set_error("itx_bamout: no memory for a stream of %llu bytes in %llu members%s", total, n_mem, bo->sort ? " (run without -s)" : "");
        return ITX_E_NOMEM;
    }
    const int rc = itx_grow_commit(bo->st, g, 6);
    if (rc != ITX_OK) return rc;
    if (want_pay) {
        bo->pay_cap = want_pay;
        bo->stats.grows++;
    }
    if (want_mem) bo->mem_cap = want_mem;
    if (want_pk) s->cap = want_pk;
    return ITX_OK;
}

// d_pay holds `total` bytes: its whole payloads (with_tail: and the short rest) become members in the next slot, the rest moves
// to the front. bo_reserve(total, that many members) has succeeded.
static int bo_emit(itx_bamout *bo, ull total, int with_tail)
{
    int rc = ITX_OK;
    const ull n_full = total / BO_P, rest = total - n_full * BO_P;
    const uint32_t n_mem = (uint32_t)(n_full + (with_tail && rest ? 1 : 0));
    if (n_mem) {
        bo_slot *s = &bo->slot[(bo->head + bo->pending) & 1];
        ITX_TRY(hipEventRecord(s->e0, bo->st));
        const ull n_bytes = with_tail ? total : n_full * BO_P;
        if (bo->level == 6) hipLaunchKernelGGL(k_bo_member, dim3(n_mem), dim3(64), 0, bo->st, bo->d_pay, n_bytes, bo->d_mem, bo->d_msize);
        else if (bo->level == 1) hipLaunchKernelGGL(k_bo_member_fast, dim3(n_mem), dim3(64), 0, bo->st, bo->d_pay, n_bytes, bo->d_mem, bo->d_msize);
        else hipLaunchKernelGGL(k_bo_member_stored, dim3(n_mem), dim3(64), 0, bo->st, bo->d_pay, n_bytes, bo->d_mem, bo->d_msize);
        ITX_TRY(hipGetLastError());
        if (bo->ix && (rc = itx_bamidx_members(bo->ix, bo->st, bo->d_msize, n_mem)) != ITX_OK) goto out;
        hipLaunchKernelGGL(k_bo_scan, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_msize, (uint64_t)n_mem, bo->d_moff);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bo_pack, dim3(n_mem), dim3(256), 0, bo->st, bo->d_mem, bo->d_msize, bo->d_moff, s->d_packed);
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(s->h_total, bo->d_moff + n_mem, 8, hipMemcpyDeviceToHost, bo->st));
        ITX_TRY(hipEventRecord(s->e1, bo->st));
        s->n_mem = n_mem;
        s->busy = 1;
        bo->pending++;
        bo->stats.members += n_mem;
    }
    if (with_tail) {
        bo->carry = 0;
    } else {
        if (n_full && rest) ITX_TRY(hipMemcpyAsync(bo->d_pay, bo->d_pay + n_full * BO_P, (size_t)rest, hipMemcpyDeviceToDevice, bo->st));   // (rest < BO_P: no overlap)
        bo->carry = (size_t)rest;
    }
    bo->stream_base += with_tail ? total : n_full * BO_P;
out:
    return rc;
}

// measure + scan (waited for: the totals size every buffer), then gather, members and pack are enqueued
int itx_bamout_start(itx_bamout *bo, const uint8_t *u, const uint32_t *rec_off, const int32_t *d_hit_row, size_t n, void *stream)
{
    if (!bo || (n && (!u || !rec_off || !d_hit_row))) {
        itx_set_error("itx_bamout: bad argument");
        return ITX_E_ARG;
    }
    if (n > bo->cap) {
        itx_set_error("itx_bamout: batch exceeds the capacity");
        return ITX_E_ARG;
    }
    if (bo->finished || bo->sort == 2) {
        itx_set_error("itx_bamout: the stream is %s", bo->finished ? "finished" : "being replayed in sorted order");
        return ITX_E_STATE;
    }
    if (!n) return ITX_OK;
    int rc = ITX_OK;
    float ms = 0;
    ull total = 0;
    const uint32_t nt = (uint32_t)((n + BO_TILE - 1) / BO_TILE);
    ITX_TRY(hipSetDevice(bo->device));
    if ((hipStream_t)stream != bo->st) {                                   // the chosen rows were left on another stream
        ITX_TRY(hipEventRecord(bo->ev[4], (hipStream_t)stream));
        ITX_TRY(hipStreamWaitEvent(bo->st, bo->ev[4], 0));
    }
    ITX_TRY(hipEventRecord(bo->ev[0], bo->st));
    ITX_TRY(hipMemsetAsync(bo->d_tot, 0, BO_TOT_BYTES, bo->st));
    if (bo->annotate)
        hipLaunchKernelGGL((k_bo_measure<true>), dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, d_hit_row, (uint32_t)n, bo->d_len, bo->d_tile_sum, bo->d_tot, bo->ann);
    else
        hipLaunchKernelGGL((k_bo_measure<false>), dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, d_hit_row, (uint32_t)n, bo->d_len, bo->d_tile_sum, bo->d_tot, bo->ann);
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_tile_sum, nt, bo->d_tile_base, bo->d_tot);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(bo->ev[1], bo->st));
    ITX_TRY(hipMemcpyAsync(bo->h_tot, bo->d_tot, BO_TOT_BYTES, hipMemcpyDeviceToHost, bo->st));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bo_read_gather_time(bo);                                               // (the batch before this one)
    ITX_TRY(hipEventElapsedTime(&ms, bo->ev[0], bo->ev[1]));
    bo->stats.gather_ms += (double)ms;
    if (bo->h_tot[3]) {
        itx_set_error("itx_bamout: %llu records chose a row outside the %u rows given to itx_bamout_annotate_enable", bo->h_tot[3], bo->ann.n_rows);
        rc = ITX_E_ARG;
        goto out;
    }
    if (bo->h_tot[2]) {
        itx_set_error("itx_bamout: %llu records of a gibibyte or more%s", bo->h_tot[2], bo->annotate ? " with their tags" : "");
        rc = ITX_E_LIMIT;
        goto out;
    }
    total = (ull)bo->carry + bo->h_tot[0];
    // (sort mode: the stream is held whole, no member is made and nothing is indexed before the replay)
    if ((rc = bo_reserve(bo, total, bo->sort ? 0 : total / BO_P)) != ITX_OK) goto out;
    if (bo->sort && (rc = bs_reserve(bo, bo->h_tot[1])) != ITX_OK) goto out;
    if (bo->ix && !bo->sort && (rc = itx_bamidx_reserve(bo->ix, bo->st, bo->h_tot[1], total / BO_P)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(bo->ev[2], bo->st));
    if (bo->h_tot[0]) {
        if (bo->annotate)
            hipLaunchKernelGGL((k_bo_gather<uint32_t, true>), dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, (uint32_t)n, bo->d_len, bo->d_tile_base, (ull)bo->carry,
                               bo->d_pay, d_hit_row, bo->ann);
        else
            hipLaunchKernelGGL((k_bo_gather<uint32_t, false>), dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, (uint32_t)n, bo->d_len, bo->d_tile_base, (ull)bo->carry,
                               bo->d_pay, d_hit_row, bo->ann);
        ITX_TRY(hipGetLastError());
    }
    if (bo->sort && bo->h_tot[1]) {
        hipLaunchKernelGGL(k_bs_entries, dim3(nt), dim3(BO_TILE), 0, bo->st, u, rec_off, (uint32_t)n, bo->d_len, bo->d_tile_base, (ull)bo->carry, bo->n_sent, bo->d_sent,
                           bo->d_sflag);
        ITX_TRY(hipGetLastError());
        bo->n_sent += bo->h_tot[1];
    }
    ITX_TRY(hipEventRecord(bo->ev[3], bo->st));
    bo->gather_timed = 1;
    if (bo->ix && !bo->sort &&
        (rc = itx_bamidx_entries(bo->ix, bo->st, u, rec_off, (uint32_t)n, bo->d_len, bo->d_tile_base, bo->stream_base + bo->carry, bo->h_tot[1])) != ITX_OK)
        goto out;
    bo->stats.batches++;
    bo->stats.records += bo->h_tot[1];
    bo->stats.payload_bytes += bo->h_tot[0];
    bo->tag_bytes += bo->h_tot[4];
    if (bo->sort) bo->carry = (size_t)total;
    else rc = bo_emit(bo, total, 0);
out:
    return rc;
}

extern "C" int itx_bamout_run(itx_bamout *bo, const void *d_bytes, const uint32_t *d_rec_off, const int32_t *d_hit_row, size_t n, void *stream)
{
    return itx_bamout_start(bo, (const uint8_t *)d_bytes, d_rec_off, d_hit_row, n, stream);
}

// the batch's records have been read (its members may still be in the making): the window's arrays are the decoder's again
extern "C" int itx_bamout_wait_kernels(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_wait_kernels: bad argument");
        return ITX_E_ARG;
    }
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(bo->device));
    if (bo->gather_timed) {
        const double t0 = itx_wall_now();
        ITX_TRY(hipEventSynchronize(bo->ev[3]));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
        bo_read_gather_time(bo);
    }
out:
    return rc;
}

extern "C" int itx_bamout_append_host(itx_bamout *bo, const void *bytes, size_t len)
{
    if (!bo || (len && !bytes)) {
        itx_set_error("itx_bamout_append_host: bad argument");
        return ITX_E_ARG;
    }
    if (bo->finished || bo->sort == 2) {
        itx_set_error("itx_bamout_append_host: the stream is %s", bo->finished ? "finished" : "being replayed in sorted order");
        return ITX_E_STATE;
    }
    size_t at = 0, n_rec = 0;
    uint32_t *h_off = nullptr;                                             // with an index: where every record starts
    BoSortEnt *h_ent = nullptr;                                            // sort mode: the records' entries, made here
    ull bad = 0;
    uint32_t maxtid = 0;
    if (bo->ix && !bo->sort && len >= 0xffffff00ull) {
        itx_set_error("itx_bamout_append_host: %zu bytes in one call while an index is built", len);
        return ITX_E_LIMIT;
    }
    while (at < len) {                                                     // whole records, or nothing is appended
        uint32_t bs = 0;
        if (len - at >= 4) memcpy(&bs, (const uint8_t *)bytes + at, 4);
        if (len - at < 4 || bs >= BO_MAX_RECORD || (size_t)bs > len - at - 4) {
            itx_set_error("itx_bamout_append_host: the bytes are not whole records (record %zu at byte %zu of %zu)", n_rec, at, len);
            return ITX_E_ARG;
        }
        at += 4 + (size_t)bs;
        n_rec++;
    }
    if (!len) return ITX_OK;
    int rc = ITX_OK;
    const ull total = (ull)bo->carry + len;
    if (bo->sort) {
        if (!(h_ent = (BoSortEnt *)malloc(sizeof(BoSortEnt) * n_rec))) {
            itx_set_error("itx_bamout_append_host: no memory for the sort entries of %zu records", n_rec);
            return ITX_E_NOMEM;
        }
        at = 0;
        for (size_t i = 0; i < n_rec; i++) {
            uint32_t bs;
            ItxBamSortKey k;
            memcpy(&bs, (const uint8_t *)bytes + at, 4);
            if (itx_bamsort_key((const uint8_t *)bytes + at, 4u + bs, &k)) bad++;
            else if ((uint32_t)k.tid > maxtid) maxtid = (uint32_t)k.tid;
            h_ent[i].tid = itx_bamsort_high(&k);
            h_ent[i].low = itx_bamsort_low(&k);
            h_ent[i].off = (ull)bo->carry + at;
            h_ent[i].len = 4u + bs;
            h_ent[i].pad = 0;
            at += 4 + (size_t)bs;
        }
    } else if (bo->ix) {
        if (!(h_off = (uint32_t *)malloc(4 * n_rec))) {
            itx_set_error("itx_bamout_append_host: no memory for the offsets of %zu records", n_rec);
            return ITX_E_NOMEM;
        }
        at = 0;
        for (size_t i = 0; i < n_rec; i++) {
            uint32_t bs;
            memcpy(&bs, (const uint8_t *)bytes + at, 4);
            h_off[i] = (uint32_t)at;
            at += 4 + (size_t)bs;
        }
    }
    ITX_TRY(hipSetDevice(bo->device));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));                              // device batches before this one have their place
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bo_read_gather_time(bo);
    if ((rc = bo_reserve(bo, total, bo->sort ? 0 : total / BO_P)) != ITX_OK) goto out;
    if (bo->sort && (rc = bs_reserve(bo, n_rec)) != ITX_OK) goto out;
    if (bo->ix && !bo->sort && (rc = itx_bamidx_reserve(bo->ix, bo->st, n_rec, total / BO_P)) != ITX_OK) goto out;
    ITX_TRY(hipMemcpyAsync(bo->d_pay + bo->carry, bytes, len, hipMemcpyHostToDevice, bo->st));
    if (bo->sort) ITX_TRY(hipMemcpyAsync(bo->d_sent + bo->n_sent, h_ent, sizeof(BoSortEnt) * n_rec, hipMemcpyHostToDevice, bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));                                  // the caller's bytes are its own again
    if (bo->ix && !bo->sort &&
        (rc = itx_bamidx_host_records(bo->ix, bo->st, bo->d_pay + bo->carry, h_off, (uint32_t)n_rec, bo->stream_base + bo->carry)) != ITX_OK)
        goto out;
    bo->stats.host_batches++;
    bo->stats.records += n_rec;
    bo->stats.payload_bytes += len;
    if (bo->sort) {                                                        // held whole: the entries stand in the pool in stream order
        bo->n_sent += n_rec;
        bo->host_bad += bad;
        if (maxtid > bo->host_maxtid) bo->host_maxtid = maxtid;
        bo->carry = (size_t)total;
    } else {
        rc = bo_emit(bo, total, 0);
    }
out:
    free(h_off);
    free(h_ent);
    return rc;
}

extern "C" int itx_bamout_finish(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_finish: bad argument");
        return ITX_E_ARG;
    }
    if (bo->finished) {
        itx_set_error("itx_bamout_finish: called twice");
        return ITX_E_STATE;
    }
    if (bo->sort) {
        itx_set_error("itx_bamout_finish: the stream is to be sorted (itx_bamout_sort_next)");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    ITX_TRY(hipSetDevice(bo->device));
    ITX_TRY(hipStreamSynchronize(bo->st));
    bo_read_gather_time(bo);
    if (bo->carry) {
        if ((rc = bo_reserve(bo, bo->carry, 1)) != ITX_OK) goto out;
        if (bo->ix && (rc = itx_bamidx_reserve(bo->ix, bo->st, 0, 1)) != ITX_OK) goto out;
        if ((rc = bo_emit(bo, bo->carry, 1)) != ITX_OK) goto out;
    }
    bo->finished = 1;
out:
    return rc;
}

extern "C" int itx_bamout_collect(itx_bamout *bo, itx_bamout_members *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_collect: bad argument");
        return ITX_E_ARG;
    }
    memset(out, 0, sizeof *out);
    if (!bo->pending) return ITX_OK;
    int rc = ITX_OK;
    float ms = 0;
    bo_slot *s = &bo->slot[bo->head];
    ITX_TRY(hipSetDevice(bo->device));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipEventSynchronize(s->e1));
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    if (hipEventElapsedTime(&ms, s->e0, s->e1) == hipSuccess) bo->stats.member_ms += (double)ms;    if (*s->h_total > s->cap) {
        itx_set_error("itx_bamout_collect: %llu packed bytes in a buffer of %zu", *s->h_total, s->cap);
        rc = ITX_E_LIMIT;
        goto out;
    }
    if (*s->h_total) {
        ITX_TRY(hipMemcpyAsync(s->h_pin, s->d_packed, (size_t)*s->h_total, hipMemcpyDeviceToHost, bo->cst));
        ITX_TRY(hipStreamSynchronize(bo->cst));
    }
    out->bytes = s->h_pin;
    out->len = *s->h_total;
    out->room = s->cap;
    out->n_members = s->n_mem;
    bo->stats.out_bytes += *s->h_total;
    s->busy = 0;
    bo->head ^= 1;
    bo->pending--;
out:
    return rc;
}

extern "C" int itx_bamout_pending(const itx_bamout *bo) { return bo ? bo->pending : 0; }

extern "C" int itx_bamout_get_stats(const itx_bamout *bo, itx_bamout_stats *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *out = bo->stats;
    out->carry = bo->carry;
    return ITX_OK;
}

// ---- filter -b -l: the level of the members
extern "C" int itx_bamout_set_level(itx_bamout *bo, int level)
{
    if (!bo || !ITX_BGZF_LEVEL_OK(level)) {
        itx_set_error("itx_bamout_set_level: %s", bo ? "the level is 0 (stored), 1 (fast) or 6 (the default)" : "bad argument");
        return ITX_E_ARG;
    }
    if (bo->level_set || bo->finished || bo->stats.batches || bo->stats.host_batches) {
        itx_set_error("itx_bamout_set_level: %s", bo->level_set ? "called twice" : "the stream has begun");
        return ITX_E_STATE;
    }
    bo->level = level;
    bo->level_set = 1;
    return ITX_OK;
}

extern "C" int itx_bamout_get_level(const itx_bamout *bo) { return bo ? bo->level : ITX_E_ARG; }

// ---- filter -b -a: the tags of the chosen row behind every counted record (csrc/itx_reptag.h)
// one name table's checks: offsets that ascend, no name of 2^16 bytes or more. Returns ITX_OK, ITX_E_ARG or ITX_E_LIMIT.
static int bo_check_names(const char *what, const uint64_t *off, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) {
            itx_set_error("itx_bamout_annotate_enable: the offsets of the %s names do not ascend (name %u)", what, i);
            return ITX_E_ARG;
        }
        if (off[i + 1] - off[i] > ITX_REPTAG_MAX_NAME) {
            itx_set_error("itx_bamout_annotate_enable: %s name %u has %llu bytes (a tag's name has at most %u)", what, i, (ull)(off[i + 1] - off[i]), ITX_REPTAG_MAX_NAME);
            return ITX_E_LIMIT;
        }
    }
    return ITX_OK;
}

extern "C" int itx_bamout_annotate_enable(itx_bamout *bo, const itx_row *rows, size_t n_rows, const char *rep_bytes, const uint64_t *rep_off, uint32_t n_rep,
                                          const char *cla_bytes, const uint64_t *cla_off, uint32_t n_cla, const char *fam_bytes, const uint64_t *fam_off, uint32_t n_fam)
{
    if (!bo || (n_rows && !rows) || !rep_bytes || !rep_off || !cla_bytes || !cla_off || !fam_bytes || !fam_off || n_rows >= 0x7fffffffull) {
        itx_set_error("itx_bamout_annotate_enable: bad argument");
        return ITX_E_ARG;
    }
    if (bo->annotate || bo->finished || bo->stats.batches || bo->stats.host_batches) {
        itx_set_error("itx_bamout_annotate_enable: %s", bo->annotate ? "called twice" : "the stream has begun");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    if ((rc = bo_check_names("repName", rep_off, n_rep)) != ITX_OK || (rc = bo_check_names("repClass", cla_off, n_cla)) != ITX_OK ||
        (rc = bo_check_names("repFamily", fam_off, n_fam)) != ITX_OK)
        return rc;
    for (size_t r = 0; r < n_rows; r++)
        if (rows[r].rep >= n_rep || rows[r].cla >= n_cla || rows[r].fam >= n_fam) {
            itx_set_error("itx_bamout_annotate_enable: row %zu names repName %u of %u, repClass %u of %u, repFamily %u of %u", r, rows[r].rep, n_rep, rows[r].cla, n_cla,
                          rows[r].fam, n_fam);
            return ITX_E_ARG;
        }
    // one block, laid out on the host and uploaded once: the three offset arrays (8-byte aligned), the rows, the three pools.
    // Offsets are rebased to the pool's first used byte, so a caller's off[0] need not be 0.
    const size_t o_rep = 0, o_cla = o_rep + 8 * ((size_t)n_rep + 1), o_fam = o_cla + 8 * ((size_t)n_cla + 1), o_rows = o_fam + 8 * ((size_t)n_fam + 1);
    const size_t b_rep = o_rows + 4 * (size_t)BO_ROW_WORDS * n_rows, b_cla = b_rep + (size_t)(rep_off[n_rep] - rep_off[0]);
    const size_t b_fam = b_cla + (size_t)(cla_off[n_cla] - cla_off[0]), bytes = b_fam + (size_t)(fam_off[n_fam] - fam_off[0]);
    uint8_t *h = (uint8_t *)malloc(bytes + 16), *d = nullptr;
    if (!h) {
        itx_set_error("itx_bamout_annotate_enable: no host memory for a table of %zu bytes", bytes);
        return ITX_E_NOMEM;
    }
    {
        const uint64_t *const offs[3] = {rep_off, cla_off, fam_off};
        const char *const pools[3] = {rep_bytes, cla_bytes, fam_bytes};
        const uint32_t ns[3] = {n_rep, n_cla, n_fam};
        const size_t at_off[3] = {o_rep, o_cla, o_fam}, at_bytes[3] = {b_rep, b_cla, b_fam};
        for (int t = 0; t < 3; t++) {
            ull *o = (ull *)(h + at_off[t]);
            for (uint32_t i = 0; i <= ns[t]; i++) o[i] = offs[t][i] - offs[t][0];
            if (o[ns[t]]) memcpy(h + at_bytes[t], pools[t] + offs[t][0], (size_t)o[ns[t]]);
        }
        uint32_t *w = (uint32_t *)(h + o_rows);
        for (size_t r = 0; r < n_rows; r++) {
            w[BO_ROW_WORDS * r] = rows[r].start;
            w[BO_ROW_WORDS * r + 1] = rows[r].end;
            w[BO_ROW_WORDS * r + 2] = rows[r].rep;
            w[BO_ROW_WORDS * r + 3] = rows[r].cla;
            w[BO_ROW_WORDS * r + 4] = rows[r].fam;
        }
    }
    ITX_TRY(hipSetDevice(bo->device));
    if (hipMalloc((void **)&d, bytes + 16) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_annotate_enable: no device memory for a table of %zu bytes", bytes);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));                 // (synchronous: the caller's arrays and h are free on return)
    bo->ann.rep_off = (const ull *)(d + o_rep);
    bo->ann.cla_off = (const ull *)(d + o_cla);
    bo->ann.fam_off = (const ull *)(d + o_fam);
    bo->ann.rows = (const uint32_t *)(d + o_rows);
    bo->ann.rep = d + b_rep;
    bo->ann.cla = d + b_cla;
    bo->ann.fam = d + b_fam;
    bo->ann.n_rows = (uint32_t)n_rows;
    bo->d_ann = d;
    bo->annotate = 1;
    d = nullptr;
out:
    (void)hipFree(d);                                                      // (the block that was not taken)
    free(h);
    return rc;
}

extern "C" int itx_bamout_annotate_get_stats(const itx_bamout *bo, uint64_t *tag_bytes)
{
    if (!bo || !tag_bytes) {
        itx_set_error("itx_bamout_annotate_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *tag_bytes = bo->tag_bytes;
    return ITX_OK;
}

// ---- filter -b -s: the stream held, sorted by coordinate and replayed
extern "C" int itx_bamout_sort_enable(itx_bamout *bo)
{
    if (!bo) {
        itx_set_error("itx_bamout_sort_enable: bad argument");
        return ITX_E_ARG;
    }
    if (bo->sort || bo->finished || bo->stats.batches || bo->stats.host_batches) {
        itx_set_error("itx_bamout_sort_enable: %s", bo->sort ? "called twice" : "the stream has begun");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    uint32_t *flag = nullptr, *h_flag = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ITX_TRY(hipSetDevice(bo->device));
    if (hipMalloc((void **)&flag, 16) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_sort_enable: no device memory (run without -s)");
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipHostMalloc((void **)&h_flag, 16, hipHostMallocDefault));
    ITX_TRY(hipMemset(flag, 0, 16));
    ITX_TRY(hipEventCreate(&ev[0]));
    ITX_TRY(hipEventCreate(&ev[1]));
    bo->d_sflag = flag;
    bo->h_sflag = h_flag;
    bo->sev[0] = ev[0];
    bo->sev[1] = ev[1];
    bo->sort = 1;
    return ITX_OK;
out:
    (void)hipFree(flag);
    if (h_flag) (void)hipHostFree(h_flag);
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

// the sort's device time is read once its events are through (the round's wait for its totals is behind them)
static void bs_read_sort_time(itx_bamout *bo)
{
    if (!bo->sort_timed) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, bo->sev[0], bo->sev[1]) == hipSuccess) bo->sort_ms += (double)ms;
    bo->sort_timed = 0;
}

// The first sort_next: the flags are read, the replay's buffers allocated, and the sort of the pool enqueued. bo->st is idle.
// Nothing of the object changes before every check has passed and every buffer is there.
static int bs_begin(itx_bamout *bo)
{
    int rc = ITX_OK;
    const uint32_t N = (uint32_t)bo->n_sent;
    uint2 *k0 = nullptr, *k1 = nullptr, *sorted = nullptr;
    uint32_t *hist = nullptr, n_ref = 0, high = 0;
    ull *soff = nullptr, bad = 0;
    uint8_t *npay = nullptr;
    const size_t pay_cap = 4 * (size_t)BO_P;
    ITX_TRY(hipMemcpyAsync(bo->h_sflag, bo->d_sflag, 8, hipMemcpyDeviceToHost, bo->st));
    ITX_TRY(hipStreamSynchronize(bo->st));
    bad = bo->host_bad + bo->h_sflag[0];
    if (bad) {
        itx_set_error("itx_bamout_sort_next: %llu counted records name no reference or no position (tid or pos below 0): they cannot be sorted by coordinate", bad);
        rc = ITX_E_LIMIT;
        goto out;
    }
    if (N) {
        if (hipMalloc((void **)&k0, 8 * (size_t)N) != hipSuccess || hipMalloc((void **)&k1, 8 * (size_t)N) != hipSuccess ||
            hipMalloc((void **)&hist, itx_sort_hist_bytes(N)) != hipSuccess || hipMalloc((void **)&soff, 8 * (bo->cap + 64)) != hipSuccess ||
            hipMalloc((void **)&npay, pay_cap + 16) != hipSuccess) {
            (void)hipGetLastError();
            itx_set_error("itx_bamout_sort_next: no device memory to sort %u records beside a held stream of %zu bytes (run without -s)", N, bo->carry);
            rc = ITX_E_NOMEM;
            goto out;
        }
        n_ref = bo->n_ref > 0 ? (uint32_t)bo->n_ref : 0u;
        {
            const uint32_t seen = (bo->h_sflag[1] > bo->host_maxtid ? bo->h_sflag[1] : bo->host_maxtid) + 1u;
            if (seen > n_ref) n_ref = seen;                                // (a tid beyond the header's list still finds its place)
        }
        high = itx_bamsort_high_passes(n_ref);
        ITX_TRY(hipEventRecord(bo->sev[0], bo->st));
        hipLaunchKernelGGL(k_bs_keys, dim3((N + 255u) / 256u), dim3(256), 0, bo->st, bo->d_sent, N, k0);
        ITX_TRY(hipGetLastError());
        // four passes by the low key; then the keys become the tids, and the shift starts again at 0
        if ((rc = itx_sort_run(bo->st, k0, k1, N, 0u, 4u, hist, &sorted)) != ITX_OK) goto out;
        if (high) {
            hipLaunchKernelGGL(k_bs_rekey, dim3((N + 255u) / 256u), dim3(256), 0, bo->st, bo->d_sent, N, sorted);
            ITX_TRY(hipGetLastError());
            if ((rc = itx_sort_run(bo->st, sorted, sorted == k0 ? k1 : k0, N, 0u, high, hist, &sorted)) != ITX_OK) goto out;
        }
        ITX_TRY(hipEventRecord(bo->sev[1], bo->st));
        bo->sort_timed = 1;
    }
    // the held stream is what d_pay was; the payload stream starts anew
    bo->d_held = bo->d_pay;
    bo->d_pay = npay;
    bo->pay_cap = npay ? pay_cap : 0;
    bo->carry = 0;
    bo->d_k0 = k0;
    bo->d_k1 = k1;
    bo->sorted = sorted;
    bo->d_hist = hist;
    bo->d_soff = soff;
    bo->sort = 2;
    return ITX_OK;
out:
    if (k0 || k1) (void)hipStreamSynchronize(bo->st);                      // (kernels that were enqueued before something failed)
    (void)hipFree(k0);
    (void)hipFree(k1);
    (void)hipFree(hist);
    (void)hipFree(soff);
    (void)hipFree(npay);
    return rc;
}

// the sort's work arrays and the held stream go (the kernels that read them are through)
static void bs_release(itx_bamout *bo)
{
    (void)hipFree(bo->d_held);
    (void)hipFree(bo->d_k0);
    (void)hipFree(bo->d_k1);
    (void)hipFree(bo->d_hist);
    (void)hipFree(bo->d_soff);
    (void)hipFree(bo->d_sent);
    bo->d_held = nullptr;
    bo->d_k0 = bo->d_k1 = bo->sorted = nullptr;
    bo->d_hist = nullptr;
    bo->d_soff = nullptr;
    bo->d_sent = nullptr;
    bo->sent_cap = 0;
}

extern "C" int itx_bamout_sort_next(itx_bamout *bo, int *more)
{
    if (!bo || !more) {
        itx_set_error("itx_bamout_sort_next: bad argument");
        return ITX_E_ARG;
    }
    *more = 0;
    if (!bo->sort || bo->finished) {
        itx_set_error("itx_bamout_sort_next: %s", bo->sort ? "the stream is finished" : "no sort was asked for (itx_bamout_sort_enable)");
        return ITX_E_STATE;
    }
    int rc = ITX_OK;
    float ms = 0;
    ull total = 0, n_mem = 0;
    const ull N = bo->n_sent;
    uint32_t n = 0, nt = 0;
    int last = 0;
    ITX_TRY(hipSetDevice(bo->device));
    ITX_TRY(hipStreamSynchronize(bo->st));
    bo_read_gather_time(bo);
    if (bo->sort == 1 && (rc = bs_begin(bo)) != ITX_OK) goto out;
    if (!N) {                                                              // nothing was counted: no member
        bs_release(bo);
        bo->finished = 1;
        goto out;
    }
    n = (uint32_t)(N - bo->sort_done < bo->cap ? N - bo->sort_done : bo->cap);
    nt = (n + BO_TILE - 1) / BO_TILE;
    last = bo->sort_done + n == N;
    ITX_TRY(hipEventRecord(bo->ev[0], bo->st));
    ITX_TRY(hipMemsetAsync(bo->d_tot, 0, 32, bo->st));
    hipLaunchKernelGGL(k_bs_lengths, dim3(nt), dim3(BO_TILE), 0, bo->st, bo->sorted + bo->sort_done, bo->d_sent, n, bo->d_len, bo->d_soff, bo->d_tile_sum);
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_tile_sum, nt, bo->d_tile_base, bo->d_tot);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(bo->ev[1], bo->st));
    ITX_TRY(hipMemcpyAsync(bo->h_tot, bo->d_tot, 32, hipMemcpyDeviceToHost, bo->st));
    {
        const double t0 = itx_wall_now();
        ITX_TRY(hipStreamSynchronize(bo->st));                              // (the members of the round before are through as well)
        bo->stats.wait_ms += 1e3 * (itx_wall_now() - t0);
    }
    bs_read_sort_time(bo);
    ITX_TRY(hipEventElapsedTime(&ms, bo->ev[0], bo->ev[1]));
    bo->replay_ms += (double)ms;
    total = (ull)bo->carry + bo->h_tot[0];
    n_mem = total / BO_P + (last && total % BO_P ? 1 : 0);
    if ((rc = bo_reserve(bo, total, n_mem)) != ITX_OK) goto out;
    if (bo->ix && (rc = itx_bamidx_reserve(bo->ix, bo->st, n, n_mem)) != ITX_OK) goto out;
    ITX_TRY(hipEventRecord(bo->ev[2], bo->st));
    // (under -a the held records are annotated already: the replay copies them byte for byte)
    hipLaunchKernelGGL((k_bo_gather<ull, false>), dim3(nt), dim3(BO_TILE), 0, bo->st, bo->d_held, bo->d_soff, n, bo->d_len, bo->d_tile_base, (ull)bo->carry, bo->d_pay,
                       (const int32_t *)nullptr, bo->ann);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(bo->ev[3], bo->st));
    bo->gather_timed = 1;
    if (bo->ix && (rc = itx_bamidx_entries64(bo->ix, bo->st, bo->d_held, bo->d_soff, n, bo->d_len, bo->d_tile_base, bo->stream_base + bo->carry, n)) != ITX_OK) goto out;
    bo->sort_done += n;
    bo->rounds++;
    if ((rc = bo_emit(bo, total, last)) != ITX_OK) goto out;
    if (last) {
        // the held stream goes as soon as the last gather (and the index's entry kernel behind it) has read it
        if (bo->ix) itx_bamidx_batch_time(bo->ix);
        ITX_TRY(hipEventSynchronize(bo->ev[3]));
        bo_read_gather_time(bo);
        bs_release(bo);
        bo->finished = 1;
    }
    *more = !last;
out:
    return rc;
}

extern "C" int itx_bamout_sort_get_stats(const itx_bamout *bo, itx_bamout_sort_stats *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_sort_get_stats: bad argument");
        return ITX_E_ARG;
    }
    out->records = bo->n_sent;
    out->rounds = bo->rounds;
    out->pool_grows = bo->sent_grows;
    out->sort_ms = bo->sort_ms;
    out->replay_ms = bo->replay_ms;
    return ITX_OK;
}

// ---- the .bai index of the stream (csrc/itx_bamidx.hip)
extern "C" int itx_bamout_index_enable(itx_bamout *bo, int32_t n_ref, const int32_t *l_ref)
{
    if (!bo || n_ref < 0 || (n_ref && !l_ref)) {
        itx_set_error("itx_bamout_index_enable: bad argument");
        return ITX_E_ARG;
    }
    if (bo->ix || bo->finished || bo->stats.batches || bo->stats.host_batches) {
        itx_set_error("itx_bamout_index_enable: %s", bo->ix ? "called twice" : "the stream has begun");
        return ITX_E_STATE;
    }
    const int rc = itx_bamidx_create(bo->device, n_ref, l_ref, &bo->ix);
    if (rc == ITX_OK) bo->n_ref = n_ref;
    return rc;
}

extern "C" int itx_bamout_index_finish(itx_bamout *bo, uint64_t first_member_offset, itx_bamout_index_result *out)
{
    if (!bo || !out) {
        itx_set_error("itx_bamout_index_finish: bad argument");
        return ITX_E_ARG;
    }
    if (!bo->ix || !bo->finished) {
        itx_set_error("itx_bamout_index_finish: %s", bo->ix ? "the stream is not finished (itx_bamout_finish)" : "no index was asked for (itx_bamout_index_enable)");
        return ITX_E_STATE;
    }
    if (first_member_offset >> 47) {
        itx_set_error("itx_bamout_index_finish: a first member at byte %llu", (ull)first_member_offset);
        return ITX_E_LIMIT;
    }
    return itx_bamidx_finish(bo->ix, bo->st, first_member_offset, out);
}
