// itx_bamidx.hip — the .bai index (SAM v1 section 5.2) of the BAM that `iteres filter -b -i` writes, built where the records lie and
// in the same pass (an extension, as -b is). csrc/itx_bairule.h states what a record contributes; this file collects it and
// makes the file's bytes. The BAM writer (csrc/itx_bamout*.hip) calls it (itx_bamidx.h) on its own stream.
//
// per batch, behind the gather:
//   k_bi_entries   one lane per record. A counted record (len != 0) walks its CIGAR where it lies and appends one entry
//                  {key = tid << 16 | bin, pos, end, its byte in the record stream, its length} to a pool in HBM; its place in the
//                  stream comes from the gather's own tile bases and itx_tile_offsets, its place in the pool from the tile's record
//                  count the same way. A record that cannot be indexed (itx_bai_refuses) sets a bit of the flag word.
//   the batch's member sizes are copied behind those of the batches before (device to device).
//   The host route's records (whole records one behind the other) are measured by k_bi_measure + k_tile_scan2 and go through the
//   SAME entry kernel, so the pool is one list in stream order whatever route a window took.
// at the end (itx_bamidx_finish), N entries, M members:
//   k_bi_order     entry i against entry i - 1: (tid, pos) below its predecessor's sets the "unsorted" bit. The flag word is read
//                  once, here; a set bit ends the work: status, no bytes.
//   k_size_scan    (itx_textpack.h) exclusive sums of ALL member sizes: coff[0 .. M]
//   k_bi_heads / k_tile_scan2 / k_bi_chunks   a run of consecutive entries with one key is one chunk: run heads are counted per
//                  tile, scanned, and every run writes (key, chunk number), its first voff and its last end voff
//   k_sort_*       (itx_radixsort.h) the chunks sorted by key, stable, so a bin's chunks stay in file order
//   k_bi_merge_count / k_tile_scan2 / k_bi_merge_apply   a chunk is merged into its predecessor when prev.end >> 16 >= beg >> 16
//                  (ends rise with the file order, so the predicate needs the neighbour only); the same scan numbers the bins; the
//                  first and last chunk and bin of every reference are noted where the key's tid changes
//   k_bi_windows   per entry, 64-bit atomicMin of its voff into every window it touches (windows its predecessor on the same
//                  reference touches too are skipped: that one's voff is lower); first and last entry of every reference
//   k_bi_fill      one workgroup per reference: n_intv, then untouched windows take the nearest touched value below (carried scan)
//   k_bi_refsize   one workgroup: the bytes of every reference's part, exclusive sums
//   k_bi_write_*   the file's bytes. Every field of a .bai lies on a 4-byte boundary, so 8-byte fields go as two 32-bit stores.
// The finished bytes come back through a page-locked buffer. The pools grow by the two-phase rule of itx_devbuf.h.
#include "itx_bamidx.h"
#include "itx_bairule.h"
#include "itx_devbuf.h"
#include "itx_radixsort.h"
#include "itx_textpack.h"

#include <stdlib.h>
#include <string.h>

typedef unsigned long long ull;

#define BI_TILE ITX_BAMIDX_TILE
#define BI_P ITX_BAMIDX_PAYLOAD
#define BI_NONE 0xffffffffffffffffull
#define BI_FLAG(reason) (1u << (reason))

struct BiEnt {
    uint32_t key;                    // tid << 16 | bin
    int32_t pos, end;
    uint32_t len;                    // 4 + block_size
    ull soff;                        // the record's first byte in the record stream of the whole run
};
static_assert(sizeof(BiEnt) == 24, "BiEnt");

// ---- per batch

// the host route: every record counts, 4 + block_size bytes (the host has checked that they are whole records)
__global__ __launch_bounds__(BI_TILE) void k_bi_measure(const uint8_t *__restrict__ u, const uint32_t *__restrict__ rec_off, uint32_t n, uint32_t *__restrict__ len_out,
                                                         ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_w[BI_TILE / 64u];
    const uint32_t i = blockIdx.x * BI_TILE + threadIdx.x;
    uint32_t len = 0, total = 0;
    if (i < n) {
        len = 4u + itx_bai_u32(u + rec_off[i]);
        len_out[i] = len;
    }
    (void)itx_tile_offsets<BI_TILE>(len, s_w, &total);
    if (threadIdx.x == 0) {
        const uint32_t left = n - blockIdx.x * BI_TILE;
        tile_sum[2u * blockIdx.x] = total;
        tile_sum[2u * blockIdx.x + 1u] = left < BI_TILE ? left : BI_TILE;
    }
}

// OFF: uint32_t offsets into a window or a host batch; 64-bit offsets into the held stream of filter -b -s (itx_bamout_sort_next)
template <class OFF>
__global__ __launch_bounds__(BI_TILE) void k_bi_entries(const uint8_t *__restrict__ u, const OFF *__restrict__ rec_off, uint32_t n, const uint32_t *__restrict__ len_in,
                                                         const ull *__restrict__ tile_base, ull stream_at, ull ent_at, BiEnt *__restrict__ ent, int32_t n_ref,
                                                         const int32_t *__restrict__ l_ref, uint32_t *__restrict__ flag)
{
    __shared__ uint32_t s_w[BI_TILE / 64u], s_c[BI_TILE / 64u];
    const uint32_t i = blockIdx.x * BI_TILE + threadIdx.x;
    const uint32_t len = i < n ? len_in[i] : 0u;
    uint32_t total = 0, count = 0;
    const uint32_t moff = itx_tile_offsets<BI_TILE>(len, s_w, &total);        // the gather's rule for the record's place
    const uint32_t rank = itx_tile_offsets<BI_TILE>(len ? 1u : 0u, s_c, &count);
    if (!len) return;
    const uint8_t *p = u + rec_off[i];
    ItxBaiRec r;
    // `len` is the record's length in the stream, which is what its chunk needs. Under filter -b -a that is the annotated length
    // while the bytes at p are the source record's: the fields are read inside the shorter of the two (equal without -a)
    const uint32_t src_len = 4u + itx_bai_u32(p);
    itx_bai_fields(p, src_len < len ? src_len : len, &r);
    const int why = itx_bai_refuses(&r, n_ref, l_ref);
    BiEnt e;
    e.pos = r.pos;
    e.len = len;
    e.soff = stream_at + tile_base[2u * blockIdx.x] + moff;
    if (why) {                                                             // no index will be made: the entry only keeps the pool's count right
        atomicOr(flag, BI_FLAG(why));
        e.key = itx_bai_key(r.tid, 0u);
        e.end = r.pos;
    } else {
        e.key = itx_bai_key(r.tid, itx_bai_reg2bin(r.pos, r.end));
        e.end = (int32_t)r.end;
    }
    ent[ent_at + tile_base[2u * blockIdx.x + 1u] + rank] = e;
}

// ---- at the end

__global__ __launch_bounds__(256) void k_bi_order(const BiEnt *__restrict__ ent, uint32_t n, uint32_t *__restrict__ flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0 || i >= n) return;
    const int32_t ta = (int32_t)(ent[i - 1].key >> 16), tb = (int32_t)(ent[i].key >> 16);
    if (tb < ta || (tb == ta && ent[i].pos < ent[i - 1].pos)) atomicOr(flag, BI_FLAG(ITX_BAI_UNSORTED));
}

__device__ __forceinline__ bool bi_run_head(const BiEnt *__restrict__ ent, uint32_t i) { return i == 0 || ent[i].key != ent[i - 1].key; }

__global__ __launch_bounds__(BI_TILE) void k_bi_heads(const BiEnt *__restrict__ ent, uint32_t n, ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_w[BI_TILE / 64u];
    const uint32_t i = blockIdx.x * BI_TILE + threadIdx.x;
    uint32_t total = 0;
    (void)itx_tile_offsets<BI_TILE>(i < n && bi_run_head(ent, i) ? 1u : 0u, s_w, &total);
    if (threadIdx.x == 0) {
        tile_sum[2u * blockIdx.x] = total;
        tile_sum[2u * blockIdx.x + 1u] = 0;
    }
}

// chunk c = the c-th run of equal keys: (key, c) for the sort, the voff of its first record, the end voff of its last
__global__ __launch_bounds__(BI_TILE) void k_bi_chunks(const BiEnt *__restrict__ ent, uint32_t n, const ull *__restrict__ tile_base, const uint64_t *__restrict__ coff,
                                                        uint64_t first, uint2 *__restrict__ ck, uint64_t *__restrict__ cbeg, uint64_t *__restrict__ cend)
{
    __shared__ uint32_t s_w[BI_TILE / 64u];
    const uint32_t i = blockIdx.x * BI_TILE + threadIdx.x;
    const bool head = i < n && bi_run_head(ent, i);
    uint32_t total = 0;
    const uint32_t before = itx_tile_offsets<BI_TILE>(head ? 1u : 0u, s_w, &total);
    if (i >= n) return;
    const uint32_t c = (uint32_t)tile_base[2u * blockIdx.x] + before + (head ? 1u : 0u) - 1u;     // the run this entry belongs to
    const BiEnt e = ent[i];
    if (head) {
        ck[c] = make_uint2(e.key, c);
        cbeg[c] = itx_bai_voff(first, coff, e.soff, BI_P);
    }
    if (i + 1u == n || ent[i + 1u].key != e.key) cend[c] = itx_bai_voff(first, coff, e.soff + e.len, BI_P);
}

// sorted chunk j opens a chunk of the file (it is not merged into its predecessor)
__device__ __forceinline__ bool bi_chunk_head(const uint2 *__restrict__ s, const uint64_t *__restrict__ cbeg, const uint64_t *__restrict__ cend, uint32_t j)
{
    if (j == 0) return true;
    const uint2 a = s[j - 1], b = s[j];
    return a.x != b.x || (cend[a.y] >> 16) < (cbeg[b.y] >> 16);
}

__global__ __launch_bounds__(BI_TILE) void k_bi_merge_count(const uint2 *__restrict__ s, uint32_t n, const uint64_t *__restrict__ cbeg, const uint64_t *__restrict__ cend,
                                                             ull *__restrict__ tile_sum)
{
    __shared__ uint32_t s_a[BI_TILE / 64u], s_b[BI_TILE / 64u];
    const uint32_t j = blockIdx.x * BI_TILE + threadIdx.x;
    const bool ch = j < n && bi_chunk_head(s, cbeg, cend, j), bh = j < n && (j == 0 || s[j].x != s[j - 1].x);
    uint32_t ta = 0, tb = 0;
    (void)itx_tile_offsets<BI_TILE>(ch ? 1u : 0u, s_a, &ta);
    (void)itx_tile_offsets<BI_TILE>(bh ? 1u : 0u, s_b, &tb);
    if (threadIdx.x == 0) {
        tile_sum[2u * blockIdx.x] = ta;
        tile_sum[2u * blockIdx.x + 1u] = tb;
    }
}

// per reference: chunks [f0, f1), bins [b0, b1), entries [e0, e1), n_intv; all zero for a reference without records
struct BiRefs {
    uint32_t *f0, *f1, *b0, *b1, *e0, *e1, *n_intv;
};

// file chunk f: fkey, fbin (its bin's number among all bins), fbeg, fend; bin b starts at file chunk bin_first[b]
__global__ __launch_bounds__(BI_TILE) void k_bi_merge_apply(const uint2 *__restrict__ s, uint32_t n, const uint64_t *__restrict__ cbeg, const uint64_t *__restrict__ cend,
                                                             const ull *__restrict__ tile_base, uint32_t *__restrict__ fkey, uint32_t *__restrict__ fbin,
                                                             uint64_t *__restrict__ fbeg, uint64_t *__restrict__ fend, uint32_t *__restrict__ bin_first, BiRefs R)
{
    __shared__ uint32_t s_a[BI_TILE / 64u], s_b[BI_TILE / 64u];
    const uint32_t j = blockIdx.x * BI_TILE + threadIdx.x;
    const bool ch = j < n && bi_chunk_head(s, cbeg, cend, j), bh = j < n && (j == 0 || s[j].x != s[j - 1].x);
    uint32_t ta = 0, tb = 0;
    const uint32_t fa = itx_tile_offsets<BI_TILE>(ch ? 1u : 0u, s_a, &ta);
    const uint32_t fb = itx_tile_offsets<BI_TILE>(bh ? 1u : 0u, s_b, &tb);
    if (j >= n) return;
    const uint32_t f = (uint32_t)tile_base[2u * blockIdx.x] + fa + (ch ? 1u : 0u) - 1u;          // the file chunk and the bin this
    const uint32_t b = (uint32_t)tile_base[2u * blockIdx.x + 1u] + fb + (bh ? 1u : 0u) - 1u;     // sorted chunk belongs to
    const uint2 me = s[j];
    const uint32_t tid = me.x >> 16;
    const bool last = j + 1u == n;
    if (ch) {
        fkey[f] = me.x;
        fbin[f] = b;
        fbeg[f] = cbeg[me.y];
    }
    if (last || bi_chunk_head(s, cbeg, cend, j + 1u)) fend[f] = cend[me.y];
    if (bh) bin_first[b] = f;
    if (last) bin_first[b + 1u] = f + 1u;
    if (j == 0 || (s[j - 1].x >> 16) != tid) {
        R.f0[tid] = f;
        R.b0[tid] = b;
    }
    if (last || (s[j + 1u].x >> 16) != tid) {
        R.f1[tid] = f + 1u;
        R.b1[tid] = b + 1u;
    }
}

__global__ __launch_bounds__(256) void k_bi_windows(const BiEnt *__restrict__ ent, uint32_t n, const uint64_t *__restrict__ coff, uint64_t first,
                                                    const uint64_t *__restrict__ woff, ull *__restrict__ lin, BiRefs R)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const BiEnt e = ent[i];
    const uint32_t tid = e.key >> 16;
    uint32_t w = itx_bai_win_first(e.pos);
    const uint32_t w1 = itx_bai_win_last(e.end);
    if (i != 0 && (ent[i - 1].key >> 16) == tid) {
        // the entry before starts no later and lies earlier in the file: the windows it touches too already hold a lower voff
        const uint32_t pw = itx_bai_win_last(ent[i - 1].end) + 1u;
        if (pw > w) w = pw;
    } else {
        R.e0[tid] = i;
    }
    if (i + 1u == n || (ent[i + 1u].key >> 16) != tid) R.e1[tid] = i + 1u;
    const ull v = itx_bai_voff(first, coff, e.soff, BI_P);
    ull *row = lin + woff[tid];
    for (; w <= w1; w++) atomicMin(&row[w], v);                            // (a spliced record may touch thousands: a loop, one lane)
}

// one workgroup per reference: n_intv = the highest touched window + 1; below it an untouched window takes the value of the
// nearest touched one below, 0 when there is none
__global__ __launch_bounds__(256) void k_bi_fill(const uint64_t *__restrict__ woff, ull *__restrict__ lin, uint32_t *__restrict__ n_intv)
{
    __shared__ uint32_t s_n;
    __shared__ int32_t s_idx[256];
    __shared__ ull s_val[256];
    const uint32_t t = threadIdx.x;
    ull *row = lin + woff[blockIdx.x];
    const uint32_t nw = (uint32_t)(woff[blockIdx.x + 1u] - woff[blockIdx.x]);
    if (t == 0) s_n = 0;
    __syncthreads();
    uint32_t top = 0;
    for (uint32_t w = t; w < nw; w += 256u)
        if (row[w] != BI_NONE) top = w + 1u;
    if (top) atomicMax(&s_n, top);
    __syncthreads();
    const uint32_t n = s_n;
    if (t == 0) n_intv[blockIdx.x] = n;
    ull carry = 0;
    for (uint32_t w0 = 0; w0 < n; w0 += 256u) {
        const uint32_t w = w0 + t;
        const ull v = w < n ? row[w] : BI_NONE;
        s_val[t] = v;
        s_idx[t] = v != BI_NONE ? (int32_t)t : -1;
        __syncthreads();
        for (uint32_t o = 1; o < 256u; o <<= 1) {                          // inclusive max scan: the nearest touched lane at or below
            const int32_t x = t >= o ? s_idx[t - o] : -1;
            __syncthreads();
            if (x > s_idx[t]) s_idx[t] = x;
            __syncthreads();
        }
        const int32_t mine = s_idx[t], end = s_idx[255];
        const ull out = mine >= 0 ? s_val[mine] : carry;
        if (w < n) row[w] = out;
        carry = end >= 0 ? s_val[end] : carry;
        __syncthreads();
    }
}

// roff[r]: where reference r's part starts in the file; roff[n_ref]: where n_no_coor stands (one workgroup)
__global__ __launch_bounds__(ITX_SCAN_WG) void k_bi_refsize(uint32_t n_ref, BiRefs R, uint64_t *__restrict__ roff)
{
    __shared__ uint64_t s[ITX_SCAN_WG];
    uint64_t lo, hi;
    itx_scan_chunk(n_ref, &lo, &hi);
    auto size = [&](uint64_t r) -> uint64_t {
        return 4ull + 8ull * (R.b1[r] - R.b0[r]) + 16ull * (R.f1[r] - R.f0[r]) + (R.e1[r] > R.e0[r] ? 40ull : 0ull) + 4ull + 8ull * R.n_intv[r];
    };
    uint64_t a = 0, total;
    for (uint64_t r = lo; r < hi; r++) a += size(r);
    uint64_t e = 8ull + itx_scan_wg(a, s, &total);
    for (uint64_t r = lo; r < hi; r++) {
        roff[r] = e;
        e += size(r);
    }
    if (threadIdx.x == 0) roff[n_ref] = 8ull + total;
}

__device__ __forceinline__ void bi_put32(uint8_t *out, uint64_t at, uint32_t v) { *reinterpret_cast<uint32_t *>(out + at) = v; }
__device__ __forceinline__ void bi_put64(uint8_t *out, uint64_t at, uint64_t v)
{
    bi_put32(out, at, (uint32_t)v);
    bi_put32(out, at + 4u, (uint32_t)(v >> 32));
}

// magic, n_ref, per reference n_bin, the pseudo-bin and n_intv, and n_no_coor at the end
__global__ __launch_bounds__(256) void k_bi_write_refs(uint32_t n_ref, BiRefs R, const uint64_t *__restrict__ roff, const BiEnt *__restrict__ ent,
                                                       const uint64_t *__restrict__ coff, uint64_t first, uint8_t *__restrict__ out)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r == 0) {
        bi_put32(out, 0, 0x01494142u);                                     // "BAI\1"
        bi_put32(out, 4, n_ref);
        bi_put64(out, roff[n_ref], 0);
    }
    if (r >= n_ref) return;
    const uint32_t nb = R.b1[r] - R.b0[r], nc = R.f1[r] - R.f0[r];
    const bool has = R.e1[r] > R.e0[r];
    uint64_t at = roff[r];
    bi_put32(out, at, nb + (has ? 1u : 0u));
    at += 4ull + 8ull * nb + 16ull * nc;
    if (has) {
        const BiEnt a = ent[R.e0[r]], b = ent[R.e1[r] - 1u];
        bi_put32(out, at, ITX_BAI_PSEUDO_BIN);
        bi_put32(out, at + 4u, 2u);
        bi_put64(out, at + 8u, itx_bai_voff(first, coff, a.soff, BI_P));
        bi_put64(out, at + 16u, itx_bai_voff(first, coff, b.soff + b.len, BI_P));
        bi_put64(out, at + 24u, (uint64_t)(R.e1[r] - R.e0[r]));
        bi_put64(out, at + 32u, 0);
        at += 40u;
    }
    bi_put32(out, at, R.n_intv[r]);
}

__global__ __launch_bounds__(256) void k_bi_write_chunks(const ull *__restrict__ tot, const uint32_t *__restrict__ fkey, const uint32_t *__restrict__ fbin,
                                                         const uint64_t *__restrict__ fbeg, const uint64_t *__restrict__ fend, const uint32_t *__restrict__ bin_first, BiRefs R,
                                                         const uint64_t *__restrict__ roff, uint8_t *__restrict__ out)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= tot[0]) return;
    const uint32_t key = fkey[f], tid = key >> 16, b = fbin[f];
    const uint64_t at = roff[tid] + 4ull + 8ull * (b - R.b0[tid] + 1u) + 16ull * (f - R.f0[tid]);
    if (bin_first[b] == f) {
        bi_put32(out, at - 8u, key & 0xffffu);
        bi_put32(out, at - 4u, bin_first[b + 1u] - f);
    }
    bi_put64(out, at, fbeg[f]);
    bi_put64(out, at + 8u, fend[f]);
}

__global__ __launch_bounds__(256) void k_bi_write_linear(BiRefs R, const uint64_t *__restrict__ roff, const uint64_t *__restrict__ woff, const ull *__restrict__ lin,
                                                         uint8_t *__restrict__ out)
{
    const uint32_t r = blockIdx.x, n = R.n_intv[r];
    const uint64_t at = roff[r] + 4ull + 8ull * (R.b1[r] - R.b0[r]) + 16ull * (R.f1[r] - R.f0[r]) + (R.e1[r] > R.e0[r] ? 40ull : 0ull) + 4ull;
    const ull *row = lin + woff[r];
    for (uint32_t w = threadIdx.x; w < n; w += 256u) bi_put64(out, at + 8ull * w, row[w]);
}

// ---- host side
struct itx_bamidx {
    int device;
    int reason;                      // ITX_BAI_TOO_MANY_REFS: there will be no index, nothing is collected
    int32_t n_ref;
    uint64_t *h_woff;                // [n_ref + 1] where every reference's windows start in the linear array (the host's heap)
    ItxBuf d_lref, d_woff, d_flag;
    ItxPin h_flag;
    ItxBuf d_ent, d_ms;              // BiEnt[n_ent], and all member sizes of the run: grown together and kept (ItxGrow), cap is theirs in bytes
    uint64_t n_ent, n_ms;
    ItxBuf d_hoff, d_hlen;           // the host route's offsets and lengths
    ItxBuf d_hts, d_htb, d_htot;
    ItxEvent eb[2], ef[2];
    int batch_timed, done;
    double batch_ms, finish_ms;
    uint64_t grows;
    ItxBuf d_out;                    // the finished file
    ItxPin h_out;
};

void itx_bamidx_destroy(itx_bamidx *ix)
{
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    free(ix->h_woff);
    delete ix;
}

int itx_bamidx_create(int device, int32_t n_ref, const int32_t *l_ref, itx_bamidx **out)
{
    int rc = ITX_OK;
    const char *const who = "itx_bamout_index_enable";
    itx_bamidx *ix = new itx_bamidx();
    ix->device = device;
    ix->n_ref = n_ref;
    if (n_ref >= ITX_BAI_MAX_REFS) {
        ix->reason = ITX_BAI_TOO_MANY_REFS;
        *out = ix;
        return ITX_OK;
    }
    ix->h_woff = (uint64_t *)malloc(8 * ((size_t)n_ref + 1));
    if (!ix->h_woff) {
        itx_set_error("itx_bamout_index_enable: no memory for %d references", n_ref);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ix->h_woff[0] = 0;
    for (int32_t r = 0; r < n_ref; r++) ix->h_woff[r + 1] = ix->h_woff[r] + itx_bai_windows(l_ref[r]);
    ITX_TRY(hipSetDevice(device));
    if ((rc = itx_buf_need(who, ix->d_lref, 4 * ((size_t)n_ref + 1))) || (rc = itx_buf_need(who, ix->d_woff, 8 * ((size_t)n_ref + 1))) ||
        (rc = itx_buf_need(who, ix->d_flag, 16))) {
        itx_set_error("itx_bamout_index_enable: no device memory for %d references", n_ref);
        goto out;
    }
    if ((rc = itx_pin_need(who, ix->h_flag, 16)) != ITX_OK) goto out;
    if (n_ref) ITX_TRY(hipMemcpy(ix->d_lref.p, l_ref, 4 * (size_t)n_ref, hipMemcpyHostToDevice));
    ITX_TRY(hipMemcpy(ix->d_woff.p, ix->h_woff, 8 * ((size_t)n_ref + 1), hipMemcpyHostToDevice));
    ITX_TRY(hipMemset(ix->d_flag.p, 0, 16));
    for (auto *ev : {ix->eb, ix->ef})
        for (int k = 0; k < 2; k++)
            if ((rc = itx_event_make(ev[k])) != ITX_OK) goto out;
out:
    if (rc != ITX_OK) {
        itx_bamidx_destroy(ix);
        return rc;
    }
    *out = ix;
    return ITX_OK;
}

int itx_bamidx_reserve(itx_bamidx *ix, hipStream_t st, uint64_t n_entries, uint64_t n_members)
{
    if (ix->reason) return ITX_OK;
    uint64_t want_ent = 0, want_ms = 0;
    if (ix->n_ent + n_entries > 0xffffff00ull) {
        itx_set_error("itx_bamout: %llu records to index", (ull)(ix->n_ent + n_entries));
        return ITX_E_LIMIT;
    }
    if (ix->n_ent + n_entries > ix->d_ent.cap / sizeof(BiEnt)) want_ent = ix->n_ent + n_entries + (ix->n_ent + n_entries) / 2 + 1024;
    if (ix->n_ms + n_members > ix->d_ms.cap / 4) want_ms = ix->n_ms + n_members + (ix->n_ms + n_members) / 2 + 1024;
    const bool first = !ix->d_ent.p;
    // the entries and the member sizes are taken together (itx_devbuf.h); what they hold is kept
    ItxGrow g[2] = {{&ix->d_ent.p, sizeof(BiEnt) * ix->n_ent, sizeof(BiEnt) * want_ent}, {&ix->d_ms.p, 4 * ix->n_ms, 4 * want_ms}};
    if (itx_grow_alloc(g, 2) >= 0) {
        itx_set_error("itx_bamout: no device memory for the index entries of %llu records and %llu members", (ull)(ix->n_ent + n_entries), (ull)(ix->n_ms + n_members));
        return ITX_E_NOMEM;
    }
    const int rc = itx_grow_commit(st, g, 2);
    if (rc != ITX_OK) return rc;
    if (want_ent) {
        ix->d_ent.cap = sizeof(BiEnt) * want_ent;
        if (!first) ix->grows++;
    }
    if (want_ms) ix->d_ms.cap = 4 * want_ms;
    return ITX_OK;
}

template <class OFF>
static int bi_entries(itx_bamidx *ix, hipStream_t st, const uint8_t *u, const OFF *rec_off, uint32_t n, const uint32_t *len_in, const ull *tile_base, ull stream_at,
                      uint64_t n_counted)
{
    if (ix->reason || !n || !n_counted) return ITX_OK;
    int rc = ITX_OK;
    if (ix->n_ent + n_counted > ix->d_ent.cap / sizeof(BiEnt)) {
        itx_set_error("itx_bamidx_entries: no room was reserved");
        return ITX_E_STATE;
    }
    ITX_TRY(hipEventRecord(ix->eb[0], st));
    hipLaunchKernelGGL((k_bi_entries<OFF>), dim3((n + BI_TILE - 1) / BI_TILE), dim3(BI_TILE), 0, st, u, rec_off, n, len_in, tile_base, stream_at, (ull)ix->n_ent,
                       ix->d_ent.as<BiEnt>(), ix->n_ref, ix->d_lref.as<int32_t>(), ix->d_flag.as<uint32_t>());
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipEventRecord(ix->eb[1], st));
    ix->batch_timed = 1;
    ix->n_ent += n_counted;
out:
    return rc;
}

int itx_bamidx_entries(itx_bamidx *ix, hipStream_t st, const uint8_t *u, const uint32_t *rec_off, uint32_t n, const uint32_t *len_in, const ull *tile_base,
                       ull stream_at, uint64_t n_counted)
{
    return bi_entries(ix, st, u, rec_off, n, len_in, tile_base, stream_at, n_counted);
}

int itx_bamidx_entries64(itx_bamidx *ix, hipStream_t st, const uint8_t *u, const ull *rec_off, uint32_t n, const uint32_t *len_in, const ull *tile_base, ull stream_at,
                         uint64_t n_counted)
{
    return bi_entries(ix, st, u, rec_off, n, len_in, tile_base, stream_at, n_counted);
}

int itx_bamidx_host_records(itx_bamidx *ix, hipStream_t st, const uint8_t *d_bytes, const uint32_t *h_off, uint32_t n, ull stream_at)
{
    if (ix->reason || !n) return ITX_OK;
    int rc = ITX_OK;
    const uint32_t nt = (n + BI_TILE - 1) / BI_TILE;
    if (n > ix->d_hoff.cap / 4) {
        const uint64_t want = (uint64_t)n + n / 2 + 1024, wt = (want + BI_TILE - 1) / BI_TILE + 1;
        // the offsets, the lengths, the tiles' sums and bases and the totals are taken together; nothing is kept (st is idle: nothing reads them)
        ItxGrow g[5] = {{&ix->d_hoff.p, 0, 4 * want}, {&ix->d_hlen.p, 0, 4 * want}, {&ix->d_hts.p, 0, 16 * wt}, {&ix->d_htb.p, 0, 16 * wt}, {&ix->d_htot.p, 0, 16}};
        if (itx_grow_alloc(g, 5) >= 0) {
            itx_set_error("itx_bamout_append_host: no device memory for the offsets of %u records", n);
            return ITX_E_NOMEM;
        }
        if ((rc = itx_grow_commit(st, g, 5)) != ITX_OK) goto out;
        ix->d_hoff.cap = ix->d_hlen.cap = 4 * want, ix->d_hts.cap = ix->d_htb.cap = 16 * wt, ix->d_htot.cap = 16;
    }
    ITX_TRY(hipMemcpyAsync(ix->d_hoff.p, h_off, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    ITX_TRY(hipStreamSynchronize(st));
    hipLaunchKernelGGL(k_bi_measure, dim3(nt), dim3(BI_TILE), 0, st, d_bytes, ix->d_hoff.as<uint32_t>(), n, ix->d_hlen.as<uint32_t>(), ix->d_hts.as<ull>());
    ITX_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, ix->d_hts.as<ull>(), nt, ix->d_htb.as<ull>(), ix->d_htot.as<ull>());
    ITX_TRY(hipGetLastError());
    rc = itx_bamidx_entries(ix, st, d_bytes, ix->d_hoff.as<uint32_t>(), n, ix->d_hlen.as<uint32_t>(), ix->d_htb.as<ull>(), stream_at, n);
out:
    return rc;
}

int itx_bamidx_members(itx_bamidx *ix, hipStream_t st, const uint32_t *d_msize, uint32_t n)
{
    if (ix->reason || !n) return ITX_OK;
    int rc = ITX_OK;
    if (ix->n_ms + n > ix->d_ms.cap / 4) {
        itx_set_error("itx_bamidx_members: no room was reserved");
        return ITX_E_STATE;
    }
    ITX_TRY(hipMemcpyAsync(ix->d_ms.as<uint32_t>() + ix->n_ms, d_msize, 4 * (size_t)n, hipMemcpyDeviceToDevice, st));
    ix->n_ms += n;
out:
    return rc;
}

void itx_bamidx_batch_time(itx_bamidx *ix)
{
    if (!ix->batch_timed) return;
    float ms = 0;
    if (hipEventSynchronize(ix->eb[1]) == hipSuccess && hipEventElapsedTime(&ms, ix->eb[0], ix->eb[1]) == hipSuccess) ix->batch_ms += (double)ms;
    ix->batch_timed = 0;
}

static uint32_t bi_sort_passes(int32_t n_ref)
{
    uint32_t bits = 16;
    for (uint32_t v = n_ref > 0 ? (uint32_t)n_ref - 1u : 0u; v; v >>= 1) bits++;
    return (bits + 7u) / 8u;
}

int itx_bamidx_finish(itx_bamidx *ix, hipStream_t st, uint64_t first, itx_bamout_index_result *res)
{
    memset(res, 0, sizeof *res);
    if (ix->done) {
        itx_set_error("itx_bamout_index_finish: called twice");
        return ITX_E_STATE;
    }
    if (ix->reason) {
        res->status = ix->reason;
        ix->done = 1;
        return ITX_OK;
    }
    int rc = ITX_OK;
    const uint32_t N = (uint32_t)ix->n_ent, ntN = (N + BI_TILE - 1) / BI_TILE, n_ref = (uint32_t)ix->n_ref;
    const uint64_t M = ix->n_ms, W = ix->h_woff[n_ref];
    uint32_t C = 0, ntC = 0;
    float ms = 0;
    uint64_t total = 0;
    // work arrays: the views the kernels take, and their owners
    ItxBuf coff, cbeg, cend, fbeg, fend, roff, ts, tb, tot, lin, k0, k1, hist, fkey, fbin, binfirst, refs;
    ItxPin tot_pin;
    const char *const who = "itx_bamout_index_finish";
    BiEnt *const d_ent = ix->d_ent.as<BiEnt>();
    uint32_t *const d_flag = ix->d_flag.as<uint32_t>(), *const h_flag = ix->h_flag.as<uint32_t>();
    uint64_t *const d_woff = ix->d_woff.as<uint64_t>();
    uint8_t *d_out = nullptr;
    uint64_t *d_coff = nullptr, *d_cbeg = nullptr, *d_cend = nullptr, *d_fbeg = nullptr, *d_fend = nullptr, *d_roff = nullptr;
    ull *d_ts = nullptr, *d_tb = nullptr, *d_tot = nullptr, *d_lin = nullptr, *h_tot = nullptr;
    uint2 *d_k0 = nullptr, *d_k1 = nullptr, *sorted = nullptr;
    uint32_t *d_hist = nullptr, *d_fkey = nullptr, *d_fbin = nullptr, *d_binfirst = nullptr, *d_refs = nullptr;
    BiRefs R = {};
    ITX_TRY(hipSetDevice(ix->device));
    ITX_TRY(hipEventRecord(ix->ef[0], st));
    if (N) {
        hipLaunchKernelGGL(k_bi_order, dim3((N + 255u) / 256u), dim3(256), 0, st, d_ent, N, d_flag);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    ITX_TRY(hipStreamSynchronize(st));
    itx_bamidx_batch_time(ix);
    res->entries = N;
    res->grows = ix->grows;
    res->batch_ms = ix->batch_ms;
    if (*h_flag) {
        const uint32_t f = *h_flag;
        res->status = f & BI_FLAG(ITX_BAI_UNSORTED) ? ITX_BAI_UNSORTED : f & BI_FLAG(ITX_BAI_BEYOND_MAX) ? ITX_BAI_BEYOND_MAX : ITX_BAI_BEYOND_REF;
        ix->done = 1;
        goto out;
    }
    if ((rc = itx_buf_need(who, coff, 8 * (M + 1))) || (rc = itx_buf_need(who, ts, 16 * ((size_t)ntN + 1))) || (rc = itx_buf_need(who, tb, 16 * ((size_t)ntN + 1))) ||
        (rc = itx_buf_need(who, tot, 16)) || (rc = itx_buf_need(who, lin, 8 * (W + 1))) || (rc = itx_buf_need(who, refs, 4 * 7 * ((size_t)n_ref + 1))) ||
        (rc = itx_buf_need(who, roff, 8 * ((size_t)n_ref + 1))) || (rc = itx_pin_need(who, tot_pin, 16))) {
        itx_set_error("itx_bamout_index_finish: no memory for %u entries, %llu members and %llu windows", N, (ull)M, (ull)W);
        goto out;
    }
    d_coff = coff.as<uint64_t>(), d_roff = roff.as<uint64_t>(), d_refs = refs.as<uint32_t>();
    d_ts = ts.as<ull>(), d_tb = tb.as<ull>(), d_tot = tot.as<ull>(), d_lin = lin.as<ull>(), h_tot = tot_pin.as<ull>();
    R.f0 = d_refs;
    R.f1 = d_refs + 1 * ((size_t)n_ref + 1);
    R.b0 = d_refs + 2 * ((size_t)n_ref + 1);
    R.b1 = d_refs + 3 * ((size_t)n_ref + 1);
    R.e0 = d_refs + 4 * ((size_t)n_ref + 1);
    R.e1 = d_refs + 5 * ((size_t)n_ref + 1);
    R.n_intv = d_refs + 6 * ((size_t)n_ref + 1);
    ITX_TRY(hipMemsetAsync(d_refs, 0, 4 * 7 * ((size_t)n_ref + 1), st));
    ITX_TRY(hipMemsetAsync(d_lin, 0xff, 8 * (W + 1), st));
    ITX_TRY(hipMemsetAsync(d_tot, 0, 16, st));
    hipLaunchKernelGGL(k_size_scan, dim3(1), dim3(ITX_SCAN_WG), 0, st, ix->d_ms.as<uint32_t>(), M, d_coff);
    ITX_TRY(hipGetLastError());
    if (N) {
        hipLaunchKernelGGL(k_bi_heads, dim3(ntN), dim3(BI_TILE), 0, st, d_ent, N, d_ts);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, d_ts, ntN, d_tb, d_tot);
        ITX_TRY(hipGetLastError());
        ITX_TRY(hipMemcpyAsync(h_tot, d_tot, 16, hipMemcpyDeviceToHost, st));
        ITX_TRY(hipStreamSynchronize(st));                                  // the number of chunks sizes what follows
        C = (uint32_t)h_tot[0];
        ntC = (C + BI_TILE - 1) / BI_TILE;
        if ((rc = itx_buf_need(who, cbeg, 8 * (size_t)C)) || (rc = itx_buf_need(who, cend, 8 * (size_t)C)) || (rc = itx_buf_need(who, fbeg, 8 * (size_t)C)) ||
            (rc = itx_buf_need(who, fend, 8 * (size_t)C)) || (rc = itx_buf_need(who, k0, 8 * (size_t)C)) || (rc = itx_buf_need(who, k1, 8 * (size_t)C)) ||
            (rc = itx_buf_need(who, hist, itx_sort_hist_bytes(C))) || (rc = itx_buf_need(who, fkey, 4 * (size_t)C)) || (rc = itx_buf_need(who, fbin, 4 * (size_t)C)) ||
            (rc = itx_buf_need(who, binfirst, 4 * ((size_t)C + 1)))) {
            itx_set_error("itx_bamout_index_finish: no device memory for %u chunks", C);
            goto out;
        }
        d_cbeg = cbeg.as<uint64_t>(), d_cend = cend.as<uint64_t>(), d_fbeg = fbeg.as<uint64_t>(), d_fend = fend.as<uint64_t>();
        d_k0 = k0.as<uint2>(), d_k1 = k1.as<uint2>(), d_hist = hist.as<uint32_t>();
        d_fkey = fkey.as<uint32_t>(), d_fbin = fbin.as<uint32_t>(), d_binfirst = binfirst.as<uint32_t>();
        hipLaunchKernelGGL(k_bi_chunks, dim3(ntN), dim3(BI_TILE), 0, st, d_ent, N, d_tb, d_coff, first, d_k0, d_cbeg, d_cend);
        ITX_TRY(hipGetLastError());
        if ((rc = itx_sort_run(st, d_k0, d_k1, C, 0u, bi_sort_passes(ix->n_ref), d_hist, &sorted)) != ITX_OK) goto out;
        hipLaunchKernelGGL(k_bi_merge_count, dim3(ntC), dim3(BI_TILE), 0, st, sorted, C, d_cbeg, d_cend, d_ts);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_tile_scan2, dim3(1), dim3(ITX_SCAN_WG), 0, st, d_ts, ntC, d_tb, d_tot);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bi_merge_apply, dim3(ntC), dim3(BI_TILE), 0, st, sorted, C, d_cbeg, d_cend, d_tb, d_fkey, d_fbin, d_fbeg, d_fend, d_binfirst, R);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bi_windows, dim3((N + 255u) / 256u), dim3(256), 0, st, d_ent, N, d_coff, first, d_woff, d_lin, R);
        ITX_TRY(hipGetLastError());
    }
    if (n_ref) {
        hipLaunchKernelGGL(k_bi_fill, dim3(n_ref), dim3(256), 0, st, d_woff, d_lin, R.n_intv);
        ITX_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_bi_refsize, dim3(1), dim3(ITX_SCAN_WG), 0, st, n_ref, R, d_roff);
    ITX_TRY(hipGetLastError());
    ITX_TRY(hipMemcpyAsync(h_tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    ITX_TRY(hipMemcpyAsync(h_flag + 2, d_roff + n_ref, 8, hipMemcpyDeviceToHost, st));
    ITX_TRY(hipStreamSynchronize(st));                                      // the file's size
    memcpy(&total, h_flag + 2, 8);
    total += 8;
    if ((rc = itx_buf_need(who, ix->d_out, total)) || (rc = itx_pin_need(who, ix->h_out, total))) {
        itx_set_error("itx_bamout_index_finish: no memory for an index of %llu bytes", (ull)total);
        goto out;
    }
    d_out = ix->d_out.as<uint8_t>();
    hipLaunchKernelGGL(k_bi_write_refs, dim3(n_ref / 256u + 1u), dim3(256), 0, st, n_ref, R, d_roff, d_ent, d_coff, first, d_out);
    ITX_TRY(hipGetLastError());
    if (C) {
        hipLaunchKernelGGL(k_bi_write_chunks, dim3(ntC), dim3(256), 0, st, d_tot, d_fkey, d_fbin, d_fbeg, d_fend, d_binfirst, R, d_roff, d_out);
        ITX_TRY(hipGetLastError());
    }
    if (n_ref) {
        hipLaunchKernelGGL(k_bi_write_linear, dim3(n_ref), dim3(256), 0, st, R, d_roff, d_woff, d_lin, d_out);
        ITX_TRY(hipGetLastError());
    }
    ITX_TRY(hipMemcpyAsync(ix->h_out.p, d_out, total, hipMemcpyDeviceToHost, st));
    ITX_TRY(hipEventRecord(ix->ef[1], st));
    ITX_TRY(hipStreamSynchronize(st));
    if (hipEventElapsedTime(&ms, ix->ef[0], ix->ef[1]) == hipSuccess) ix->finish_ms = (double)ms;
    res->bytes = ix->h_out.as<uint8_t>();
    res->len = total;
    res->chunks = C ? h_tot[0] : 0;
    res->finish_ms = ix->finish_ms;
    ix->done = 1;
out:
    return rc;                                                              // (a finish that failed is not done; the next one sizes d_out, h_out again)
}
