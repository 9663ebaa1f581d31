// itx_bamout_members.hip — the BAM writer's last step (itx_bamout.hip has the whole path): a stream of payload bytes in d_pay
// becomes BGZF members, packed one behind the other in a slot that itx_bamout_collect hands out.
//   k_bo_member     one wave per whole payload: the payload into LDS, itx_bgzf_member into the member's slot (a fixed stride).
//                   After itx_bamout_set_level (filter -b -l) k_bo_member_stored (level 0) or k_bo_member_fast (level 1) stands in
//                   its place (itx_bgzflevels.h), in the same launch shape; nothing behind it knows the level.
//   k_size_scan     (itx_textpack.h) exclusive sums of the member sizes, one workgroup
//   k_pack_blocks   (itx_textpack.h) the members one behind the other
//   then the stream's rest, less than one payload, moves to its front (device to device), and the packed total to the host.
// With an index the batch's member sizes go to it behind the member kernel (itx_bamidx_members).
//
// k_bo_member is bound by the encoder's serial parse (one lane per member); ITX_BAMOUT_PAYLOAD is chosen for that
// (itx_bgzfmember.h). k_bo_member and k_bo_member_fast keep the 144 bytes of scratch per lane that itxd_huff's serial tail costs
// every user of the core; the stored level uses none (DESIGN.md has the figures).
#include "itx_bamout_priv.h"
#include "itx_bgzflevels.h"
#include "itx_textpack.h"

// payload `m` of the stream into LDS as little-endian words, zero beyond its n bytes; returns n. Payload m is
// pay[m * BO_P, min((m + 1) * BO_P, total)); pay is 16-byte aligned and BO_P a multiple of 16.
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

// one wave per member, level 6
__global__ __launch_bounds__(64) void k_bo_member(const uint8_t *__restrict__ pay, ull total, uint8_t *__restrict__ mem, uint32_t *__restrict__ msize)
{
    __shared__ ItxdLds<BO_P> s;
    const uint32_t n = bo_load_payload(pay, total, s.in);
    const uint32_t z = itx_bgzf_member(ws_of(s), n, mem + (ull)blockIdx.x * BO_STRIDE, threadIdx.x, 64);
    if (threadIdx.x == 0) msize[blockIdx.x] = z;
}

// ---- filter -b -l: the other levels of the members (itx_bgzflevels.h), in k_bo_member's launch shape
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

// LDS of the fast level's encoder: the member's staging area over the hash heads (dead when it is first written), which is 32
// bytes longer than they are, and the slices' bit counts
struct BoLdsFast : ItxdLds<BO_P, BO_STAGE_WORDS> {
    uint32_t sbits[ITXF_SLICES(BO_P) + 1];
};
static_assert(BO_STAGE_WORDS >= (1u << ITXD_HBITS), "the staging area holds the hash heads");
static_assert(3u * sizeof(BoLdsFast) <= 160u * 1024u, "three members in flight per CU, as k_bo_member");

// level 1: every stage of the encoder on all 64 lanes (itx_deflate_fast.h)
__global__ __launch_bounds__(64) void k_bo_member_fast(const uint8_t *__restrict__ pay, ull total, uint8_t *__restrict__ mem, uint32_t *__restrict__ msize)
{
    __shared__ BoLdsFast s;
    const uint32_t n = bo_load_payload(pay, total, s.in);
    const itxf_ws w = {ws_of(s), s.head, s.sbits};
    const uint32_t z = itx_bgzf_member_level(w, n, mem + (ull)blockIdx.x * BO_STRIDE, threadIdx.x, 64, 1u);
    if (threadIdx.x == 0) msize[blockIdx.x] = z;
}

int bo_emit(itx_bamout *bo, ull total, int with_tail)
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
        hipLaunchKernelGGL(k_size_scan, dim3(1), dim3(ITX_SCAN_WG), 0, bo->st, bo->d_msize, (uint64_t)n_mem, bo->d_moff);
        ITX_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pack_blocks, dim3(n_mem), dim3(256), 0, bo->st, bo->d_mem, (const uint64_t *)nullptr, BO_STRIDE, bo->d_msize, bo->d_moff, s->d_packed);
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

// ---- filter -b -l: the level of the members
extern "C" int itx_bamout_set_level(itx_bamout *bo, int level)
{
    if (!bo || !ITX_BGZF_LEVEL_OK(level)) {
        itx_set_error("itx_bamout_set_level: %s", bo ? "the level is 0 (stored), 1 (fast) or 6 (the default)" : "bad argument");
        return ITX_E_ARG;
    }
    if (bo_not_begun(bo, "itx_bamout_set_level", bo->level_set) != ITX_OK) return ITX_E_STATE;
    bo->level = level;
    bo->level_set = 1;
    return ITX_OK;
}

extern "C" int itx_bamout_get_level(const itx_bamout *bo) { return bo ? bo->level : ITX_E_ARG; }
