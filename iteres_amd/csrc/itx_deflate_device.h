// itx_deflate_device.h — device only: the encoder of itx_deflate_core.h as a kernel takes it. The ITXD_* hooks of the device are
// defined here and nowhere else (those of itx_deflate_fast.h included, so a file may include that header behind this one), and
// the LDS one block's encoder works in is one struct. The bigWig builders (itx_bwblock.h) and the BAM's members
// (itx_bamout_members.hip) are its users; the host builds under tests/ define their own hooks.
#pragma once
#include "itx_device.h"

#define ITXD_FN __device__ static inline
#define ITXD_SYNC() __syncthreads()
#define ITXD_AMAX(p, v) atomicMax((p), (v))
#define ITXD_CTZ(x) ((uint32_t)__builtin_ctz(x))
#define ITXD_AADD(p, v) ((void)atomicAdd((p), (v)))
#define ITXD_AOR(p, v) ((void)atomicOr((p), (v)))
#include "itx_deflate_core.h"

// LDS of one block's encoder (itxd_ws), sized for inputs of up to MAXN bytes. HEAD_WORDS: the hash heads, or a longer array that
// holds them and is something else once they are dead (the fast level's staging area).
template <uint32_t MAXN, uint32_t HEAD_WORDS = 1u << ITXD_HBITS>
struct ItxdLds {
    uint32_t in[MAXN / 4 + 4];
    uint32_t head[HEAD_WORDS];
    uint16_t md[MAXN];
    uint8_t ml[MAXN];
    uint32_t fq[ITXD_NSYM], key[ITXD_NSYM];
    uint16_t srt[ITXD_NSYM], code[ITXD_NSYM];
    uint8_t len[ITXD_NSYM];
    uint32_t clfq[20];
    uint16_t clcode[20];
    uint8_t cllen[20];
    uint64_t red[128];
    uint32_t misc[16];
};

template <uint32_t MAXN, uint32_t HEAD_WORDS>
__device__ static inline itxd_ws ws_of(ItxdLds<MAXN, HEAD_WORDS> &s)
{
    return itxd_ws{s.in, s.head, s.ml, s.md, s.fq, s.key, s.srt, s.len, s.code, s.clfq, s.cllen, s.clcode, s.red, s.misc};
}
