// Host build of the BGZF member rule (iteres_amd/csrc/itx_bgzfmember.h over itx_deflate_core.h) with a one-lane "wave" and plain
// arrays for its workspace: test infrastructure — the CPU suite holds it to zlib, the GPU suite holds the device's bytes to it.
#include <stdint.h>
#include <string.h>
#define ITXD_FN static inline
#define ITXD_SYNC() ((void)0)
#define ITXD_AMAX(p, v) ((void)(*(p) = *(p) > (v) ? *(p) : (v)))
#define ITXD_CTZ(x) ((uint32_t)__builtin_ctz(x))
#include "../iteres_amd/csrc/itx_bgzfmember.h"

static thread_local uint32_t in[ITXD_MAX_IN / 4 + 4];

static void load(const uint8_t *src, uint32_t n)
{
    memset(in, 0, sizeof in);
    if (n) memcpy(in, src, n);
}

extern "C" uint32_t itx_bamout_payload_host(void) { return ITX_BAMOUT_PAYLOAD; }
extern "C" uint32_t itx_bgzf_member_cap_host(uint32_t n) { return ITX_BGZF_MEMBER_CAP(n); }

// n (<= 32768) payload bytes at src -> the member at dst (room: ITX_BGZF_MEMBER_CAP(n)); returns its size, 0 for a payload too long
extern "C" uint32_t itx_bgzf_member_host(const uint8_t *src, uint32_t n, uint8_t *dst)
{
    static thread_local uint32_t head[1u << ITXD_HBITS], fq[ITXD_NSYM], key[ITXD_NSYM], clfq[20], misc[16];
    static thread_local uint8_t ml[ITXD_MAX_IN], len[ITXD_NSYM], cllen[20];
    static thread_local uint16_t md[ITXD_MAX_IN], srt[ITXD_NSYM], code[ITXD_NSYM], clcode[20];
    static thread_local uint64_t red[2];
    if (n > ITXD_MAX_IN) return 0;
    load(src, n);
    itxd_ws w = {in, head, ml, md, fq, key, srt, len, code, clfq, cllen, clcode, red, misc};
    return itx_bgzf_member(w, n, dst, 0, 1);
}

// the CRC-32 of n bytes as nl lanes compute it: every lane's term, one after the other, XORed
extern "C" uint32_t itx_crc32_lanes_host(const uint8_t *src, uint32_t n, uint32_t nl)
{
    if (n > ITXD_MAX_IN || nl == 0) return 0;
    load(src, n);
    uint32_t crc = 0;
    for (uint32_t l = 0; l < nl; l++) crc ^= itx_crc32_term(in, n, l, nl);
    return crc;
}
