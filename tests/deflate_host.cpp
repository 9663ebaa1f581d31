// Host build of the device DEFLATE encoder (iteres_amd/csrc/itx_deflate_core.h) with a one-lane "wave" and plain arrays
// for its workspace: test infrastructure — the CPU suite checks it against zlib before it runs on a GPU.
#include <stdint.h>
#include <string.h>
#define ITXD_FN static inline
#define ITXD_SYNC() ((void)0)
#define ITXD_AMAX(p, v) ((void)(*(p) = *(p) > (v) ? *(p) : (v)))
#define ITXD_CTZ(x) ((uint32_t)__builtin_ctz(x))
#include "../iteres_amd/csrc/itx_deflate_core.h"

// n (<= 32768) bytes at src -> a zlib stream at dst (room: ITXD_OUT_CAP(n)); returns its size
extern "C" uint32_t itxd_deflate_host(const uint8_t *src, uint32_t n, uint8_t *dst)
{
    static thread_local uint32_t in[ITXD_MAX_IN / 4 + 4], head[1u << ITXD_HBITS], fq[ITXD_NSYM], key[ITXD_NSYM], clfq[20], misc[16];
    static thread_local uint8_t ml[ITXD_MAX_IN], len[ITXD_NSYM], cllen[20];
    static thread_local uint16_t md[ITXD_MAX_IN], srt[ITXD_NSYM], code[ITXD_NSYM], clcode[20];
    static thread_local uint64_t red[2];
    if (n > ITXD_MAX_IN) return 0;
    memset(in, 0, sizeof in);
    memcpy(in, src, n);
    itxd_ws w = {in, head, ml, md, fq, key, srt, len, code, clfq, cllen, clcode, red, misc};
    return itxd_deflate(w, n, dst, 0, 1);
}
