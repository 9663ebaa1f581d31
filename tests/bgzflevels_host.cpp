// Host build of the member levels (iteres_amd/csrc/itx_bgzflevels.h over itx_deflate_fast.h): test infrastructure — the CPU suite
// holds it to zlib, the GPU suite holds the device's bytes to it. A "wave" of nl lanes is nl threads that meet at a barrier where
// the device build has one, so the bytes of 1, 3 and 64 lanes can be compared; the hooks are atomic so that the threads may run
// them at once (for one lane they are the plain operations).
// With -DBGZFLEVELS_MAIN it is a stand-alone program: stdin holds payloads as (uint32 n, n bytes) records; every payload goes
// through levels 0 and 1 (1 and 3 lanes) and 6 into exact-size heap blocks, and every member goes to stdout as (uint32 level, lanes,
// n, size; size bytes) for the test to compare. That build is the one run under the sanitizers.
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local pthread_barrier_t *g_bar = nullptr;
static inline void lanes_sync(void)
{
    if (g_bar) pthread_barrier_wait(g_bar);
}
static inline void amax32(uint32_t *p, uint32_t v)
{
    uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}

#define ITXD_FN static inline
#define ITXD_SYNC() lanes_sync()
#define ITXD_AMAX(p, v) amax32((p), (v))
#define ITXD_AADD(p, v) ((void)__atomic_fetch_add((p), (v), __ATOMIC_RELAXED))
#define ITXD_AOR(p, v) ((void)__atomic_fetch_or((p), (v), __ATOMIC_RELAXED))
#define ITXD_CTZ(x) ((uint32_t)__builtin_ctz(x))
#include "../iteres_amd/csrc/itx_bgzflevels.h"

#define MAX_LANES 64u

// one member's workspace; the staging area is the hash heads' memory, as on the device
struct Work {
    uint32_t in[ITXD_MAX_IN / 4 + 4];
    uint32_t head_stage[ITXF_STAGE_WORDS(ITXD_MAX_IN, ITX_BGZF_LEAD) > (1u << ITXD_HBITS) ? ITXF_STAGE_WORDS(ITXD_MAX_IN, ITX_BGZF_LEAD) : (1u << ITXD_HBITS)];
    uint32_t fq[ITXD_NSYM], key[ITXD_NSYM], clfq[20], misc[16], sbits[ITXF_SLICES(ITXD_MAX_IN) + 1];
    uint8_t ml[ITXD_MAX_IN], len[ITXD_NSYM], cllen[20];
    uint16_t md[ITXD_MAX_IN], srt[ITXD_NSYM], code[ITXD_NSYM], clcode[20];
    uint64_t red[2 * MAX_LANES];
};

struct Job {
    Work *wk;
    uint32_t n, nl, level, lane, size;
    uint8_t *dst;
    pthread_barrier_t *bar;
};

static void *lane_main(void *arg)
{
    Job *j = (Job *)arg;
    Work *k = j->wk;
    g_bar = j->bar;
    const itxf_ws w = {{k->in, k->head_stage, k->ml, k->md, k->fq, k->key, k->srt, k->len, k->code, k->clfq, k->cllen, k->clcode, k->red, k->misc}, k->head_stage, k->sbits};
    j->size = itx_bgzf_member_level(w, j->n, j->dst, j->lane, j->nl, j->level);
    g_bar = nullptr;
    return nullptr;
}

extern "C" uint32_t itx_bgzf_levels_payload_host(void) { return ITX_BAMOUT_PAYLOAD; }
extern "C" uint32_t itx_bgzf_levels_cap_host(uint32_t n) { return ITX_BGZF_MEMBER_CAP(n); }
extern "C" uint32_t itx_bgzf_levels_slice_host(void) { return ITXF_SLICE; }

// n (<= 32768) payload bytes at src -> the member of `level` at dst (4-byte aligned, room: ITX_BGZF_MEMBER_CAP(n)), made by nl
// (1 .. 64) lanes; returns its size, 0 for an argument out of range
extern "C" uint32_t itx_bgzf_member_level_host(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t level, uint32_t nl)
{
    if (n > ITXD_MAX_IN || nl == 0 || nl > MAX_LANES || !ITX_BGZF_LEVEL_OK(level) || ((uintptr_t)dst & 3u)) return 0;
    Work *k = (Work *)calloc(1, sizeof(Work));
    if (!k) return 0;
    if (n) memcpy(k->in, src, n);
    Job job[MAX_LANES];
    pthread_barrier_t bar;
    for (uint32_t l = 0; l < nl; l++) job[l] = Job{k, n, nl, level, l, 0, dst, nl > 1 ? &bar : nullptr};
    uint32_t size = 0;
    if (nl == 1) {
        lane_main(&job[0]);
        size = job[0].size;
    } else {
        pthread_t th[MAX_LANES];
        uint32_t started = 0;
        pthread_barrier_init(&bar, nullptr, nl);
        for (; started < nl; started++)
            if (pthread_create(&th[started], nullptr, lane_main, &job[started]) != 0) break;
        if (started < nl) abort();                                 // (the started lanes would wait at the barrier for ever)
        for (uint32_t l = 0; l < nl; l++) pthread_join(th[l], nullptr);
        pthread_barrier_destroy(&bar);
        size = job[0].size;
        for (uint32_t l = 1; l < nl; l++)
            if (job[l].size != size) size = 0;                     // every lane is told the same size
    }
    free(k);
    return size;
}

// level 6 without the level call: itx_bgzf_member itself, one lane
extern "C" uint32_t itx_bgzf_member_plain_host(const uint8_t *src, uint32_t n, uint8_t *dst)
{
    if (n > ITXD_MAX_IN) return 0;
    Work *k = (Work *)calloc(1, sizeof(Work));
    if (!k) return 0;
    if (n) memcpy(k->in, src, n);
    const itxd_ws w = {k->in, k->head_stage, k->ml, k->md, k->fq, k->key, k->srt, k->len, k->code, k->clfq, k->cllen, k->clcode, k->red, k->misc};
    const uint32_t size = itx_bgzf_member(w, n, dst, 0, 1);
    free(k);
    return size;
}

#ifdef BGZFLEVELS_MAIN
int main(void)
{
    static const uint32_t runs[5][2] = {{0, 1}, {0, 3}, {1, 1}, {1, 3}, {6, 1}};
    uint32_t n, count = 0;
    while (fread(&n, 4, 1, stdin) == 1) {
        if (n > ITXD_MAX_IN) return 2;
        uint8_t *src = (uint8_t *)malloc(n ? n : 1);               // exact size: a read past the payload is an error
        if (!src || (n && fread(src, 1, n, stdin) != n)) return 2;
        for (const auto &r : runs) {
            const uint32_t cap = ITX_BGZF_MEMBER_CAP(n);
            uint8_t *dst = (uint8_t *)malloc(cap);                 // exact size: a write past the room is an error
            if (!dst) return 2;
            const uint32_t size = itx_bgzf_member_level_host(src, n, dst, r[0], r[1]);
            if (size == 0 || size > cap) return 3;
            const uint32_t rec[4] = {r[0], r[1], n, size};
            if (fwrite(rec, 4, 4, stdout) != 4 || fwrite(dst, 1, size, stdout) != size) return 4;
            free(dst);
        }
        free(src);
        count++;
    }
    fprintf(stderr, "%u payloads\n", count);
    return 0;
}
#endif
