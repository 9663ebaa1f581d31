// itx_hostmem.hip — two host-side objects that own memory and launch nothing: page-locked buffers for the reader's chunks
// (itx_pinned_*) and the backlog of parsed records in HBM (itx_backlog_*).
#include "itx_common.h"

#include <stdio.h>
#include <stdlib.h>

// Page-locked host memory for the reader's chunk buffers. hipHostMalloc of 384 MB takes 62 ms — nearly all of it the kernel
// handing out and zeroing 98 k small pages, under a lock that other HIP calls of the process wait for; an anonymous mapping the
// kernel is asked to back with 2 MB pages (the box has transparent huge pages in "madvise" mode), touched once by a few threads
// and then registered, takes 25 ms single-threaded (touch 24 + hipHostRegister 1; profiles/r03_pin_probe.txt) and copies to
// the device at the same 57 GB/s. Falls back to hipHostMalloc where any step fails.
#include <sys/mman.h>
#include <mutex>
#include <thread>
#include <vector>
struct PinnedMap {
    void *user, *base;
    size_t len;
};
static std::mutex g_pin_mu;
static std::vector<PinnedMap> g_pinned;

extern "C" void *itx_pinned_alloc(size_t bytes)
{
    if (bytes == 0) bytes = 1;
    const size_t huge = (size_t)2 << 20;
    if (bytes >= 4 * huge && !getenv("ITX_PIN_PLAIN")) {
        const size_t len = ((bytes + huge - 1) & ~(huge - 1)) + huge;
        struct timespec t0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        void *base = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (base != MAP_FAILED) {
            uint8_t *user = (uint8_t *)(((uintptr_t)base + huge - 1) & ~(uintptr_t)(huge - 1));
            const size_t ulen = (bytes + huge - 1) & ~(huge - 1);
            (void)madvise(user, ulen, MADV_HUGEPAGE);
            // first touch (one byte per 2 MB would do for huge pages; every 4 KB page when the kernel declines them)
            const unsigned nt = 4;
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; t++)
                th.emplace_back([=]() {
                    const size_t lo = ulen / nt * t, hi = t + 1 == nt ? ulen : ulen / nt * (t + 1);
                    for (size_t a = lo; a < hi; a += 4096) ((volatile uint8_t *)user)[a] = 0;
                });
            for (auto &x : th) x.join();
            struct timespec ta, tb;
            clock_gettime(CLOCK_MONOTONIC, &ta);
            const hipError_t re = hipHostRegister(user, ulen, hipHostRegisterDefault);
            clock_gettime(CLOCK_MONOTONIC, &tb);
            if (getenv("ITX_TIMING_ALLOC"))
                fprintf(stderr, "[itx alloc] page-locked %.0f MB: mapped + touched %.1f ms, hipHostRegister %.1f ms\n", (double)ulen / 1e6,
                        1e3 * ((double)(ta.tv_sec - t0.tv_sec) + 1e-9 * (double)(ta.tv_nsec - t0.tv_nsec)), 1e3 * ((double)(tb.tv_sec - ta.tv_sec) + 1e-9 * (double)(tb.tv_nsec - ta.tv_nsec)));
            if (re == hipSuccess) {
                std::lock_guard<std::mutex> g(g_pin_mu);
                g_pinned.push_back(PinnedMap{user, base, len});
                return user;
            }
            (void)hipGetLastError();
            munmap(base, len);
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

extern "C" void itx_pinned_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        for (size_t i = 0; i < g_pinned.size(); i++)
            if (g_pinned[i].user == p) {
                const PinnedMap m = g_pinned[i];
                g_pinned.erase(g_pinned.begin() + (long)i);
                (void)hipHostUnregister(m.user);
                munmap(m.base, m.len);
                return;
            }
    }
    (void)hipHostFree(p);
}

// ---------------------------------------------------------------------------------------------------------------------
// A backlog of parsed records in HBM (SoA, 14 B per record, 22 with mates): the caller parses windows while its table is
// still being built, keeps only what the engine will read — a ninth of the inflated bytes — and lets the windows go
// (host/stream.c). Offsets are multiples of 16 records (itx_engine_submit_device* wants batches to start there).
struct itx_backlog {
    int device;
    size_t cap, used;
    int32_t *tid, *pos, *end, *mpos, *isize;
    uint8_t *mapq, *f5;
    hipStream_t st;
};

extern "C" int itx_backlog_create(int device, size_t max_records, itx_backlog **out)
{
    if (!out || max_records == 0 || max_records >= ((size_t)1 << 31)) return ITX_E_ARG;
    *out = nullptr;
    ITX_HIP(hipSetDevice(device));
    itx_backlog *b = (itx_backlog *)calloc(1, sizeof *b);
    if (!b) return ITX_E_NOMEM;
    b->device = device;
    b->cap = (max_records + 15) & ~(size_t)15;
    const size_t n = b->cap + 64;
    if (hipMalloc((void **)&b->tid, n * 4) != hipSuccess || hipMalloc((void **)&b->pos, n * 4) != hipSuccess || hipMalloc((void **)&b->end, n * 4) != hipSuccess ||
        hipMalloc((void **)&b->mapq, n) != hipSuccess || hipMalloc((void **)&b->f5, n) != hipSuccess) {
        itx_set_error("itx_backlog_create: no device memory for %zu records", max_records);
        (void)hipGetLastError();
        (void)hipFree(b->tid); (void)hipFree(b->pos); (void)hipFree(b->end); (void)hipFree(b->mapq); (void)hipFree(b->f5);
        free(b);
        return ITX_E_NOMEM;
    }
    *out = b;
    return ITX_OK;
}

extern "C" void itx_backlog_destroy(itx_backlog *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->st) {
        (void)hipStreamSynchronize(b->st);
        (void)hipStreamDestroy(b->st);
    }
    (void)hipFree(b->tid); (void)hipFree(b->pos); (void)hipFree(b->end); (void)hipFree(b->mapq); (void)hipFree(b->f5);
    (void)hipFree(b->mpos); (void)hipFree(b->isize);
    free(b);
}

/* room left, in records */
extern "C" size_t itx_backlog_room(const itx_backlog *b) { return b ? b->cap - b->used : 0; }

/* appends n records (DEVICE arrays; mpos / isize NULL: no mates) — copied, the source may be reused when the call returns;
 * *at = where they lie (a multiple of 16). ITX_E_LIMIT: no room (nothing copied). */
extern "C" int itx_backlog_append(itx_backlog *b, const itx_batch *src, size_t n, size_t *at)
{
    if (!b || !src || !at || !src->tid || !src->pos || !src->tmpend || !src->mapq || !src->flag5) return ITX_E_ARG;
    if (n > b->cap - b->used) return ITX_E_LIMIT;
    ITX_HIP(hipSetDevice(b->device));
    const size_t o = b->used;
    if (src->mpos && src->isize && !b->mpos) {
        const size_t m = b->cap + 64;
        ITX_HIP(hipMalloc((void **)&b->mpos, m * 4));
        ITX_HIP(hipMalloc((void **)&b->isize, m * 4));
    }
    if (!b->st) ITX_HIP(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));       // (a run that appends nothing has no such stream)
    ITX_HIP(hipMemcpyAsync(b->tid + o, src->tid, n * 4, hipMemcpyDeviceToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(b->pos + o, src->pos, n * 4, hipMemcpyDeviceToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(b->end + o, src->tmpend, n * 4, hipMemcpyDeviceToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(b->mapq + o, src->mapq, n, hipMemcpyDeviceToDevice, b->st));
    ITX_HIP(hipMemcpyAsync(b->f5 + o, src->flag5, n, hipMemcpyDeviceToDevice, b->st));
    if (src->mpos && src->isize) {
        ITX_HIP(hipMemcpyAsync(b->mpos + o, src->mpos, n * 4, hipMemcpyDeviceToDevice, b->st));
        ITX_HIP(hipMemcpyAsync(b->isize + o, src->isize, n * 4, hipMemcpyDeviceToDevice, b->st));
    }
    ITX_HIP(hipStreamSynchronize(b->st));
    *at = o;
    b->used = (o + n + 15) & ~(size_t)15;
    return ITX_OK;
}

/* the records at `at` as a batch for itx_engine_submit_device* (with_mates: the batch was appended with mates) */
extern "C" int itx_backlog_batch(const itx_backlog *b, size_t at, int with_mates, itx_batch *out)
{
    if (!b || !out || at > b->used || (at & 15u) || (with_mates && !b->mpos)) return ITX_E_ARG;
    out->tid = b->tid + at;
    out->pos = b->pos + at;
    out->tmpend = b->end + at;
    out->mapq = b->mapq + at;
    out->flag5 = b->f5 + at;
    out->mpos = with_mates ? b->mpos + at : nullptr;
    out->isize = with_mates ? b->isize + at : nullptr;
    return ITX_OK;
}
