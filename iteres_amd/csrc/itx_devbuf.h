// itx_devbuf.h — host only: the plumbing the device objects' host halves share ("Host-side plumbing of the device objects").
//   itx_grow_alloc, itx_grow_commit   buffers grow and keep what they hold; several are taken together or not at all
//   itx_copy_out                      device memory to host memory, in chunks through a page-locked pair
//   ItxBuf, itx_buf_need              a device buffer that lives as long as its scope (a build's working memory, an object's
//                                     members): made or enlarged on demand WITHOUT keeping what it held, freed by its destructor
//   ItxPin, itx_pin_need              the same in page-locked host memory
//   ItxEvent, itx_event_make          an event that lives as long as its scope
#pragma once
#include "itx_common.h"

#include <string.h>

template <bool PINNED>
struct ItxMem {
    void *p = nullptr;
    size_t cap = 0;
    ItxMem() = default;
    ItxMem(const ItxMem &) = delete;
    ItxMem &operator=(const ItxMem &) = delete;
    ~ItxMem() { drop(); }                    // (the owner has waited for the work that uses it)
    void drop()
    {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr, cap = 0;
    }
    void swap(ItxMem &o)
    {
        void *const op = o.p;
        const size_t oc = o.cap;
        o.p = p, o.cap = cap, p = op, cap = oc;
    }
    template <class T>
    T *as() const { return (T *)p; }
};
typedef ItxMem<false> ItxBuf;
typedef ItxMem<true> ItxPin;

// ITX_OK, or ITX_E_NOMEM with "who: no device (page-locked) memory for N bytes" (HIP's error is cleared, the buffer is empty)
template <bool PINNED>
static inline int itx_mem_need(const char *who, ItxMem<PINNED> &b, size_t bytes)
{
    if (bytes <= b.cap && b.p) return ITX_OK;
    b.drop();
    const size_t take = bytes ? bytes : 16;
    if ((PINNED ? hipHostMalloc(&b.p, take, hipHostMallocDefault) : hipMalloc(&b.p, take)) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        itx_set_error("%s: no %s memory for %zu bytes", who, PINNED ? "page-locked" : "device", bytes);
        return ITX_E_NOMEM;
    }
    b.cap = bytes;
    return ITX_OK;
}
static inline int itx_buf_need(const char *who, ItxBuf &b, size_t bytes) { return itx_mem_need(who, b, bytes); }
static inline int itx_pin_need(const char *who, ItxPin &b, size_t bytes) { return itx_mem_need(who, b, bytes); }

struct ItxEvent {
    hipEvent_t e = nullptr;
    ItxEvent() = default;
    ItxEvent(const ItxEvent &) = delete;
    ItxEvent &operator=(const ItxEvent &) = delete;
    ~ItxEvent()
    {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
};

static inline int itx_event_make(ItxEvent &ev) { return ev.e ? ITX_OK : itx_hip_rc(hipEventCreate(&ev.e), "hipEventCreate", __FILE__, __LINE__); }

// One buffer of a growth: *ptr becomes a buffer of `want` bytes (0: it stays as it is) that holds the first `keep` bytes of the old one.
struct ItxGrow {
    void **ptr;
    size_t keep, want;
    int pinned;                      // page-locked host memory, not HBM (keep is 0)
    void *fresh;                     // the helper's: the new buffer until it is swapped in, then the old one
};

static inline void itx_grow_free(ItxGrow *g, int n)
{
    for (int i = 0; i < n; i++) {
        if (g[i].fresh) (void)(g[i].pinned ? hipHostFree(g[i].fresh) : hipFree(g[i].fresh));
        g[i].fresh = nullptr;
    }
}

// Phase one: every new buffer is allocated, nothing of the object changes. Returns -1, or the index of the buffer that did not fit:
// then what was allocated is free again and HIP's error is cleared; the caller sets its own text and returns ITX_E_NOMEM.
static inline int itx_grow_alloc(ItxGrow *g, int n)
{
    for (int i = 0; i < n; i++) g[i].fresh = nullptr;
    for (int i = 0; i < n; i++) {
        if (!g[i].want) continue;
        if ((g[i].pinned ? hipHostMalloc(&g[i].fresh, g[i].want, hipHostMallocDefault) : hipMalloc(&g[i].fresh, g[i].want)) == hipSuccess) continue;
        (void)hipGetLastError();
        g[i].fresh = nullptr;
        itx_grow_free(g, n);
        return i;
    }
    return -1;
}

// Phase two: the kept bytes move device to device on st, st is waited for once if anything moved (before the old buffers go), the
// new buffers are swapped in and the old ones freed. If a copy fails the new buffers are freed: the object is as it was.
static inline int itx_grow_commit(hipStream_t st, ItxGrow *g, int n)
{
    int rc = ITX_OK;
    bool moved = false;
    for (int i = 0; i < n; i++)
        if (g[i].fresh && g[i].keep) {
            ITX_TRY(hipMemcpyAsync(g[i].fresh, *g[i].ptr, g[i].keep, hipMemcpyDeviceToDevice, st));
            moved = true;
        }
    if (moved) ITX_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++)
        if (g[i].fresh) {
            void *old = *g[i].ptr;
            *g[i].ptr = g[i].fresh;
            g[i].fresh = old;
        }
out:
    itx_grow_free(g, n);
    return rc;
}

#define ITX_COPY_CHUNK ((size_t)8 << 20)
// bytes of d_src to dst (pageable host memory) through the page-locked pair `pin`, allocated at the first call and the caller's to
// free: chunk k + 1 crosses the link while chunk k is copied out
static inline int itx_copy_out(hipStream_t st, uint8_t *pin[2], void *dst, const void *d_src, size_t bytes)
{
    int rc = ITX_OK;
    size_t done = 0, prev = 0;
    int k = 0;
    for (int i = 0; i < 2; i++)
        if (!pin[i]) ITX_TRY(hipHostMalloc((void **)&pin[i], ITX_COPY_CHUNK, hipHostMallocDefault));
    while (done < bytes || prev) {
        const size_t m = bytes - done < ITX_COPY_CHUNK ? bytes - done : ITX_COPY_CHUNK;
        if (m) ITX_TRY(hipMemcpyAsync(pin[k], (const uint8_t *)d_src + done, m, hipMemcpyDeviceToHost, st));
        if (prev) memcpy((uint8_t *)dst + done - prev, pin[k ^ 1], prev);
        ITX_TRY(hipStreamSynchronize(st));
        done += m;
        prev = m;
        k ^= 1;
    }
out:
    return rc;
}
