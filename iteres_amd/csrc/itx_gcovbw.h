// itx_gcovbw.h — between itx_gcov.hip (the coverage object and its C ABI) and itx_gcovbw.hip (the bigWig content of one of its
// files): the build takes the change points as they lie on the device and keeps what it made until it is freed.
#pragma once
#include "itx_device.h"

struct GcBw;
// pts[n_pts]: (position, depth from here on, visited chromosome, 0); vsize[nv] / vchrom[nv]: size of visited chromosome k and its
// index for the caller. ITX_OK with *out set (a file without an item: n_items 0), or ITX_E_NOMEM / ITX_E_LIMIT / a HIP failure with
// nothing kept.
int gcbw_build(int device, hipStream_t st, const uint4 *pts, unsigned long long n_pts, const uint32_t *vsize, const uint32_t *vchrom, uint32_t nv, GcBw **out);
void gcbw_result(const GcBw *b, itx_gcov_bw_result *out);
double gcbw_device_ms(const GcBw *b);
void gcbw_free(GcBw *b);
