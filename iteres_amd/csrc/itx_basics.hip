// itx_basics.hip — the library's basics: the thread's last error message, the ABI version, the device count.
#include "itx_common.h"

#include <cstdarg>
#include <cstdio>

static thread_local char g_err[512];
void itx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" const char *itx_last_error(void) { return g_err; }
extern "C" int itx_abi_version(void) { return 1005; }
extern "C" int itx_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        itx_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return ITX_E_NO_DEVICE;
    }
    return n;
}
