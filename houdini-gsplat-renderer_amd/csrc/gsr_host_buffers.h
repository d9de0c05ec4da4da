// gsr_host_buffers.h -- host side of gsr_api.hip's buffer handling: the thread's last error, HIP_TRY, device allocations that grow,
// and the staging buffer a frame slot keeps for a caller's host memory.  No kernels; included by gsr_api.hip alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/gsplat_hip.h"

static thread_local char g_err[512] = "";

static int set_err(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err(e_ == hipErrorOutOfMemory ? GSR_E_OOM : GSR_E_HIP, "%s failed: %s (%s:%d)", #expr, \
                           hipGetErrorString(e_), __FILE__, __LINE__);                             \
    } while (0)

template <typename T>
static int dev_alloc(T** p, size_t count)
{
    *p = nullptr;
    if (count == 0) count = 1;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return GSR_OK;
}
template <typename T>
static void dev_free(T*& p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

// a slot buffer too small for this frame: drain what may still read the old one, then replace it (count elements; cap = the new capacity)
template <typename T>
static int regrow(hipStream_t s, T*& p, size_t& cap, size_t count, size_t new_cap)
{
    HIP_TRY(hipStreamSynchronize(s));
    dev_free(p);
    cap = 0;
    const int rc = dev_alloc(&p, count);
    if (rc) return rc;
    cap = new_cap;
    return GSR_OK;
}

// The device side of a caller's HOST buffer, kept by a frame slot from frame to frame: the image and the AOV plane a frame is
// composited into before it is copied back, the copies of a host depth buffer and of a host background image.  Bytes throughout.
//
// sig: the band shape the buffer was last cleared for (the image's: and the target format).  A sharded context's band is padded
// (gsr_band_rows) and the pixel rows behind the rank's last image row are never written.  In a host target they read as zeros: the
// buffer is cleared whenever the band it is to hold is not the one it was last cleared for, and a buffer that was just allocated
// has been cleared for none.
struct StageBuf {
    void* p = nullptr;
    size_t cap = 0;
    int sig[6] = {-1, -1, -1, -1, -1, -1};

    void release()
    {
        dev_free(p);
        cap = 0;
        std::memset(sig, 0xff, sizeof sig);
    }
    int ensure(hipStream_t s, size_t bytes)
    {
        if (bytes <= cap) return GSR_OK;
        std::memset(sig, 0xff, sizeof sig);
        return regrow(s, reinterpret_cast<char*&>(p), cap, bytes, bytes);
    }
    int clear_if_reshaped(hipStream_t s, const int (&now)[6], size_t bytes)
    {
        if (std::memcmp(now, sig, sizeof sig) == 0) return GSR_OK;
        HIP_TRY(hipMemsetAsync(p, 0, bytes, s));
        std::memcpy(sig, now, sizeof sig);
        return GSR_OK;
    }
    int upload(hipStream_t s, const void* host, size_t bytes)
    {
        const int rc = ensure(s, bytes);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, s));
        return GSR_OK;
    }
};
