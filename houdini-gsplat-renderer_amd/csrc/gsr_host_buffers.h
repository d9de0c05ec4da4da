// gsr_host_buffers.h -- host side of gsr_api.hip's buffer handling: the thread's last error, HIP_TRY, the four handles that own what
// the host code allocates, buffers that grow (replace, regrow) and the staging buffer a frame slot keeps for a caller's host memory
// (StageBuf).  No kernels; included by gsr_api.hip alone.
//
//   DevMem<T>      device memory (hipMalloc): alloc / alloc_zeroed, converts to T*
//   PinnedMem<T>   pinned host memory (hipHostMalloc); where mapped, dev() is the address the kernels write it at
//   Event, Stream  hipEventCreateWithFlags / hipStreamCreateWithFlags; convert to the HIP handle
//
// The rule: a member that owns is a handle; a raw pointer never owns.  A handle releases in its destructor (on whatever device is
// current: gsr_destroy sets it once, in front of `delete c`), moves by std::move or swap, and is never copied or made from a raw pointer
// (DevMem::adopt takes one over, explicitly).  g_live counts the live objects of each kind (gsr_debug_live_handles).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>

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

enum { GSR_LIVE_DEV = 0, GSR_LIVE_PINNED = 1, GSR_LIVE_EVENT = 2, GSR_LIVE_STREAM = 3 };
static std::atomic<int64_t> g_live[4];
static inline void live_count(int kind, int64_t by) { g_live[kind].fetch_add(by, std::memory_order_relaxed); }

// What the four handles share: one raw value of kind K (GSR_LIVE_*), moved and swapped but never copied, released by K's call.
template <class Raw, int K>
class Owned {
protected:
    Raw h_ = nullptr;
    void take(Raw raw) { reset(); h_ = raw; if (raw) live_count(K, 1); }

public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    ~Owned() { reset(); }
    operator Raw() const { return h_; }
    Raw get() const { return h_; }
    void swap(Owned& o) noexcept { std::swap(h_, o.h_); }
    void reset()
    {
        if (!h_) return;
        if constexpr (K == GSR_LIVE_DEV) (void)hipFree(h_);
        else if constexpr (K == GSR_LIVE_PINNED) (void)hipHostFree(h_);
        else if constexpr (K == GSR_LIVE_EVENT) (void)hipEventDestroy(h_);
        else (void)hipStreamDestroy(h_);
        live_count(K, -1);
        h_ = nullptr;
    }
};

// alloc: count elements in place of what the handle held (0: one element); a failure leaves it empty
template <typename T>
struct DevMem : Owned<T*, GSR_LIVE_DEV> {
    void adopt(T* raw) { this->take(raw); }
    int alloc(size_t count)
    {
        this->reset();
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
        adopt(static_cast<T*>(q));
        return GSR_OK;
    }
    int alloc_zeroed(size_t count)
    {
        const int rc = alloc(count);
        if (rc) return rc;
        HIP_TRY(hipMemset(this->h_, 0, (count ? count : 1) * sizeof(T)));
        return GSR_OK;
    }
};

// alloc: count elements, zeroed, with hipHostMalloc's `flags`; where those map the memory, dev() is its device-side address
template <typename T>
class PinnedMem : public Owned<T*, GSR_LIVE_PINNED> {
    T* dev_ = nullptr;                 // (read only while the handle holds memory)

public:
    T* dev() const { return this->h_ ? dev_ : nullptr; }
    void swap(PinnedMem& o) noexcept { Owned<T*, GSR_LIVE_PINNED>::swap(o); std::swap(dev_, o.dev_); }
    int alloc(size_t count, unsigned flags)
    {
        this->reset();
        void *q = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&q, count * sizeof(T), flags));
        this->take(static_cast<T*>(q));
        std::memset(q, 0, count * sizeof(T));
        const hipError_t e = (flags & hipHostMallocMapped) ? hipHostGetDevicePointer(&d, q, 0) : hipSuccess;
        if (e != hipSuccess) { this->reset(); return set_err(GSR_E_HIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e)); }
        dev_ = static_cast<T*>(d);
        return GSR_OK;
    }
};

// create: the runtime's own code (the callers word their errors); a failure leaves the handle empty
struct Event : Owned<hipEvent_t, GSR_LIVE_EVENT> {
    hipError_t create(unsigned flags)
    {
        hipEvent_t e = nullptr;
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        take(rc == hipSuccess ? e : nullptr);
        return rc;
    }
};
struct Stream : Owned<hipStream_t, GSR_LIVE_STREAM> {
    hipError_t create(unsigned flags)
    {
        hipStream_t s = nullptr;
        const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
        take(rc == hipSuccess ? s : nullptr);
        return rc;
    }
};

// p is to hold `count` elements in place of what it held (cap = the new capacity; 0 and an empty handle after a failure)
template <typename T>
static int replace(DevMem<T>& p, size_t& cap, size_t count, size_t new_cap)
{
    cap = 0;
    const int rc = p.alloc(count);
    if (!rc) cap = new_cap;
    return rc;
}
// a slot buffer too small for this frame: drain what may still read the old one, then replace it
template <typename T>
static int regrow(hipStream_t s, DevMem<T>& p, size_t& cap, size_t count, size_t new_cap)
{
    HIP_TRY(hipStreamSynchronize(s));
    return replace(p, cap, count, new_cap);
}

// The device side of a caller's HOST buffer, kept by a frame slot from frame to frame: the image and the AOV plane a frame is
// composited into before it is copied back, the copies of a host depth buffer and of a host background image.  Bytes throughout.
//
// sig: the band shape the buffer was last cleared for (the image's: and the target format).  A sharded context's band is padded
// (gsr_band_rows) and the pixel rows behind the rank's last image row are never written.  In a host target they read as zeros: the
// buffer is cleared whenever the band it is to hold is not the one it was last cleared for, and a buffer that was just allocated
// has been cleared for none.
struct StageBuf {
    DevMem<char> p;
    size_t cap = 0;
    int sig[6] = {-1, -1, -1, -1, -1, -1};

    void release()
    {
        p.reset();
        cap = 0;
        std::memset(sig, 0xff, sizeof sig);
    }
    int ensure(hipStream_t s, size_t bytes)
    {
        if (bytes <= cap) return GSR_OK;
        std::memset(sig, 0xff, sizeof sig);
        return regrow(s, p, cap, bytes, bytes);
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
