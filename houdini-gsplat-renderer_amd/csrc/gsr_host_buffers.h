// gsr_host_buffers.h -- host side of gsr_api.hip's buffer handling: the thread's last error, HIP_TRY, the handles that own what the host
// code allocates, and what is built of them: groups of buffers that share a capacity (DevGroup: TileSet, WirePair, MortonScratch) and the
// staging buffer a frame slot keeps for a caller's host memory (StageBuf).  No kernels; included by gsr_api.hip alone.
//
//   DevMem<T>      device memory (hipMalloc): alloc / alloc_zeroed, converts to T*
//   PinnedMem<T>   pinned host memory (hipHostMalloc); where mapped, dev() is the address the kernels write it at
//   Event, Stream  hipEventCreateWithFlags / hipStreamCreateWithFlags; convert to the HIP handle
//   DevVec<T>      a DevMem and its capacity in elements, kept in step by construction: ensure / ensure_drained grow it, converts to T*
//
// The rule: a member that owns is a handle; a raw pointer never owns; a capacity lives inside the handle it speaks of.  A handle
// releases in its destructor (on whatever device is current: gsr_destroy sets it once, in front of `delete c`), moves by std::move or
// swap, and is never copied or made from a raw pointer (DevMem::adopt takes one over, explicitly).  g_live counts the live objects of
// each kind (gsr_debug_live_handles).  How much beyond its need a buffer allocates is written once per rule: at its one site, or in
// the helper its users share (ensure_counts, ensure_stage, MortonScratch::hold).
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

// A device buffer that grows: a DevMem and the capacity it answers for, in elements -- zero exactly when the handle is empty.
//   ensure(count, alloc_count)   count <= cap(): nothing, not a HIP call.  Otherwise what it held is released, THEN alloc_count elements
//                                (count, unless the site allocates slack that is no capacity) are allocated and cap() is count; a
//                                failure leaves it empty, cap() 0, and returns DevMem::alloc's code
//   ensure_drained(s, ...)       the same for a buffer that work queued on `s` may still read: drained first, only when it has to go
template <typename T>
class DevVec {
    DevMem<T> p_;
    size_t cap_ = 0;

public:
    DevVec() = default;
    DevVec(DevVec&& o) noexcept : p_(std::move(o.p_)), cap_(o.cap_) { o.cap_ = 0; }
    DevVec& operator=(DevVec&& o) noexcept { if (this != &o) { p_ = std::move(o.p_); cap_ = o.cap_; o.cap_ = 0; } return *this; }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    void reset() { p_.reset(); cap_ = 0; }
    void swap(DevVec& o) noexcept { p_.swap(o.p_); std::swap(cap_, o.cap_); }
    int ensure(size_t count, size_t alloc_count)
    {
        if (count <= cap_) return GSR_OK;
        const int rc = p_.alloc(alloc_count);
        cap_ = rc ? 0 : count;
        return rc;
    }
    int ensure(size_t count) { return ensure(count, count); }
    int ensure_drained(hipStream_t s, size_t count, size_t alloc_count)
    {
        if (count <= cap_) return GSR_OK;
        HIP_TRY(hipStreamSynchronize(s));
        return ensure(count, alloc_count);
    }
    int ensure_drained(hipStream_t s, size_t count) { return ensure_drained(s, count, count); }
};

// Buffers that share ONE capacity.  A group lists its members once, in each(f, n): f(member, its elements at capacity n), in the order
// they are released and allocated.  ensure / ensure_drained as DevVec's; a member that cannot be allocated leaves ALL of them empty,
// the capacity 0, and its code is the group's.
template <class Group>
class DevGroup {
    size_t cap_ = 0;
    Group& self() { return static_cast<Group&>(*this); }

public:
    size_t cap() const { return cap_; }
    void release() { self().each([](auto& m, size_t) { m.reset(); }, 0); cap_ = 0; }
    int ensure(size_t n)
    {
        if (n <= cap_) return GSR_OK;
        release();
        int rc = GSR_OK;
        self().each([&rc](auto& m, size_t count) { if (!rc) rc = m.alloc(count); }, n);
        if (rc) release(); else cap_ = n;
        return rc;
    }
    int ensure_drained(hipStream_t s, size_t n)
    {
        if (n <= cap_) return GSR_OK;
        HIP_TRY(hipStreamSynchronize(s));
        return ensure(n);
    }
};

// a frame slot's per-tile arrays (per tile: entries scanned, records gathered, wave-record evaluations; phase 1's copy of a front-slab
// frame; the tiles lazy colour gave up) and its super-tile ranges (65537 each)
struct TileSet : DevGroup<TileSet> {
    DevMem<uint4> tile_work, tile_work_a;
    DevMem<int32_t> sstart, send, redo;
    template <class F> void each(F f, size_t n) { f(tile_work, n); f(tile_work_a, n); f(sstart, (size_t)65536 + 1); f(send, (size_t)65536 + 1); f(redo, n); }
};
// the wire overlay: (depth bits, splat index) per pixel, and the image staged for a host target (16 bytes per pixel: enough for every format)
struct WirePair : DevGroup<WirePair> {
    DevMem<unsigned long long> zbuf;
    DevMem<float> out;
    template <class F> void each(F f, size_t n) { f(zbuf, n); f(out, n * 4); }
};
// the scratch of a Morton sort: codes / upload indices, ping-pong.  hold(n): an eighth and 1024 entries beyond the need; the callers go
// on without it (upload order) or word their own refusal, so a failure also clears the runtime's sticky error
struct MortonScratch : DevGroup<MortonScratch> {
    DevMem<uint32_t> kA, kB, vA, vB;
    template <class F> void each(F f, size_t n) { f(kA, n); f(kB, n); f(vA, n); f(vB, n); }
    int hold(size_t n)
    {
        const int rc = n <= cap() ? GSR_OK : ensure(n + n / 8 + 1024);
        if (rc) (void)hipGetLastError();
        return rc;
    }
};

// The device side of a caller's HOST buffer, kept by a frame slot from frame to frame: the image and the AOV plane a frame is
// composited into before it is copied back, the copies of a host depth buffer and of a host background image.  Bytes throughout.
//
// sig: the band shape the buffer was last cleared for (the image's: and the target format).  A sharded context's band is padded
// (gsr_band_rows) and the pixel rows behind the rank's last image row are never written.  In a host target they read as zeros: the
// buffer is cleared whenever the band it is to hold is not the one it was last cleared for, and a buffer that was just allocated
// has been cleared for none.
struct StageBuf {
    DevVec<char> p;                    // (grown to the exact size asked for)
    int sig[6] = {-1, -1, -1, -1, -1, -1};

    void release() { p.reset(); std::memset(sig, 0xff, sizeof sig); }
    int ensure(hipStream_t s, size_t bytes)
    {
        if (bytes > p.cap()) std::memset(sig, 0xff, sizeof sig);
        return p.ensure_drained(s, bytes);
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
        if (const int rc = ensure(s, bytes)) return rc;
        HIP_TRY(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, s));
        return GSR_OK;
    }
};
