// A stand-in for <hip/hip_runtime.h> that lets csrc/gsr_host_buffers.h compile and run with the host compiler alone
// (tests/host_buffers_main.cpp): the calls the header uses, backed by malloc / free.  It counts the live objects per kind, and can be
// told to fail the k-th acquisition from now on with hipErrorOutOfMemory.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct stub_stream* hipStream_t;
typedef struct stub_event* hipEvent_t;
struct stub_stream { int flags; };
struct stub_event { int flags; };
enum { hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000, hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };

enum { STUB_DEV = 0, STUB_PINNED = 1, STUB_EVENT = 2, STUB_STREAM = 3 };
static long stub_live[4] = {0, 0, 0, 0};
static long stub_fail_in = 0;          // k > 0: the k-th acquisition from now fails; 0: none does
static long stub_syncs = 0;            // hipStreamSynchronize calls
static long stub_calls = 0;            // every stubbed call that acquires, releases, synchronises or clears the last error
static long stub_peak[4] = {0, 0, 0, 0};   // the largest live count per kind since the test last set it
static long stub_errors_cleared = 0;   // hipGetLastError calls
struct uint4 { unsigned x, y, z, w; };

static inline void stub_fail_kth(long k) { stub_fail_in = k; }
static inline bool stub_acquire(int kind)
{
    stub_calls += 1;
    if (stub_fail_in > 0 && --stub_fail_in == 0) return false;
    stub_live[kind] += 1;
    if (stub_live[kind] > stub_peak[kind]) stub_peak[kind] = stub_live[kind];
    return true;
}

static inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : (e == hipErrorOutOfMemory ? "out of memory" : "invalid value"); }
static inline hipError_t hipMalloc(void** p, size_t bytes)
{
    *p = nullptr;
    if (!stub_acquire(STUB_DEV)) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    return hipSuccess;
}
static inline hipError_t hipFree(void* p)
{
    stub_calls += 1;
    if (p) stub_live[STUB_DEV] -= 1;
    std::free(p);
    return hipSuccess;
}
static inline hipError_t hipMemset(void* p, int v, size_t bytes) { std::memset(p, v, bytes); return hipSuccess; }
static inline hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) { std::memset(p, v, bytes); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t bytes, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, bytes); return hipSuccess; }
static inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned)
{
    *p = nullptr;
    if (!stub_acquire(STUB_PINNED)) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    return hipSuccess;
}
static inline hipError_t hipHostFree(void* p)
{
    if (p) stub_live[STUB_PINNED] -= 1;
    std::free(p);
    return hipSuccess;
}
static inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    *e = nullptr;
    if (!stub_acquire(STUB_EVENT)) return hipErrorOutOfMemory;
    *e = new stub_event{(int)flags};
    return hipSuccess;
}
static inline hipError_t hipEventDestroy(hipEvent_t e)
{
    if (e) stub_live[STUB_EVENT] -= 1;
    delete e;
    return hipSuccess;
}
static inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags)
{
    *s = nullptr;
    if (!stub_acquire(STUB_STREAM)) return hipErrorOutOfMemory;
    *s = new stub_stream{(int)flags};
    return hipSuccess;
}
static inline hipError_t hipStreamDestroy(hipStream_t s)
{
    if (s) stub_live[STUB_STREAM] -= 1;
    delete s;
    return hipSuccess;
}
static inline hipError_t hipStreamSynchronize(hipStream_t) { stub_syncs += 1; stub_calls += 1; return hipSuccess; }
static inline hipError_t hipGetLastError() { stub_errors_cleared += 1; stub_calls += 1; return hipSuccess; }
