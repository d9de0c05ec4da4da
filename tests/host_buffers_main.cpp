// The owning handles of csrc/gsr_host_buffers.h on the host alone: compiled against tests/hip_stub (malloc / free behind the HIP
// calls, with counters) and run under the address and undefined-behaviour sanitizers by tests/test_host_buffers.py.  Exit status 0:
// every check held, every object the stub handed out came back, and the header's own counts (g_live) agree with the stub's.
#include "../houdini-gsplat-renderer_amd/csrc/gsr_host_buffers.h"

#include <cstdio>
#include <utility>

static int g_failed = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed += 1; } \
    } while (0)

static bool live_is(long dev, long pinned, long events, long streams)
{
    const long want[4] = {dev, pinned, events, streams};
    for (int k = 0; k < 4; ++k)
        if (stub_live[k] != want[k] || g_live[k].load() != want[k]) {
            std::printf("  kind %d: stub %ld, g_live %ld, want %ld\n", k, stub_live[k], (long)g_live[k].load(), want[k]);
            return false;
        }
    return true;
}

static void scope_exit_releases()
{
    {
        DevMem<float> d;
        PinnedMem<unsigned> p;
        Event e;
        Stream s;
        CHECK(!d && !p && !e && !s);
        CHECK(d.alloc(10) == GSR_OK && p.alloc(4, 0) == GSR_OK && e.create(hipEventDisableTiming) == hipSuccess && s.create(hipStreamNonBlocking) == hipSuccess);
        CHECK(d && p && e && s);
        CHECK(live_is(1, 1, 1, 1));
    }
    CHECK(live_is(0, 0, 0, 0));
}

template <class H, class Make>
static void moves_and_swaps(int kind, Make&& make)
{
    long want[4] = {0, 0, 0, 0};
    auto is = [&](long n) { want[kind] = n; return live_is(want[0], want[1], want[2], want[3]); };
    H a, b;
    make(a); make(b);
    CHECK(is(2));
    const auto pa = static_cast<decltype(+a)>(a), pb = static_cast<decltype(+b)>(b);
    CHECK(pa && pb && pa != pb);
    a.swap(b);                         // releases nothing
    CHECK(is(2) && a == pb && b == pa);
    H c(std::move(a));                 // move construction: the source is empty, nothing is released
    CHECK(is(2) && !a && c == pb);
    b = std::move(c);                  // move assignment: what b held is released exactly once
    CHECK(is(1) && !c && b == pb);
    b = std::move(a);                  // ... from an empty source: b is empty
    CHECK(is(0) && !b);
    make(a);
    a.reset(); a.reset();              // twice is harmless
    CHECK(is(0) && !a);
    H& self = a;
    make(a);
    a = std::move(self);               // self-assignment keeps the object
    CHECK(is(1) && a);
    make(a);                           // acquiring again releases what was held
    CHECK(is(1));
}

static void allocation_edges()
{
    DevMem<double> d;
    CHECK(d.alloc(0) == GSR_OK && d != nullptr);                     // a count of 0 allocates one element
    d[0] = 1.5;
    CHECK(d.alloc_zeroed(3) == GSR_OK && d[0] == 0.0 && d[2] == 0.0 && live_is(1, 0, 0, 0));
    CHECK(d.alloc_zeroed(0) == GSR_OK && d[0] == 0.0);
    const double* alias = d + 0;                                     // converts for pointer arithmetic, and in a conditional
    CHECK((true ? d : (const double*)nullptr) == alias);
    stub_fail_kth(1);
    CHECK(d.alloc(8) == GSR_E_OOM && !d && live_is(0, 0, 0, 0));     // a failure leaves the handle empty (what it held is gone)
    CHECK(std::strstr(g_err, "hipMalloc") && std::strstr(g_err, "out of memory"));
    double* raw = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&raw), 8) == hipSuccess);
    d.adopt(raw);                                                    // a raw pointer is taken over explicitly, and counted
    CHECK(d == raw && live_is(1, 0, 0, 0));
    d.reset();
    stub_fail_kth(1);
    Event e;
    CHECK(e.create(hipEventDefault) == hipErrorOutOfMemory && !e);
    stub_fail_kth(1);
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipErrorOutOfMemory && !s);
    CHECK(live_is(0, 0, 0, 0));
}

static void pinned_aliases()
{
    PinnedMem<unsigned long long> plain, mapped;
    CHECK(plain.alloc(8, 0) == GSR_OK && plain && plain.dev() == nullptr);           // no alias unless mapped
    CHECK(mapped.alloc(4, hipHostMallocMapped | hipHostMallocCoherent) == GSR_OK && mapped.dev() != nullptr);
    for (int k = 0; k < 4; ++k) CHECK(mapped[k] == 0ull);                            // zeroed
    mapped[3] = 7ull;
    CHECK(mapped.dev()[3] == 7ull);
    PinnedMem<unsigned long long> taken(std::move(mapped));
    CHECK(!mapped && mapped.dev() == nullptr && taken.dev() != nullptr && live_is(0, 2, 0, 0));
    stub_fail_kth(1);
    CHECK(taken.alloc(4, hipHostMallocMapped) == GSR_E_OOM && !taken && taken.dev() == nullptr && live_is(0, 1, 0, 0));
}

static void growing_buffers()
{
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    DevMem<int> p;
    size_t cap = 0;
    const long syncs = stub_syncs;
    CHECK(regrow(s, p, cap, 100, 96) == GSR_OK && p && cap == 96 && stub_syncs == syncs + 1);   // (drains the stream first)
    stub_fail_kth(1);
    CHECK(regrow(s, p, cap, 200, 200) == GSR_E_OOM && !p && cap == 0);             // a failed growth: no pointer, no capacity
    CHECK(live_is(0, 0, 0, 1));

    StageBuf b;
    const int shape[6] = {1, 2, 3, 4, 5, 6};
    CHECK(b.ensure(s, 64) == GSR_OK && b.p && b.cap == 64 && b.sig[0] == -1);
    CHECK(b.clear_if_reshaped(s, shape, 64) == GSR_OK && b.sig[5] == 6 && b.p[63] == 0);
    const char* kept = b.p;
    CHECK(b.ensure(s, 32) == GSR_OK && b.p == kept && b.cap == 64 && b.sig[5] == 6);   // large enough: the same buffer, still cleared for its shape
    const char host[4] = {1, 2, 3, 4};
    CHECK(b.upload(s, host, 4) == GSR_OK && b.p == kept && b.p[2] == 3);
    stub_fail_kth(1);
    CHECK(b.ensure(s, 128) == GSR_E_OOM && !b.p && b.cap == 0 && b.sig[0] == -1 && b.sig[5] == -1);   // ... and cleared for no shape
    CHECK(b.ensure(s, 128) == GSR_OK && b.cap == 128);
    b.release();
    CHECK(!b.p && b.cap == 0 && b.sig[0] == -1 && live_is(0, 0, 0, 1));
}

int main()
{
    scope_exit_releases();
    moves_and_swaps<DevMem<float>>(GSR_LIVE_DEV, [](DevMem<float>& h) { CHECK(h.alloc(16) == GSR_OK); });
    moves_and_swaps<PinnedMem<int>>(GSR_LIVE_PINNED, [](PinnedMem<int>& h) { CHECK(h.alloc(16, hipHostMallocMapped) == GSR_OK); });
    moves_and_swaps<Event>(GSR_LIVE_EVENT, [](Event& h) { CHECK(h.create(hipEventDisableTiming) == hipSuccess); });
    moves_and_swaps<Stream>(GSR_LIVE_STREAM, [](Stream& h) { CHECK(h.create(hipStreamNonBlocking) == hipSuccess); });
    CHECK(live_is(0, 0, 0, 0));
    allocation_edges();
    pinned_aliases();
    growing_buffers();
    CHECK(live_is(0, 0, 0, 0));        // at exit every counter is 0
    std::printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
