// The owning handles of csrc/gsr_host_buffers.h on the host alone: compiled against tests/hip_stub (malloc / free behind the HIP
// calls, with counters) and run under the address and undefined-behaviour sanitizers by tests/test_host_buffers.py.  Exit status 0:
// every check held -- the growing buffers (DevVec), the staging buffer and the groups that share a capacity included --, every object the
// stub handed out came back, and the header's own counts (g_live) agree with the stub's.
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
    DevVec<int> p;
    const long syncs = stub_syncs;
    CHECK(!p && p.cap() == 0);
    CHECK(p.ensure_drained(s, 96, 100) == GSR_OK && p && p.cap() == 96 && stub_syncs == syncs + 1);   // (drains the stream first; the slack is not capacity)
    p[99] = 7;                                                                     // (100 elements are there: the sanitizer checks)
    stub_fail_kth(1);
    CHECK(p.ensure_drained(s, 200) == GSR_E_OOM && !p && p.cap() == 0);            // a failed growth: no pointer, no capacity
    CHECK(std::strstr(g_err, "hipMalloc") && stub_syncs == syncs + 2);
    CHECK(live_is(0, 0, 0, 1));

    // below the capacity: the same pointer and not a HIP call
    CHECK(p.ensure(64) == GSR_OK && p.cap() == 64 && live_is(1, 0, 0, 1));
    const int* kept = p;
    const long calls = stub_calls;
    CHECK(p.ensure(64) == GSR_OK && p.ensure(1) == GSR_OK && p.ensure(0, 1000) == GSR_OK && p.ensure_drained(s, 64, 65) == GSR_OK);
    CHECK(p == kept && p.get() == kept && p.cap() == 64 && stub_calls == calls);
    // above it: what it held is released BEFORE the new buffer is allocated (one buffer never holds two), without a drain unless asked for
    stub_peak[STUB_DEV] = stub_live[STUB_DEV];
    CHECK(p.ensure(65) == GSR_OK && p.cap() == 65 && stub_peak[STUB_DEV] == 1 && stub_syncs == syncs + 2);
    CHECK(p.ensure_drained(s, 66) == GSR_OK && p.cap() == 66 && stub_peak[STUB_DEV] == 1 && stub_syncs == syncs + 3);
    stub_fail_kth(1);
    CHECK(p.ensure(67, 70) == GSR_E_OOM && !p && p.cap() == 0 && live_is(0, 0, 0, 1));
    CHECK(p.ensure(0) == GSR_OK && !p && p.cap() == 0);                            // (nothing asked for, nothing held)

    // move and swap carry the capacity with the pointer
    DevVec<int> a, b;
    CHECK(a.ensure(10, 12) == GSR_OK && b.ensure(20) == GSR_OK);
    const int *pa = a, *pb = b;
    a.swap(b);
    CHECK(a == pb && a.cap() == 20 && b == pa && b.cap() == 10 && live_is(2, 0, 0, 1));
    DevVec<int> c(std::move(a));
    CHECK(!a && a.cap() == 0 && c == pb && c.cap() == 20 && live_is(2, 0, 0, 1));
    b = std::move(c);                                                              // what b held is released exactly once
    CHECK(!c && c.cap() == 0 && b == pb && b.cap() == 20 && live_is(1, 0, 0, 1));
    DevVec<int>& self = b;
    b = std::move(self);                                                           // self-assignment keeps buffer and capacity
    CHECK(b == pb && b.cap() == 20);
    b = std::move(a);                                                              // from an empty source: empty
    CHECK(!b && b.cap() == 0 && live_is(0, 0, 0, 1));
    CHECK(b.ensure(5) == GSR_OK);
    b.reset(); b.reset();
    CHECK(!b && b.cap() == 0 && live_is(0, 0, 0, 1));

    StageBuf sb;
    const int shape[6] = {1, 2, 3, 4, 5, 6};
    CHECK(sb.ensure(s, 64) == GSR_OK && sb.p && sb.p.cap() == 64 && sb.sig[0] == -1);
    CHECK(sb.clear_if_reshaped(s, shape, 64) == GSR_OK && sb.sig[5] == 6 && sb.p[63] == 0);
    const char* held = sb.p;
    CHECK(sb.ensure(s, 32) == GSR_OK && sb.p == held && sb.p.cap() == 64 && sb.sig[5] == 6);   // large enough: the same buffer, still cleared for its shape
    const char host[4] = {1, 2, 3, 4};
    CHECK(sb.upload(s, host, 4) == GSR_OK && sb.p == held && sb.p[2] == 3);
    stub_fail_kth(1);
    CHECK(sb.ensure(s, 128) == GSR_E_OOM && !sb.p && sb.p.cap() == 0 && sb.sig[0] == -1 && sb.sig[5] == -1);   // ... and cleared for no shape
    CHECK(sb.ensure(s, 128) == GSR_OK && sb.p.cap() == 128);
    sb.release();
    CHECK(!sb.p && sb.p.cap() == 0 && sb.sig[0] == -1 && live_is(0, 0, 0, 1));
}

// A group (DevGroup): every member or none.  grow: `members` allocations in the group's order, a capacity at or below the one held
// costs nothing, and a k-th member that cannot be allocated -- for each k -- leaves the whole group empty with that failure's code.
template <class G, class Ensure, class Holds>
static void group_grows_whole(int members, Ensure&& ensure, Holds&& holds)
{
    G g;
    CHECK(g.cap() == 0 && !holds(g));
    CHECK(ensure(g, 100) == GSR_OK && g.cap() >= 100 && holds(g) && live_is(members, 0, 0, 1));
    const size_t cap = g.cap();
    const long calls = stub_calls;
    CHECK(ensure(g, 100) == GSR_OK && ensure(g, 1) == GSR_OK && ensure(g, cap) == GSR_OK && g.cap() == cap && stub_calls == calls);
    stub_peak[STUB_DEV] = stub_live[STUB_DEV];
    CHECK(ensure(g, cap + 1) == GSR_OK && g.cap() > cap && holds(g) && stub_peak[STUB_DEV] == members && live_is(members, 0, 0, 1));   // released first
    for (int k = 1; k <= members; ++k) {
        stub_fail_kth(k);
        CHECK(ensure(g, g.cap() + 1) == GSR_E_OOM && g.cap() == 0 && !holds(g) && live_is(0, 0, 0, 1));
        CHECK(ensure(g, 10) == GSR_OK && g.cap() >= 10 && holds(g) && live_is(members, 0, 0, 1));
    }
    g.release(); g.release();
    CHECK(g.cap() == 0 && !holds(g) && live_is(0, 0, 0, 1));
    CHECK(ensure(g, 3) == GSR_OK);         // (and the destructor releases what release() did not)
}

static void groups()
{
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    long syncs = stub_syncs;
    group_grows_whole<TileSet>(5, [&](TileSet& g, size_t n) { return g.ensure_drained(s, n); },
                               [](TileSet& g) { return g.tile_work || g.tile_work_a || g.sstart || g.send || g.redo; });
    CHECK(stub_syncs == syncs + 2 + 2 * 5 + 1);                                    // one drain per growth, failed ones included; none otherwise
    {
        TileSet t;
        CHECK(t.ensure_drained(s, 3) == GSR_OK && t.cap() == 3);
        t.tile_work[2].x = 1u; t.tile_work_a[2].x = 1u; t.redo[2] = 1; t.sstart[65536] = 1; t.send[65536] = 1;   // (each member's own size)
    }
    syncs = stub_syncs;
    group_grows_whole<WirePair>(2, [](WirePair& g, size_t n) { return g.ensure(n); }, [](WirePair& g) { return g.zbuf || g.out; });
    {
        WirePair w;
        CHECK(w.ensure(5) == GSR_OK && w.cap() == 5);
        w.zbuf[4] = 1ull; w.out[19] = 1.0f;                                        // (16 bytes of image per pixel)
    }
    const long cleared = stub_errors_cleared;
    group_grows_whole<MortonScratch>(4, [](MortonScratch& g, size_t n) { return g.hold(n); },
                                     [](MortonScratch& g) { return g.kA || g.kB || g.vA || g.vB; });
    CHECK(stub_errors_cleared == cleared + 4 && stub_syncs == syncs);              // a failure clears the runtime's sticky error; nobody drains
    {
        MortonScratch m;
        CHECK(m.hold(800) == GSR_OK && m.cap() == 800 + 100 + 1024);             // an eighth and 1024 beyond the need
        m.kA[1923] = m.kB[1923] = m.vA[1923] = m.vB[1923] = 1u;
        CHECK(m.hold(1924) == GSR_OK && m.cap() == 1924 && m.hold(1925) == GSR_OK && m.cap() == 1925 + 240 + 1024);
    }
    CHECK(live_is(0, 0, 0, 1));
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
    groups();
    CHECK(live_is(0, 0, 0, 0));        // at exit every counter is 0
    std::printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
