// csrc/dev_mem.hpp on its own: the growth rules, Buf and Event over a counting malloc source that can be told to fail its k-th
// allocation.  Prints one "... ok" line per group (tests/test_cpp_dev_mem.py reads them) and returns 1 at the first FAILED.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dev_mem.hpp"

using namespace rtk;

namespace {

struct Count {
    static int live, allocs, frees, fail_in;       // fail_in = k > 0: the k-th allocation from now fails (once)
    static int alloc(void **p, size_t bytes) {
        *p = nullptr;
        if (fail_in > 0 && --fail_in == 0) return 2;
        *p = std::malloc(bytes);
        if (!*p) return 2;
        ++allocs; ++live;
        return 0;
    }
    static void free(void *p) { std::free(p); ++frees; --live; }
};
int Count::live = 0, Count::allocs = 0, Count::frees = 0, Count::fail_in = 0;

struct CountEv {
    using handle = void *;
    static int create(handle *h) { return Count::alloc(h, 1); }
    static void destroy(handle h) { Count::free(h); }
};

template <typename T> using B = Buf<T, Count>;
using Ev = Event<CountEv>;

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

constexpr size_t kCap = size_t(1) << 20;           // api_regions.hip kRegionChunkPixels

void rules() {
    const size_t need[5] = {0, 1, 255, 256, 4096};
    const size_t bytes[5] = {257, 257, 638, 640, 6400};            // need + need / 2 + 256, at least one byte needed
    const size_t table[5] = {16, 17, 398, 400, 6160};              // n + n / 2 + 16
    const size_t lights[5] = {8, 9, 390, 392, 6152};               // n + n / 2 + 8
    const size_t capped[5] = {0, 1, 382, 384, 6144};               // n + n / 2
    for (int i = 0; i < 5; ++i) {
        CHECK(grow_exact()(need[i], 4) == need[i]);
        CHECK(set_exactly()(need[i], 4) == need[i]);
        CHECK(grow_bytes()(need[i], 1) == bytes[i]);
        CHECK(grow_table()(need[i], 40) == table[i]);
        CHECK(grow_lights()(need[i], 16) == lights[i]);
        CHECK(grow_capped{kCap}(need[i], 24) == capped[i]);
        // a typed buffer rounds the byte rule up to whole elements, never below it
        for (size_t each : {size_t(4), size_t(24), size_t(48)}) {
            const size_t nb = need[i] * each > 0 ? need[i] * each : 1, rule_bytes = nb + nb / 2 + 256, got = grow_bytes()(need[i], each);
            CHECK(got * each >= rule_bytes && got * each < rule_bytes + each);
        }
    }
    CHECK(grow_capped{kCap}(kCap - 1, 4) == kCap);                 // just under the cap: the cap
    CHECK(grow_capped{kCap}(kCap, 4) == kCap);
    CHECK(grow_capped{kCap}(kCap + 1, 4) == kCap + 1);             // over it: what was asked for, never less
    CHECK(!grow_exact::refit && !grow_bytes::refit && !grow_table::refit && !grow_lights::refit && !grow_capped::refit && set_exactly::refit);
    std::printf("rules %s\n", failures ? "FAILED" : "ok");
}

void reserve() {
    const int f0 = failures;
    B<uint32_t> b;
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(100, grow_table()) == 0 && b.capacity() == 166 && b.get() != nullptr);
    uint32_t *const p = b.get();
    p[165] = 7u;                                                     // (the sanitizers watch the last element)
    const int a0 = Count::allocs, r0 = Count::frees;
    CHECK(b.reserve(1) == 0 && b.reserve(166, grow_bytes()) == 0 && b.reserve(0) == 0);
    CHECK(b.get() == p && b.capacity() == 166 && Count::allocs == a0 && Count::frees == r0);        // within capacity: no call, same pointer
    CHECK(b.reserve(167) == 0 && b.capacity() == 167 && Count::allocs == a0 + 1 && Count::frees == r0 + 1);   // beyond: one free, one alloc
    // an empty request on an empty buffer still makes a valid pointer (grow_dev's "at least 1")
    B<uint8_t> e;
    CHECK(e.reserve(0, grow_bytes()) == 0 && e.get() != nullptr && e.capacity() == 257);
    B<uint8_t> x;
    CHECK(x.reserve(0) == 0 && x.get() != nullptr && x.capacity() == 1);
    b.reset();
    CHECK(b.get() == nullptr && b.capacity() == 0);
    b.reset();                                                       // (twice is harmless)
    std::printf("reserve %s\n", failures == f0 ? "ok" : "FAILED");
}

void exactly() {
    const int f0 = failures;
    B<uint8_t> b;
    CHECK(b.reserve(1000, set_exactly()) == 0 && b.capacity() == 1000);
    const int a0 = Count::allocs;
    CHECK(b.reserve(1000, set_exactly()) == 0 && Count::allocs == a0);                               // the same size: kept
    CHECK(b.reserve(400, set_exactly()) == 0 && b.capacity() == 400 && Count::allocs == a0 + 1);     // smaller: re-made too
    CHECK(b.reserve(401, set_exactly()) == 0 && b.capacity() == 401 && Count::allocs == a0 + 2);
    CHECK(b.reserve(10) == 0 && b.capacity() == 401 && Count::allocs == a0 + 2);                     // (the growing rules keep it)
    std::printf("exactly %s\n", failures == f0 ? "ok" : "FAILED");
}

void failure() {
    const int f0 = failures;
    B<uint32_t> b;
    CHECK(b.reserve(10) == 0);
    Count::fail_in = 1;
    CHECK(b.reserve(20) != 0 && b.get() == nullptr && b.capacity() == 0);      // the old allocation is gone, nothing dangles
    CHECK(b.reserve(5) == 0 && b.get() != nullptr && b.capacity() == 5);       // a later reserve succeeds
    Ev ev;
    Count::fail_in = 1;
    CHECK(ev.ensure() != 0 && ev.get() == nullptr);
    CHECK(ev.ensure() == 0 && ev.get() != nullptr);
    void *const h = ev.get();
    const int a0 = Count::allocs;
    CHECK(ev.ensure() == 0 && ev.get() == h && Count::allocs == a0);            // made once
    // the make-before-drop of api_state.hip reserve_lights: a larger table is made before the old one goes
    B<uint32_t> lights;
    CHECK(lights.reserve(1) == 0);
    uint32_t *const old = lights.get();
    for (int pass = 0; pass < 2; ++pass) {
        B<uint32_t> larger;
        Count::fail_in = pass == 0 ? 1 : 0;
        const int rc = larger.reserve(5, grow_lights());
        if (pass == 0) { CHECK(rc != 0 && lights.get() == old && lights.capacity() == 1); continue; }     // failed: the old table is intact
        CHECK(rc == 0);
        lights.swap(larger);
        CHECK(lights.capacity() == 15 && larger.get() == old && larger.capacity() == 1);
    }
    std::printf("failure %s\n", failures == f0 ? "ok" : "FAILED");
}

void moves() {
    const int f0 = failures;
    B<uint32_t> a, b;
    CHECK(a.reserve(3) == 0 && b.reserve(9) == 0);
    uint32_t *const pa = a.get(), *const pb = b.get();
    B<uint32_t> c(std::move(a));
    CHECK(c.get() == pa && c.capacity() == 3 && a.get() == nullptr && a.capacity() == 0);
    const int r0 = Count::frees;
    c = std::move(b);                                                // (frees what c held)
    CHECK(c.get() == pb && c.capacity() == 9 && b.get() == nullptr && b.capacity() == 0 && Count::frees == r0 + 1);
    a.swap(c);
    CHECK(a.get() == pb && a.capacity() == 9 && c.get() == nullptr && c.capacity() == 0);
    a.swap(a);
    B<uint32_t> &self = a;
    a = std::move(self);
    CHECK(a.get() == pb && a.capacity() == 9 && Count::frees == r0 + 1);
    Ev e1;
    CHECK(e1.ensure() == 0);
    void *const h = e1.get();
    Ev e2(std::move(e1)), e3;
    CHECK(e2.get() == h && e1.get() == nullptr);
    e3 = std::move(e2);
    CHECK(e3.get() == h && e2.get() == nullptr);
    std::printf("moves %s\n", failures == f0 ? "ok" : "FAILED");
}

// the shape of rtk_cost_feedback: three buffers and an event, in a vector that is resized (its elements move)
struct Feedback { B<uint32_t> cost, order; B<uint8_t> bins; Ev ev; size_t units = 0; };

void vectors() {
    const int f0 = failures, live0 = Count::live;
    {
        std::vector<Feedback> v;
        auto fill = [](Feedback &f, size_t n) { CHECK(f.cost.reserve(n) == 0 && f.order.reserve(2 * n + 12) == 0 && f.bins.reserve(n) == 0 && f.ev.ensure() == 0); f.units = n; };
        v.resize(1);
        fill(v[0], 10);
        uint32_t *const p0 = v[0].cost.get();
        v.resize(3);
        fill(v[1], 20); fill(v[2], 30);
        v.resize(40);                                                // (past any capacity: every element moves)
        CHECK(v[0].cost.get() == p0 && v[0].cost.capacity() == 10 && v[2].order.capacity() == 72 && v[39].cost.get() == nullptr);
        CHECK(Count::live == live0 + 12);
    }
    CHECK(Count::live == live0);
    std::printf("vector %s\n", failures == f0 ? "ok" : "FAILED");
}

// the shape of accel.hpp GeomBufs: swapped member-wise under a mask
struct Geom {
    B<uint32_t> nodes, fast, occl;
    void swap(Geom &o, bool with_fast, bool with_occl) { nodes.swap(o.nodes); if (with_fast) fast.swap(o.fast); if (with_occl) occl.swap(o.occl); }
};

void masked_swap() {
    const int f0 = failures;
    Geom act, spare;
    CHECK(act.nodes.reserve(1) == 0 && act.fast.reserve(2) == 0 && act.occl.reserve(3) == 0);
    CHECK(spare.nodes.reserve(11) == 0 && spare.fast.reserve(12) == 0 && spare.occl.reserve(13) == 0);
    uint32_t *const an = act.nodes.get(), *const af = act.fast.get(), *const ao = act.occl.get();
    uint32_t *const sn = spare.nodes.get(), *const sf = spare.fast.get(), *const so = spare.occl.get();
    act.swap(spare, false, true);
    CHECK(act.nodes.get() == sn && act.nodes.capacity() == 11 && spare.nodes.get() == an && spare.nodes.capacity() == 1);
    CHECK(act.fast.get() == af && act.fast.capacity() == 2 && spare.fast.get() == sf && spare.fast.capacity() == 12);       // masked out: stays
    CHECK(act.occl.get() == so && act.occl.capacity() == 13 && spare.occl.get() == ao && spare.occl.capacity() == 3);
    act.swap(spare, true, false);
    CHECK(act.nodes.get() == an && act.fast.get() == sf && act.fast.capacity() == 12 && act.occl.get() == so && spare.occl.get() == ao);
    std::printf("masked swap %s\n", failures == f0 ? "ok" : "FAILED");
}

}  // namespace

int main() {
    rules();
    reserve();
    exactly();
    failure();
    moves();
    vectors();
    masked_swap();
    // everything above has gone out of scope: nothing may be left, whether or not a leak detector is watching
    std::printf("live %d allocs %d frees %d\n", Count::live, Count::allocs, Count::frees);
    if (Count::live != 0 || Count::allocs != Count::frees || Count::allocs == 0) { std::printf("FAILED leak\n"); return 1; }
    if (failures) return 1;
    std::printf("all ok\n");
    return 0;
}
