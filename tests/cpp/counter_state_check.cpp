// frame_plan.hpp CounterState on the host (tests/test_cpp_counter_state.py): which of an accel's two counter blocks a frame counts
// into, whether a fill is issued in front of it and whether its kernel is handed the other block to clear.  The sequences are the
// launch path's (api_frame.hip render_frame_impl, api_order.hip order_launch; api_batch.hip): a steady frame is frame(stream, true), every other
// user of the counters is forget() or frame(stream, false), an error is forget() behind the frame, and a frame of a new shape
// forgets behind itself (CounterState::after_order, given OrderState's step).  Then OrderState's two sets of launch lists across the
// re-sorts: which set a frame reads, which a sort writes, and whether that sort is in front of the frame or behind it.  Plain g++, no HIP.  One "... ok" line per group; a failure
// is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "frame_plan.hpp"

using namespace rtk;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s (line %d): ", #cond, __LINE__);           \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
            if (++g_failed > 20) std::exit(1);                               \
        }                                                                    \
    } while (0)

int g_s1, g_s2;                                   // two streams: only their addresses matter
const void *const S1 = &g_s1, *const S2 = &g_s2, *const S0 = nullptr;      // (and the null stream)

void expect(const CounterState::Step &s, int current, bool fill, bool carry, const char *what, int frame) {
    CHECK(s.current == current && s.fill == fill && s.carry == carry, "%s, frame %d: {block %d, fill %d, carry %d}, expected {%d, %d, %d}", what, frame,
          s.current, int(s.fill), int(s.carry), current, int(fill), int(carry));
}

// a steady frame as render_frame_impl + order_launch run it: the counter step, then the order step of the frame's shape, which
// CounterState::after_order is told of.  Returns what the frame did, and the order step in *os.
CounterState::Step steady_frame(CounterState &c, OrderState &o, const void *s, const uint64_t sig[5], OrderState::Step *os = nullptr) {
    const CounterState::Step r = c.frame(s, true);
    const OrderState::Step st = o.step(sig, RTK_TRACE_GROUP4, false, false, {true, 16});
    c.after_order(st);                             // (the shipped rule: a frame of a new shape forgets behind itself)
    if (os) *os = st;
    return r;
}

void one_stream() {
    for (const void *s : {S1, S0}) {              // a stream of the caller's, and the null stream: a stream like any other
        CounterState c;
        expect(c.frame(s, true), 0, true, true, "first frame of an accel", 1);
        for (int f = 2; f <= 40; ++f) expect(c.frame(s, true), (f + 1) % 2, false, true, "one stream", f);
        CHECK(c.other_zero && c.stream == s, "knowledge held");
    }
    if (!g_failed) std::printf("one stream ok\n");
}

void stream_switch() {
    CounterState c;
    expect(c.frame(S1, true), 0, true, true, "switch", 1);
    expect(c.frame(S1, true), 1, false, true, "switch", 2);
    expect(c.frame(S2, true), 1, true, true, "another stream fills the block in use", 3);
    expect(c.frame(S2, true), 0, false, true, "and is steady from its second frame", 4);
    expect(c.frame(S1, true), 0, true, true, "back", 5);
    // alternating every frame: never steady, never a flip
    for (int f = 6; f <= 12; ++f) expect(c.frame(f % 2 ? S1 : S2, true), 0, true, true, "alternating", f);
    expect(c.frame(S0, true), 0, true, true, "the null stream is another stream", 13);
    if (!g_failed) std::printf("stream switch ok\n");
}

// every other user of the counters between two steady frames: the frame behind it fills the block in use, the one after that is steady
void interleaved() {
    struct Case { const char *what; bool as_frame; const void *stream; } cases[] = {
        {"the streaming engine's frame", true, S1},                       // frame(s, false): !stream is part of `carries`
        {"a collect_stats frame", true, S1},
        {"a view of a view-after-view rtk_render_views", true, S1},       // render_frame_impl(..., steady = false)
        {"the fallback launch with only_if (a streaming frame)", true, S1},
        {"rtk_render_views as launches (zero_counters)", false, S1},
        {"rtk_render_regions (zero_counters)", false, S1},
        {"intersect_stats", false, S0},
        {"rtk_accel_occluded with a count", false, S0},
        {"rtk_accel_radiance", false, S1},
        {"forget_orders: camera, vertices, geometry, lights, materials", false, S1},
    };
    for (const Case &k : cases) {
        CounterState c;
        c.frame(S1, true);
        expect(c.frame(S1, true), 1, false, true, k.what, 2);
        if (k.as_frame) expect(c.frame(k.stream, false), 1, true, false, k.what, 3);       // fills and uses the block in use; hands nothing over
        else c.forget();
        CHECK(!c.other_zero && c.current == 1, "%s: knowledge forgotten, block kept", k.what);
        expect(c.frame(S1, true), 1, true, true, k.what, 4);
        expect(c.frame(S1, true), 0, false, true, k.what, 5);
        expect(c.frame(S1, true), 1, false, true, k.what, 6);
    }
    {   // several of them in a row, and a non-carrying frame on another stream
        CounterState c;
        c.frame(S1, true); c.frame(S1, true);
        c.forget(); c.forget();
        expect(c.frame(S2, false), 1, true, false, "stats frame on another stream", 3);
        expect(c.frame(S2, false), 1, true, false, "and again", 4);
        expect(c.frame(S2, true), 1, true, true, "first steady frame behind them", 5);
        expect(c.frame(S2, true), 0, false, true, "second", 6);
    }
    if (!g_failed) std::printf("interleaved ok\n");
}

void error_in_the_middle() {
    {   // the launch of a steady frame that had flipped fails: render_frame_impl forgets; the block stays the one it flipped to
        CounterState c;
        c.frame(S1, true); c.frame(S1, true);
        expect(c.frame(S1, true), 0, false, true, "the frame that fails", 3);
        c.forget();
        expect(c.frame(S1, true), 0, true, true, "behind the error", 4);
        expect(c.frame(S1, true), 1, false, true, "steady again", 5);
    }
    {   // the first frame of an accel fails
        CounterState c;
        expect(c.frame(S1, true), 0, true, true, "fails", 1);
        c.forget();
        expect(c.frame(S1, true), 0, true, true, "behind the error", 2);
        expect(c.frame(S1, true), 1, false, true, "steady", 3);
    }
    if (!g_failed) std::printf("error ok\n");
}

const uint64_t kS[5] = {(44ull << 32) | 28, 1, (1ull << 32) | (5ull << 16), (64ull << 32) | (1ull << 16) | RTK_TRACE_GROUP4, 0};
const uint64_t kT[5] = {(24ull << 32) | 20, 1, (1ull << 32) | (5ull << 16), (64ull << 32) | (1ull << 16) | RTK_TRACE_GROUP4, 0};

void shapes_and_resorts() {
    {   // 40 frames of one shape: the prior's frame and the one behind it fill, then no frame does -- not the ones that re-sort
        // (2, 18, 34) either -- and the blocks alternate
        CounterState c;
        OrderState o;
        int current = 0, sorts = 0;
        for (int f = 1; f <= 40; ++f) {
            OrderState::Step os;
            const CounterState::Step r = steady_frame(c, o, S1, kS, &os);
            const bool fill = f <= 2;
            if (!fill) current ^= 1;
            expect(r, current, fill, true, "one shape", f);
            CHECK(os.resort == (f == 2 || f == 18 || f == 34) && os.use_order, "frame %d: resort %d", f, int(os.resort));
            sorts += os.resort ? 1 : 0;
        }
        CHECK(sorts == 3, "re-sorts %d", sorts);
    }
    {   // another shape at frame 6 and back at 7: each is a first frame of its shape and forgets behind itself
        CounterState c;
        OrderState o;
        const bool fills[] = {true, true, false, false, false, false /* 6: the new shape's own frame is still steady */, true, true, false, false};
        int current = 0;
        for (int f = 1; f <= 10; ++f) {
            const CounterState::Step r = steady_frame(c, o, S1, f == 6 ? kT : kS);
            if (!fills[f - 1]) current ^= 1;
            expect(r, current, fills[f - 1], true, "shape change", f);
        }
    }
    {   // OrderState::forget() comes with CounterState::forget() (accel.hpp forget_orders)
        CounterState c;
        OrderState o;
        for (int f = 1; f <= 5; ++f) steady_frame(c, o, S1, kS);
        o.forget(); c.forget();
        expect(steady_frame(c, o, S1, kS), c.current, true, true, "behind forget_orders: the prior's frame", 6);
        expect(steady_frame(c, o, S1, kS), c.current, true, true, "the frame that sorts", 7);
        const int before = c.current;
        expect(steady_frame(c, o, S1, kS), before ^ 1, false, true, "steady", 8);
    }
    if (!g_failed) std::printf("shapes and resorts ok\n");
}

// Which of the two sets of lists a frame reads, and which set a sort writes, in front of the frame or behind it (OrderState::Step).
void expect_sets(const OrderState::Step &s, int reads, bool front, bool behind, const char *what, int frame) {
    CHECK(s.read_set == reads && s.sort_front == front && s.sort_behind == behind && s.write_set == (reads ^ 1),
          "%s, frame %d: {reads %d, front %d, behind %d, writes %d}, expected {%d, %d, %d, %d}", what, frame, s.read_set, int(s.sort_front),
          int(s.sort_behind), s.write_set, reads, int(front), int(behind), reads ^ 1);
}

void list_sets() {
    const OrderState::Knobs k16 = {true, 16}, k1 = {true, 1};
    {   // 40 frames, re-sort every 16: the prior writes set 0 for frame 1; the shape's first sort is in front of frame 2, into set 0;
        // the list frame 18 starts on is sorted behind frame 17 into set 1, the one of frame 34 behind frame 33 into set 0 again.
        // No sort is in front of a frame but the first, and a frame never reads the set a sort launched with it writes.
        OrderState o;
        for (int f = 1; f <= 40; ++f) {
            const OrderState::Step s = o.step(kS, RTK_TRACE_GROUP4, false, false, k16);
            expect_sets(s, f < 18 ? 0 : f < 34 ? 1 : 0, f == 2, f == 17 || f == 33, "every 16", f);
            CHECK(s.resort == (f == 2 || f == 18 || f == 34) && s.prior == (f == 1), "every 16, frame %d: resort %d prior %d", f, int(s.resort), int(s.prior));
            // the length of the list a frame starts on is awaited from that frame on (the copy was enqueued behind the sort)
            CHECK(o.awaits_count() == (f == 2 || f == 18 || f == 34), "frame %d awaits %d", f, int(o.awaits_count()));
            uint32_t word = 7u;
            CHECK(o.workgroups(true, &word) == (f >= 2 ? 7u : 0u), "frame %d", f);
        }
    }
    {   // re-sort every frame: a sort behind every frame from the second, the sets alternate
        OrderState o;
        for (int f = 1; f <= 12; ++f) {
            const OrderState::Step s = o.step(kS, RTK_TRACE_GROUP4, false, false, k1);
            expect_sets(s, f <= 2 ? 0 : (f % 2), f == 2, f >= 2, "every 1", f);
        }
    }
    {   // another shape behind a frame that sorted behind itself (17): that list is dropped, the new shape starts at set 0 with its own
        // first sort in front of its second frame; the same behind forget() and behind a growth of the tables
        for (int how = 0; how < 3; ++how) {
            OrderState o;
            o.units = 64;
            for (int f = 1; f <= 17; ++f) o.step(kS, RTK_TRACE_GROUP4, false, false, k16);
            for (int f = 18; f <= 20; ++f) o.step(kS, RTK_TRACE_GROUP4, false, false, k16);
            CHECK(o.set == 1, "reads set %d", o.set);
            for (int f = 21; f <= 32; ++f) o.step(kS, RTK_TRACE_GROUP4, false, false, k16);
            const OrderState::Step s33 = o.step(kS, RTK_TRACE_GROUP4, false, false, k16);
            expect_sets(s33, 1, false, true, "before the change", 33);
            if (how == 1) o.forget();
            if (how == 2) { CHECK(o.capacity(100, false, 0) == 100, "growth"); o.units = 100; }
            const uint64_t *sig = how == 0 ? kT : kS;
            const OrderState::Step a = o.step(sig, RTK_TRACE_GROUP4, false, false, k16);
            expect_sets(a, 0, false, false, "first frame behind the change", 34);
            CHECK(a.prior && !a.resort, "how %d: prior %d resort %d", how, int(a.prior), int(a.resort));
            expect_sets(o.step(sig, RTK_TRACE_GROUP4, false, false, k16), 0, true, false, "its first sort", 35);
            for (int f = 36; f <= 49; ++f) expect_sets(o.step(sig, RTK_TRACE_GROUP4, false, false, k16), 0, false, false, "reuse", f);
            expect_sets(o.step(sig, RTK_TRACE_GROUP4, false, false, k16), 0, false, true, "sorts behind itself", 50);
            expect_sets(o.step(sig, RTK_TRACE_GROUP4, false, false, k16), 1, false, false, "changes sets", 51);
        }
    }
    if (!g_failed) std::printf("list sets ok\n");
}

}  // namespace

int main() {
    one_stream();
    stream_switch();
    interleaved();
    error_in_the_middle();
    shapes_and_resorts();
    list_sets();
    if (!g_failed) std::printf("all ok\n");
    return g_failed ? 1 : 0;
}
