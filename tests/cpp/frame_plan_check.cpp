// frame_plan.hpp on the host: the launch decisions of a frame (tests/test_cpp_frame_plan.py).  No frame test sees them -- they
// change the launch order and nothing else -- so they are pinned here, frame by frame, to what the rules gave while they stood
// inline in the launch path.  Plain g++, no HIP.  Prints one "... ok" line per group; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

constexpr int kNone = EngineTrial::kNoRecord, kPipe = EngineTrial::kPipelinePair, kMega = EngineTrial::kMegakernelPair;
const uint64_t kA[3] = {(640ull << 32) | 360, 1, (1ull << 32) | (5ull << 16) | 1};
const uint64_t kB[3] = {(320ull << 32) | 180, 1, (1ull << 32) | (5ull << 16) | 1};

// One AUTO frame of a forking scene as choose_engine runs it: with the trials on, a waiting trial has its events queried and,
// if they have completed (`ready`), gets the verdict; then the engine of the frame.
EngineTrial::Step trial_frame(EngineTrial &t, const uint64_t sig[3], bool trials_on, bool ready, float t_stream, float t_mega, int *queries = nullptr) {
    if (trials_on && t.waiting(sig)) {
        if (queries) *queries += 1;
        if (ready) t.verdict(t_stream, t_mega);
    }
    return t.next(sig, trials_on);
}

void expect(const EngineTrial::Step &s, bool stream, int record, int frame, const char *what) {
    CHECK(s.stream == stream && s.record == record, "%s, frame %d: {%s, %d}, expected {%s, %d}", what, frame, s.stream ? "pipeline" : "megakernel",
          s.record, stream ? "pipeline" : "megakernel", record);
}

// frames 1-3 of a trial with everything ready
void first_three(EngineTrial &t, const uint64_t sig[3], const char *what) {
    expect(trial_frame(t, sig, true, true, 0.f, 0.f), true, kPipe, 1, what);
    expect(trial_frame(t, sig, true, true, 0.f, 0.f), false, kNone, 2, what);
    expect(trial_frame(t, sig, true, true, 0.f, 0.f), false, kMega, 3, what);
}

void trial() {
    CHECK(EngineTrial::applies(RTK_TRACE_AUTO, true, false), "AUTO on a forking scene");
    CHECK(!EngineTrial::applies(RTK_TRACE_AUTO, false, false) && !EngineTrial::applies(RTK_TRACE_AUTO, true, true) &&
          !EngineTrial::applies(RTK_TRACE_STREAM, true, false) && !EngineTrial::applies(RTK_TRACE_GROUP4, true, false), "fork-free, stats, other modes");
    {   // the megakernel wins: 4 and later the megakernel, untimed, and no further query
        EngineTrial t;
        first_three(t, kA, "megakernel wins");
        int queries = 0;
        for (int f = 4; f <= 40; ++f) expect(trial_frame(t, kA, true, true, 2.0f, 1.0f, &queries), false, kNone, f, "megakernel wins");
        CHECK(queries == 1 && t.state == 5, "queries %d state %d", queries, t.state);
    }
    {   // the pipeline wins
        EngineTrial t;
        first_three(t, kA, "pipeline wins");
        for (int f = 4; f <= 40; ++f) expect(trial_frame(t, kA, true, true, 1.0f, 2.0f), true, kNone, f, "pipeline wins");
        CHECK(t.state == 4, "state %d", t.state);
    }
    {   // a tie keeps the pipeline
        EngineTrial t;
        first_three(t, kA, "tie");
        for (int f = 4; f <= 8; ++f) expect(trial_frame(t, kA, true, true, 1.5f, 1.5f), true, kNone, f, "tie");
        CHECK(t.state == 4, "state %d", t.state);
    }
    {   // events not ready for two frames: those go to the pipeline, untimed, and each asks again
        EngineTrial t;
        first_three(t, kA, "not ready");
        int queries = 0;
        expect(trial_frame(t, kA, true, false, 2.0f, 1.0f, &queries), true, kNone, 4, "not ready");
        expect(trial_frame(t, kA, true, false, 2.0f, 1.0f, &queries), true, kNone, 5, "not ready");
        CHECK(t.state == 3 && queries == 2, "state %d queries %d", t.state, queries);
        for (int f = 6; f <= 9; ++f) expect(trial_frame(t, kA, true, true, 2.0f, 1.0f, &queries), false, kNone, f, "not ready");
        CHECK(queries == 3, "queries %d", queries);
    }
    {   // abandon on frame 1 (fresh queues): the pipeline is timed again on the next frame, then the trial as usual
        EngineTrial t;
        expect(trial_frame(t, kA, true, true, 0.f, 0.f), true, kPipe, 1, "abandon");
        t.abandon();
        CHECK(t.state == 0, "state %d", t.state);
        first_three(t, kA, "after abandon");
        expect(trial_frame(t, kA, true, true, 2.0f, 1.0f), false, kNone, 4, "after abandon");
    }
    {   // a new signature mid-trial starts over, from every state; the old one starts over too when it comes back
        for (int at = 1; at <= 5; ++at) {
            EngineTrial t;
            for (int f = 1; f <= at; ++f) trial_frame(t, kA, true, true, 2.0f, 1.0f);
            int queries = 0;
            expect(trial_frame(t, kB, true, true, 2.0f, 1.0f, &queries), true, kPipe, at + 1, "new signature");
            CHECK(queries == 0 && t.state == 1 && std::memcmp(t.sig, kB, sizeof(kB)) == 0, "at %d: queries %d state %d", at, queries, t.state);
            expect(trial_frame(t, kA, true, true, 2.0f, 1.0f), true, kPipe, at + 2, "old signature again");
        }
    }
    {   // trials off: the pipeline, nothing timed, nothing advanced; a new signature still resets
        EngineTrial t;
        for (int f = 1; f <= 5; ++f) expect(trial_frame(t, kA, false, true, 2.0f, 1.0f), true, kNone, f, "trials off");
        CHECK(t.state == 0, "state %d", t.state);
        first_three(t, kA, "trials on again");
        trial_frame(t, kA, true, true, 2.0f, 1.0f);
        CHECK(t.state == 5, "state %d", t.state);
        expect(trial_frame(t, kA, false, true, 2.0f, 1.0f), true, kNone, 5, "trials off keeps the state");
        CHECK(t.state == 5, "state %d", t.state);
        expect(trial_frame(t, kB, false, true, 2.0f, 1.0f), true, kNone, 6, "trials off, new signature");
        CHECK(t.state == 0 && std::memcmp(t.sig, kB, sizeof(kB)) == 0, "state %d", t.state);
    }
    {   // a stats frame in between does not apply: the trial is where it was
        EngineTrial t;
        expect(trial_frame(t, kA, true, true, 0.f, 0.f), true, kPipe, 1, "stats between");
        expect(trial_frame(t, kA, true, true, 0.f, 0.f), false, kNone, 2, "stats between");
        if (EngineTrial::applies(RTK_TRACE_AUTO, true, true)) trial_frame(t, kB, true, true, 0.f, 0.f);
        expect(trial_frame(t, kA, true, true, 0.f, 0.f), false, kMega, 3, "stats between");
    }
    if (!g_failed) std::printf("trial ok\n");
}

const uint64_t kS[5] = {(44ull << 32) | 28, 1, (1ull << 32) | (5ull << 16), (64ull << 32) | (1ull << 16) | RTK_TRACE_GROUP4, 0};
const uint64_t kT[5] = {(24ull << 32) | 20, 1, (1ull << 32) | (5ull << 16), (64ull << 32) | (1ull << 16) | RTK_TRACE_GROUP4, 0};

struct Frame { bool prior, resort, use_order; unsigned n_wgs; int queries; };

// One megakernel frame as render_megakernel runs it: the step, then -- with an order in use -- the query if the count is
// awaited, and the workgroups of the launch.  `ready`: what the query would answer; `word`: the pinned word.
Frame order_frame(OrderState &st, const uint64_t sig[5], int mode, bool stats, bool regions, const OrderState::Knobs &k, bool ready, uint32_t word) {
    const OrderState::Step s = st.step(sig, mode, stats, regions, k);
    Frame f = {s.prior, s.resort, s.use_order, 0u, 0};
    if (s.use_order) {
        bool r = false;
        if (st.awaits_count()) { f.queries = 1; r = ready; }
        f.n_wgs = st.workgroups(r, &word);
    }
    return f;
}

void order_sequences() {
    const OrderState::Knobs k16 = {true, 16}, k1 = {true, 1};
    {   // resort_every 16: prior, sort, 3-17 reuse, 18 sort, 34 sort.  The read-back of a sort is seen complete one frame later.
        OrderState st;
        for (int f = 1; f <= 40; ++f) {
            const bool sorts = f == 2 || f == 18 || f == 34;
            const Frame r = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, !sorts, uint32_t(100 + f));
            CHECK(r.prior == (f == 1) && r.resort == sorts && r.use_order, "every 16, frame %d: prior %d resort %d use %d", f, r.prior, r.resort, r.use_order);
            // no count on the prior's frame and on a frame that sorts; the frame after a sort sees the read-back and asks no more
            const unsigned expect_wgs = (f == 1 || sorts) ? 0u : uint32_t(100 + f);
            const int expect_q = (sorts || f == 3 || f == 19 || f == 35) ? 1 : 0;
            CHECK(r.n_wgs == expect_wgs && r.queries == expect_q, "every 16, frame %d: n_wgs %u queries %d", f, r.n_wgs, r.queries);
        }
        CHECK(st.age == 7 && st.order_valid && st.valid, "age %u", st.age);
    }
    {   // resort_every 1: every frame from the second sorts
        OrderState st;
        for (int f = 1; f <= 40; ++f) {
            const Frame r = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k1, false, 7u);
            CHECK(r.prior == (f == 1) && r.resort == (f >= 2) && r.use_order && r.n_wgs == 0, "every 1, frame %d: prior %d resort %d", f, r.prior, r.resort);
        }
    }
    {   // the count stays 0 until the read-back is seen, however long that takes, and is 0 again after the next sort
        OrderState st;
        order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, false, 9u);
        order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, false, 9u);
        for (int f = 3; f <= 6; ++f) {
            const Frame r = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, false, 9u);
            CHECK(r.n_wgs == 0 && r.queries == 1 && !r.resort, "frame %d: n_wgs %u queries %d", f, r.n_wgs, r.queries);
        }
        for (int f = 7; f <= 17; ++f) {
            const Frame r = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, true, 9u);
            CHECK(r.n_wgs == 9u && r.queries == (f == 7 ? 1 : 0), "frame %d: n_wgs %u queries %d", f, r.n_wgs, r.queries);
        }
        const Frame r18 = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, false, 9u);
        CHECK(r18.resort && r18.n_wgs == 0 && st.nwgs_pending && !st.nwgs_known, "frame 18: resort %d n_wgs %u", r18.resort, r18.n_wgs);
        const Frame r19 = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, true, 11u);
        CHECK(!r19.resort && r19.n_wgs == 11u, "frame 19: n_wgs %u", r19.n_wgs);
    }
    {   // another shape at frame 5 and back: each is a first frame (prior, no count), the one after sorts
        OrderState st;
        for (int f = 1; f <= 9; ++f) {
            const uint64_t *sig = f == 5 ? kT : kS;
            const Frame r = order_frame(st, sig, RTK_TRACE_GROUP4, false, false, k16, f != 2 && f != 7, 5u);
            const bool first = f == 1 || f == 5 || f == 6, sorts = f == 2 || f == 7;
            CHECK(r.prior == first && r.resort == sorts && r.use_order && r.n_wgs == ((first || sorts) ? 0u : 5u), "shape change, frame %d: prior %d resort %d n_wgs %u",
                  f, r.prior, r.resort, r.n_wgs);
        }
    }
    {   // forget(): the next frame of the same shape is a first frame again
        OrderState st;
        for (int f = 1; f <= 4; ++f) order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, f != 2, 5u);
        st.forget();
        CHECK(!st.valid && !st.order_valid && st.age == 0 && !st.nwgs_pending && !st.nwgs_known, "forget");
        const Frame r = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, true, 5u);
        CHECK(r.prior && !r.resort && r.n_wgs == 0 && r.queries == 0, "after forget: prior %d resort %d n_wgs %u", r.prior, r.resort, r.n_wgs);
        const Frame r2 = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, false, 5u);
        CHECK(!r2.prior && r2.resort, "second frame after forget");
    }
    {   // no prior: the knob off, eight waves, per-ray statistics, a regions launch.  The first frame runs in the natural order, the second sorts.
        const OrderState::Knobs off = {false, 16};
        struct { int mode; bool stats, regions; const OrderState::Knobs *k; } cases[] = {
            {RTK_TRACE_GROUP4, false, false, &off}, {RTK_TRACE_GROUP8, false, false, &k16}, {RTK_TRACE_GROUP16, false, false, &k16},
            {RTK_TRACE_GROUP4, true, false, &k16}, {RTK_TRACE_GROUP4, false, true, &k16}};
        int i = 0;
        for (const auto &c : cases) {
            OrderState st;
            const OrderState::Step s1 = st.step(kS, c.mode, c.stats, c.regions, *c.k);
            CHECK(!s1.prior && !s1.resort && !s1.use_order && st.valid && !st.order_valid, "no prior, case %d, frame 1", i);
            const OrderState::Step s2 = st.step(kS, c.mode, c.stats, c.regions, *c.k);
            CHECK(!s2.prior && s2.resort && s2.use_order && st.order_valid, "no prior, case %d, frame 2", i);
            i += 1;
        }
    }
    if (!g_failed) std::printf("order ok\n");
}

void order_capacity() {
    const OrderState::Knobs k16 = {true, 16};
    {   // large enough: kept; growth: the tables hold nothing until re-made, and the next frame is a first frame
        OrderState st;
        CHECK(st.capacity(64, false, 0) == 64 && st.units == 0, "first allocation");
        st.units = 64;
        for (int f = 1; f <= 3; ++f) order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, f == 3, 5u);
        CHECK(st.capacity(50, false, 0) == 64 && st.capacity(64, false, 0) == 64 && st.units == 64 && st.valid && st.order_valid, "kept");
        CHECK(st.capacity(100, false, 0) == 100 && st.units == 0 && !st.valid && !st.order_valid, "growth clears the order");
        st.units = 100;
        const Frame r = order_frame(st, kS, RTK_TRACE_GROUP4, false, false, k16, true, 5u);
        CHECK(r.prior && !r.resort && r.n_wgs == 0, "after growth: prior %d resort %d n_wgs %u", r.prior, r.resort, r.n_wgs);
    }
    // the scene's native block count: on the frame table's first allocation only, when larger and <= 2^24
    const uint64_t M = 1ull << 24;
    { OrderState st; CHECK(st.capacity(64, true, 32) == 64, "native below"); }
    { OrderState st; CHECK(st.capacity(64, true, 64) == 64, "native equal"); }
    { OrderState st; CHECK(st.capacity(64, true, 4050) == 4050, "native above"); }
    { OrderState st; CHECK(st.capacity(64, true, M) == M, "native 2^24"); }
    { OrderState st; CHECK(st.capacity(64, true, M + 1) == 64, "native beyond 2^24"); }
    { OrderState st; CHECK(st.capacity(64, false, 4050) == 64, "not the frame table"); }
    { OrderState st; st.units = 64; CHECK(st.capacity(100, true, 4050) == 100, "not the first allocation"); }

    const size_t below = 9000;
    CHECK(OrderState::frame_mode(RTK_TRACE_AUTO, below - 1, below) == RTK_TRACE_GROUP8, "AUTO below the knob");
    CHECK(OrderState::frame_mode(RTK_TRACE_AUTO, below, below) == RTK_TRACE_GROUP4, "AUTO at the knob");
    CHECK(OrderState::frame_mode(RTK_TRACE_AUTO, below + 1, below) == RTK_TRACE_GROUP4, "AUTO above the knob");
    CHECK(OrderState::frame_mode(RTK_TRACE_AUTO, 0, 0) == RTK_TRACE_GROUP4, "knob 0: never eight waves");
    for (int m : {RTK_TRACE_GROUP4, RTK_TRACE_GROUP8, RTK_TRACE_GROUP16, RTK_TRACE_WAVE, RTK_TRACE_LANE})
        CHECK(OrderState::frame_mode(m, 1, below) == m && OrderState::frame_mode(m, below + 1, below) == m, "mode %d is kept", m);
    // the retired two-pass engine's mode: GROUP4's frames whatever the block count (never eight waves, never itself)
    for (size_t units : {size_t(0), size_t(1), below - 1, below, below + 1})
        CHECK(OrderState::frame_mode(RTK_TRACE_TWOPASS, units, below) == RTK_TRACE_GROUP4, "TWOPASS at %zu units", units);
    CHECK(OrderState::frame_mode(RTK_TRACE_TWOPASS, 1, 0) == RTK_TRACE_GROUP4, "TWOPASS, knob 0");
    CHECK(OrderState::frame_mode(RTK_TRACE_STREAM, 1, below) == RTK_TRACE_STREAM, "STREAM is kept");
    if (!g_failed) std::printf("capacity ok\n");
}

void geometry_and_views() {
    FrameGeom g = {};
    g.width = 44; g.height = 28; g.bucket = 64; g.blocks_side = 8; g.buckets_per_rank = 1; g.rank = 0; g.world = 1;
    CHECK(g.blocks() == 64, "one bucket of 64: %zu", g.blocks());
    g.buckets_per_rank = 3; g.blocks_side = 3;                              // bucket 20: ragged blocks
    CHECK(g.blocks() == 27 && g.blocks_of(510) == 4590, "three buckets of 3x3: %zu", g.blocks());
    g.buckets_per_rank = 0xFFFFFFFFu; g.blocks_side = 8192;                 // no 32-bit product on the way
    CHECK(g.blocks_of(g.buckets_per_rank) == 0xFFFFFFFFull * 8192 * 8192, "wide product");
    uint64_t sig[3];
    g.width = 1920; g.height = 1080; g.rank = 3; g.world = 8;
    shape_sig(g, 16, 5, 2, sig);
    CHECK(sig[0] == ((1920ull << 32) | 1080) && sig[1] == ((3ull << 32) | 8) && sig[2] == ((16ull << 32) | (5ull << 16) | 2), "shape_sig");
    shape_sig(g, 1, 16, 32767, sig);
    CHECK(sig[2] == ((1ull << 32) | (16ull << 16) | 32767), "shape_sig at the largest depth and gi");

    struct { size_t n, per_view, limit, per_launch, n_parts; } cases[] = {
        {0, 10, 100, 10, 0}, {1, 10, 100, 10, 1}, {10, 10, 100, 10, 1}, {25, 10, 100, 10, 3}, {10, 30, 100, 3, 4},     // per_view < limit
        {0, 100, 100, 1, 0}, {1, 100, 100, 1, 1}, {5, 100, 100, 1, 5},                                                  // =
        {0, 150, 100, 1, 0}, {1, 150, 100, 1, 1}, {7, 150, 100, 1, 7},                                                  // >
        {5, 64, 131072, 2048, 1}, {5, 64, 128, 2, 3}, {5, 51, 100, 1, 5}};
    for (const auto &c : cases) {
        const ViewsLaunches v = views_launches(c.n, c.per_view, c.limit);
        CHECK(v.per_launch == c.per_launch && v.n_parts == c.n_parts, "views n %zu per_view %zu limit %zu: {%zu, %zu}", c.n, c.per_view, c.limit, v.per_launch, v.n_parts);
    }
    if (!g_failed) std::printf("geometry and views ok\n");
}

StreamWsShape ws(size_t pixels, size_t nodes, size_t lights, int lanes, bool sum) {
    StreamWsShape s;
    s.pixels = pixels; s.nodes = nodes; s.lights = lights; s.lanes = lanes; s.sum = sum;
    return s;
}
bool equal(const StreamWsShape &a, const StreamWsShape &b) {
    return a.pixels == b.pixels && a.nodes == b.nodes && a.lights == b.lights && a.lanes == b.lanes && a.sum == b.sum;
}

void stream_ws() {
    StreamWsShape have;
    // nothing yet: even the empty request (0 lights and 0 lanes count as 1) is not covered
    CHECK(!have.covers(ws(0, 0, 0, 0, false)), "empty workspace covers nothing");
    have = have.grown(ws(0, 0, 0, 0, false));
    CHECK(equal(have, ws(0, 0, 1, 1, false)) && have.covers(ws(0, 0, 0, 0, false)) && have.covers(ws(0, 0, 1, -3, false)), "raised to one light, one lane");
    have = have.grown(ws(1000, 5000, 2, 1, false));
    CHECK(equal(have, ws(1000, 5000, 2, 1, false)), "first frame");
    // one field at a time: not covered, grown in that field alone, then covered; smaller requests change nothing
    const StreamWsShape steps[] = {ws(1001, 1, 0, 0, false), ws(1, 5001, 0, 0, false), ws(1, 1, 3, 0, false), ws(1, 1, 0, 2, false), ws(1, 1, 0, 0, true)};
    const StreamWsShape after[] = {ws(1001, 5000, 2, 1, false), ws(1001, 5001, 2, 1, false), ws(1001, 5001, 3, 1, false), ws(1001, 5001, 3, 2, false),
                                   ws(1001, 5001, 3, 2, true)};
    for (int i = 0; i < 5; ++i) {
        CHECK(!have.covers(steps[i]), "step %d is not covered", i);
        have = have.grown(steps[i]);
        CHECK(equal(have, after[i]) && have.covers(steps[i]), "step %d: {%zu, %zu, %zu, %d, %d}", i, have.pixels, have.nodes, have.lights, have.lanes, int(have.sum));
    }
    CHECK(have.covers(ws(1001, 5001, 3, 2, true)) && have.covers(ws(0, 0, 0, 0, false)) && equal(have.grown(ws(5, 5, 1, 1, false)), have), "never shrunk");
    CHECK(!ws(0, 0xFFFFFFF0ull, 1, 1, false).refused() && ws(0, 0xFFFFFFF1ull, 1, 1, false).refused(), "the 32-bit node id bound");
    CHECK(have.grown(ws(0, 0xFFFFFFF1ull, 0, 0, false)).refused() && !have.grown(ws(1ull << 40, 0xFFFFFFF0ull, 0, 0, false)).refused(), "refusal is of the grown shape's nodes");
    CHECK(StreamWsShape::hit_cap(0) == 64 && StreamWsShape::hit_cap(1001) == 564 && StreamWsShape::hit_cap(0xFFFFFFF0ull) == 0x7FFFFFF8ull + 64, "hit_cap");
    if (!g_failed) std::printf("stream workspace ok\n");
}

}  // namespace

int main() {
    trial();
    order_sequences();
    order_capacity();
    geometry_and_views();
    stream_ws();
    if (!g_failed) std::printf("all ok\n");
    return g_failed ? 1 : 0;
}
