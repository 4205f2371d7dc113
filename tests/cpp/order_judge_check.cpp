// csrc/order_judge.hpp (keep or take) and what csrc/frame_plan.hpp OrderState gained with it: the stretched re-sort schedule, the
// judge's frames and the count that is pending again behind a judge.  Stand-alone, no HIP.  Prints one "... ok" line per group.
#include <cstdio>
#include <vector>

#include "frame_plan.hpp"
#include "order_judge.hpp"

using namespace rtk;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failed += 1; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

namespace {

void the_rule() {
    // faster, equal, slower: no margin
    Verdict v = judge_order({18000u, 17200u}, kJudgeByScore);
    CHECK(v.take && v.after.champion == 17200u && v.after.challenger == 17200u, "faster: take %d champion %u", v.take, v.after.champion);
    v = judge_order({18000u, 18000u}, kJudgeByScore);
    CHECK(v.take && v.after.champion == 18000u, "equal: take %d champion %u", v.take, v.after.champion);
    v = judge_order({18000u, 18001u}, kJudgeByScore);
    CHECK(!v.take && v.after.champion == 18000u && v.after.challenger == 18001u, "one tick slower: take %d champion %u", v.take, v.after.champion);
    v = judge_order({17200u, 20300u}, kJudgeByScore);
    CHECK(!v.take && v.after.champion == 17200u && v.after.challenger == 20300u, "slower: take %d", v.take);
    // no champion yet: whatever comes is taken and brings its score
    v = judge_order({0u, 20300u}, kJudgeByScore);
    CHECK(v.take && v.after.champion == 20300u, "no champion: take %d champion %u", v.take, v.after.champion);
    // a challenger without a score (no stamp): taken, as before there was a judge; the champion's score is then unknown too
    v = judge_order({17200u, 0u}, kJudgeByScore);
    CHECK(v.take && v.after.champion == 0u && v.after.challenger == 0u, "score 0: take %d champion %u", v.take, v.after.champion);
    v = judge_order({0u, 0u}, kJudgeByScore);
    CHECK(v.take && v.after.champion == 0u, "nothing measured: take %d", v.take);
    // the champion's score refreshed by the sort behind its segment: a champion gone stale (the scene changed) loses the next comparison
    JudgeScores s = {17200u, 0u};
    s.champion = 26000u;                                   // k_order_by_cost: the newest frame under the champion
    s.challenger = 21000u;
    v = judge_order(s, kJudgeByScore);
    CHECK(v.take && v.after.champion == 21000u, "stale champion: take %d champion %u", v.take, v.after.champion);
    // the forced verdicts, whatever the scores
    for (const JudgeScores f : {JudgeScores{18000u, 17000u}, JudgeScores{17000u, 18000u}, JudgeScores{0u, 5u}, JudgeScores{5u, 0u}, JudgeScores{0u, 0u}}) {
        const Verdict t = judge_order(f, kJudgeAlwaysTake), k = judge_order(f, kJudgeAlwaysKeep);
        CHECK(t.take && t.after.champion == f.challenger && t.after.challenger == f.challenger, "always take {%u, %u}", f.champion, f.challenger);
        CHECK(!k.take && k.after.champion == f.champion && k.after.challenger == f.challenger, "always keep {%u, %u}", f.champion, f.challenger);
    }
    // the score: ticks between the two readings; 0 = not measured (no stamp, a clock that did not advance); saturates
    CHECK(judge_score(1000u, 18200u) == 17200u, "score");
    CHECK(judge_score(0u, 18200u) == 0u && judge_score(500u, 500u) == 0u && judge_score(501u, 500u) == 0u, "score not measured");
    CHECK(judge_score(1u, 2u) == 1u, "score of one tick");
    CHECK(judge_score(1u, (1ull << 40)) == 0xFFFFFFFFu, "score saturates");
    static_assert(kJudgeStampLo % 2 == 0 && kJudgeStampHi == kJudgeStampLo + 1, "the stamp is one aligned 64-bit word");
    static_assert(kJudgeWords == 6 && kJudgeTaken > kJudgeChallenger && kJudgeRejected < kJudgeWords, "judge block");
    if (!g_failed) std::printf("rule ok\n");
}

const uint64_t kS[5] = {(320ull << 32) | 180, 1, (1ull << 32) | (5ull << 16), (64ull << 32) | (1ull << 16) | RTK_TRACE_GROUP4, 0};
const uint64_t kT[5] = {(64ull << 32) | 64, 1, (1ull << 32) | (5ull << 16), (64ull << 32) | (1ull << 16) | RTK_TRACE_GROUP4, 0};

struct Seen { std::vector<int> sorts, judges, behind; };

// frames [first, last] of shape `sig`: which of them start a new list, which are judged, which have the sort launched behind them
Seen run(OrderState &st, const uint64_t sig[5], const OrderState::Knobs &k, int first, int last) {
    Seen r;
    for (int f = first; f <= last; ++f) {
        const OrderState::Step s = st.step(sig, RTK_TRACE_GROUP4, false, false, k);
        if (s.resort) r.sorts.push_back(f);
        if (s.judge) r.judges.push_back(f);
        if (s.sort_behind) r.behind.push_back(f);
        CHECK(!s.judge || (s.resort && !s.sort_front && s.read_set != s.write_set), "frame %d: a judge needs a list sorted behind the frame before", f);
        CHECK(s.resort == (s.sort_front || s.judge), "frame %d: a new list is sorted in front or judged", f);
    }
    return r;
}

bool same(const std::vector<int> &a, std::initializer_list<int> b) { return a == std::vector<int>(b); }

void the_schedule() {
    {   // the cap at 64: 2, 18, 34, 66, 130, then every 64 frames; the judge at every sort but the shape's first; the sort behind the frame before
        OrderState st;
        const OrderState::Knobs k = {true, 16, 64};
        const Seen r = run(st, kS, k, 1, 400);
        CHECK(same(r.sorts, {2, 18, 34, 66, 130, 194, 258, 322, 386}), "cap 64: %zu sorts", r.sorts.size());
        CHECK(same(r.judges, {18, 34, 66, 130, 194, 258, 322, 386}), "cap 64: %zu judges", r.judges.size());
        CHECK(same(r.behind, {17, 33, 65, 129, 193, 257, 321, 385}), "cap 64: %zu sorts behind", r.behind.size());
        // forget(): the schedule starts over
        st.forget();
        const Seen a = run(st, kS, k, 1, 140);
        CHECK(same(a.sorts, {2, 18, 34, 66, 130}) && same(a.judges, {18, 34, 66, 130}), "cap 64 after forget: %zu sorts", a.sorts.size());
        // another shape, and back: each starts over
        const Seen b = run(st, kT, k, 1, 70);
        CHECK(same(b.sorts, {2, 18, 34, 66}) && same(b.judges, {18, 34, 66}), "cap 64, another shape: %zu sorts", b.sorts.size());
        const Seen c = run(st, kS, k, 1, 70);
        CHECK(same(c.sorts, {2, 18, 34, 66}) && same(c.judges, {18, 34, 66}), "cap 64, back: %zu sorts", c.sorts.size());
    }
    {   // the library's default, 128; a cap that is no power-of-two multiple; a cap not above resort_every
        OrderState st;
        CHECK(same(run(st, kS, {true, 16, 128}, 1, 600).sorts, {2, 18, 34, 66, 130, 258, 386, 514}), "cap 128");
        OrderState s48;
        CHECK(same(run(s48, kS, {true, 16, 48}, 1, 200).sorts, {2, 18, 34, 66, 114, 162}), "cap 48");
        OrderState s16;
        CHECK(same(run(s16, kS, {true, 16, 16}, 1, 70).sorts, {2, 18, 34, 50, 66}), "cap 16");
        OrderState s8;
        CHECK(same(run(s8, kS, {true, 16, 8}, 1, 70).sorts, {2, 18, 34, 50, 66}), "cap below resort_every");
    }
    {   // the cap at 0, and two-field knobs as the existing callers write them: the sequences of frame_plan_check.cpp
        for (int variant = 0; variant < 2; ++variant) {
            const OrderState::Knobs k16 = variant ? OrderState::Knobs{true, 16, 0} : OrderState::Knobs{true, 16};
            const OrderState::Knobs k1 = variant ? OrderState::Knobs{true, 1, 0} : OrderState::Knobs{true, 1};
            OrderState st;
            const Seen r = run(st, kS, k16, 1, 40);
            CHECK(same(r.sorts, {2, 18, 34}) && same(r.judges, {18, 34}) && same(r.behind, {17, 33}) && st.age == 7, "cap 0, every 16 (variant %d)", variant);
            const Seen more = run(st, kS, k16, 41, 100);
            CHECK(same(more.sorts, {50, 66, 82, 98}), "cap 0, every 16, on to frame 100 (variant %d)", variant);
            OrderState s1;
            const Seen e = run(s1, kS, k1, 1, 40);
            CHECK(e.sorts.size() == 39 && e.sorts.front() == 2 && e.sorts.back() == 40, "cap 0, every 1: %zu sorts (variant %d)", e.sorts.size(), variant);
            CHECK(e.judges.size() == 38 && e.judges.front() == 3, "cap 0, every 1: %zu judges (variant %d)", e.judges.size(), variant);
        }
    }
    {   // restart_schedule() (the lights moved at an equal count): the intervals start over at 16 and the list's age stays, so a list
        // already older than that is sorted behind the very next frame; the order, the set and the known count stay
        const OrderState::Knobs k = {true, 16, 128};
        OrderState st;
        uint32_t word = 700u;
        for (int f = 1; f <= 100; ++f) {                    // sorts at 2, 18, 34, 66; the next would be at 130
            st.step(kS, RTK_TRACE_GROUP4, false, false, k);
            st.workgroups(st.awaits_count(), &word);
        }
        const int set_before = st.set;
        st.restart_schedule(16);
        CHECK(st.valid && st.order_valid && st.set == set_before && !st.awaits_count() && st.workgroups(false, &word) == 700u, "restart keeps the order and its count");
        const Seen r = run(st, kS, k, 101, 260);
        CHECK(same(r.sorts, {102, 118, 134, 166, 230}) && same(r.judges, {102, 118, 134, 166, 230}) && same(r.behind, {101, 117, 133, 165, 229}),
              "restart at frame 100: %zu sorts, first %d", r.sorts.size(), r.sorts.empty() ? 0 : r.sorts[0]);
        // a list younger than 16 frames keeps its age: frame 40 is the seventh frame of the list of frame 34
        OrderState young;
        run(young, kS, k, 1, 40);
        young.restart_schedule(16);
        CHECK(same(run(young, kS, k, 41, 120).sorts, {50, 66, 82, 114}), "restart of a young list");
        // right behind a frame that has the sort behind it: the next frame takes that list as planned, and the schedule starts from there
        OrderState s2;
        run(s2, kS, k, 1, 65);                              // frame 65 has the sort behind it
        CHECK(s2.presorted, "frame 65 has the sort behind it");
        s2.restart_schedule(16);
        const Seen q = run(s2, kS, k, 66, 140);
        CHECK(same(q.sorts, {66, 82, 98, 130}) && same(q.judges, {66, 82, 98, 130}), "restart behind a sort: %zu sorts", q.sorts.size());
        // with the cap at 0 it changes nothing: the interval is 16 anyway and no list grows older
        OrderState s3;
        const OrderState::Knobs k0 = {true, 16};
        run(s3, kS, k0, 1, 40);
        s3.restart_schedule(16);
        CHECK(same(run(s3, kS, k0, 41, 90).sorts, {50, 66, 82}), "restart, cap 0");
        // on a state without an order it changes nothing
        OrderState fresh;
        fresh.restart_schedule(16);
        const Seen n = run(fresh, kS, k, 1, 20);
        CHECK(same(n.sorts, {2, 18}), "restart of a fresh state");
        // It never puts a sort off, however often it comes.  An animated light: the call before every frame, and before every 10th,
        // from frame 41 on for 400 frames, with the cap and without: a sort at least every 16 frames, as before there was a cap.
        for (const OrderState::Knobs &kk : {k, k0})
            for (int period : {1, 10}) {
                OrderState an;
                std::vector<int> sorts = run(an, kS, kk, 1, 40).sorts;
                for (int f = 41; f <= 440; ++f) {
                    if (f % period == 0) an.restart_schedule(kk.resort_every);
                    const Seen one = run(an, kS, kk, f, f);
                    sorts.insert(sorts.end(), one.sorts.begin(), one.sorts.end());
                    CHECK(one.sorts.size() == one.judges.size(), "animated, frame %d: every new list is judged", f);
                }
                int worst = 0;
                for (size_t i = 1; i < sorts.size(); ++i) worst = sorts[i] - sorts[i - 1] > worst ? sorts[i] - sorts[i - 1] : worst;
                // (With the cap, the list of frame 34 is due at 66.  The call before frame 50 finds it 16 frames old: too late for a
                // sort behind frame 49, so it goes behind frame 50 -- one gap of 17, the only way a gap can exceed 16.)
                const bool late = kk.resort_max > kk.resort_every && period == 10;
                CHECK(sorts.size() == 28 && sorts[3] == (late ? 51 : 50) && sorts.back() == (late ? 435 : 434) && worst == (late ? 17 : 16),
                      "animated, cap %u, every %d frames: %zu sorts, fourth %d, last %d, longest gap %d", kk.resort_max, period, sorts.size(),
                      sorts[3], sorts.back(), worst);
                int over = 0;
                for (size_t i = 1; i < sorts.size(); ++i) over += sorts[i] - sorts[i - 1] > 16;
                CHECK(over == (late ? 1 : 0), "animated, cap %u, every %d frames: %d gaps above 16", kk.resort_max, period, over);
            }
        // (one call in mid-stretch and no more: the stretching resumes, 16, 16, 32, ... as pinned above)
    }
    if (!g_failed) std::printf("schedule ok\n");
}

void the_rearmed_count() {
    const OrderState::Knobs k = {true, 16, 64};
    OrderState st;
    uint32_t word = 0;
    // frames 1-17: the sort of frame 2 read back 700 workgroups, seen at frame 3
    for (int f = 1; f <= 17; ++f) {
        st.step(kS, RTK_TRACE_GROUP4, false, false, k);
        if (f == 2) word = 700u;
        const bool asked = st.awaits_count();
        const unsigned n = st.workgroups(asked && f >= 3, &word);
        CHECK(n == (f >= 3 ? 700u : 0u), "frame %d: %u workgroups", f, n);
    }
    // frame 18 starts the challenger's list (its length, 650, was read back behind frame 17 and is seen) and is judged
    word = 650u;
    const OrderState::Step s18 = st.step(kS, RTK_TRACE_GROUP4, false, false, k);
    CHECK(s18.judge && st.awaits_count(), "frame 18: judge %d", s18.judge);
    CHECK(st.workgroups(true, &word) == 650u && !st.awaits_count(), "frame 18 runs the challenger's 650 workgroups");
    st.rearm_count();                                      // the judge is enqueued: the champion's 700 may be back
    CHECK(st.awaits_count() && st.nwgs_pending && !st.nwgs_known, "re-armed");
    // frames 19-21: the read-back behind the judge is not seen yet: every block is launched, whatever the pinned word says
    for (int f = 19; f <= 21; ++f) {
        const OrderState::Step s = st.step(kS, RTK_TRACE_GROUP4, false, false, k);
        CHECK(s.use_order && !s.resort && !s.judge && st.awaits_count(), "frame %d", f);
        CHECK(st.workgroups(false, &word) == 0u, "frame %d: 0 until the new read-back is seen", f);
    }
    // frame 22: seen, and the word is the champion's again
    word = 700u;
    st.step(kS, RTK_TRACE_GROUP4, false, false, k);
    CHECK(st.awaits_count() && st.workgroups(true, &word) == 700u && !st.awaits_count(), "frame 22: the new word");
    st.step(kS, RTK_TRACE_GROUP4, false, false, k);
    CHECK(!st.awaits_count() && st.workgroups(false, &word) == 700u, "frame 23: known, no query");
    // without an order there is nothing to re-arm
    OrderState fresh;
    fresh.rearm_count();
    CHECK(!fresh.awaits_count() && fresh.workgroups(true, &word) == 0u, "no order: nothing pending");
    st.forget();
    st.rearm_count();
    CHECK(!st.awaits_count() && st.workgroups(true, &word) == 0u, "forgotten: nothing pending");
    if (!g_failed) std::printf("count ok\n");
}

}  // namespace

int main() {
    the_rule();
    the_schedule();
    the_rearmed_count();
    if (g_failed) { std::printf("FAILED: %d checks\n", g_failed); return 1; }
    std::printf("all ok\n");
    return 0;
}
