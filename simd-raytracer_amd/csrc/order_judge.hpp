// Keep or take: the rule by which a launch order that a re-sort has just made (the challenger) replaces the order the frames ran
// before it (the champion), or does not.  Frames of one list run in one of two regimes, 13-19 % apart, and a
// list keeps its regime: so every list is scored by the device time of a frame that ran under it -- 100 MHz ticks from the start of
// that frame's k_render to the start of the kernel launched behind it -- and a challenger that scored slower than the champion costs
// one frame instead of a whole segment.  A scored frame starts behind a one-thread k_stamp that stores the clock; k_order_by_cost
// stores the champion's score (behind the last frame of its segment, so the score is never older than one segment), k_judge_order
// (kernels.hip) scores the challenger behind its first frame and asks this.
// Plain integers, no HIP: the kernels and tests/cpp/order_judge_check.cpp both compile it.  No pixel depends on any of it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTK_JUDGE_FN __host__ __device__ inline
#else
#define RTK_JUDGE_FN inline
#endif

namespace rtk {

// rtk_knobs::judge_force (RTK_COST_JUDGE_FORCE): the verdict whatever the scores say, for the tests
enum : int { kJudgeByScore = 0, kJudgeAlwaysTake = 1, kJudgeAlwaysKeep = 2 };

// The words of a table's judge block on the device (rtk_cost_feedback::judge), 32-bit each.  The first two are the 64-bit stamp that
// k_stamp stores in front of a frame that is scored.
enum : uint32_t {
    kJudgeStampLo = 0, kJudgeStampHi = 1,
    kJudgeChampion = 2,                // ticks of the champion's newest scored frame; 0: there is no champion (yet)
    kJudgeChallenger = 3,              // ticks of the newest challenger's first frame; 0: none judged yet
    kJudgeTaken = 4, kJudgeRejected = 5,   // verdicts since the table was made (rtk_debug_order_judge; sorts and judges are counted by the host)
    kJudgeWords = 6
};

// a frame's score from the two clock readings; 0 means "not measured", so a measured frame scores at least 1
RTK_JUDGE_FN uint32_t judge_score(uint64_t frame_start, uint64_t behind_start) {
    if (frame_start == 0 || behind_start <= frame_start) return 0u;
    const uint64_t d = behind_start - frame_start;
    return d > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(d);
}

struct JudgeScores { uint32_t champion, challenger; };
struct Verdict {
    bool take;                         // the challenger's lists stay in the set the frames read; else the champion's are copied back over them
    JudgeScores after;                 // what the judge block holds behind the judge
};

// No margin: the regimes are far apart and the frames of one list spread by 2-3 %; a tie decided by noise swaps two equally fast lists.
// A challenger is taken when it is not slower than the champion, when there is no champion to keep, and when either frame could not be
// scored (a score of 0): without a measurement the newest costs win, as they did before there was a judge.  A taken challenger is the
// champion from then on and carries its score with it; a rejected one leaves the champion's score alone -- that is refreshed by the
// next sort, so a champion gone stale after the scene changed loses the comparison after it.
RTK_JUDGE_FN Verdict judge_order(JudgeScores s, int force) {
    bool take = s.champion == 0u || s.challenger == 0u || s.challenger <= s.champion;
    if (force == kJudgeAlwaysTake) take = true;
    if (force == kJudgeAlwaysKeep) take = false;
    return {take, {take ? s.challenger : s.champion, s.challenger}};
}

}  // namespace rtk
