// The layout of a counter block (rtk_accel::d_counters, a radiance lane's block), in 64-bit words: the kernels that count into it
// and the host code that zeroes, folds and reads it share these names.  No HIP, no accel: usable from host and device code.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rtk.h"

namespace rtk {

// ---- [0, 8): one word per field of rtk_counters, in its order
constexpr int kWordRays = 0;                       // batches and the streaming kernels count here; k_render counts into the shards
constexpr int kWordPrimary = 1;                    // never counted on the device: the host knows a call's camera rays
constexpr int kWordHits = 2, kWordNodes = 3, kWordBoxpass = 4, kWordLeaves = 5, kWordTris = 6, kWordPackets16 = 7;   // per-ray statistics
// ---- [8, 8 + shards): the ray count again, spread out (one atomic per pixel block: a single word takes ~88 atomics per microsecond)
constexpr int kRayShardWord = 8;
constexpr int kRayCounterShards = 64;
// ---- then as many words for the longest pixel block of the frame in s_memrealtime ticks (10 ns), sharded the same way
constexpr int kCriticalWord = kRayShardWord + kRayCounterShards;
constexpr int kCounterWords = kCriticalWord + kRayCounterShards;          // what a fold, a lane's block and a call's totals hold
// ---- the tail of an accel's block, behind the counters and zeroed with them by a frame
constexpr int kPriorScratchWord = kCounterWords;                          // k_block_prior's six 32-bit cursors: three words
constexpr int kOccludedCountWord = kCounterWords + 3;                     // closest-hit queries of rtk_accel_occluded's host variant
constexpr int kCounterAllocWords = kCounterWords + 4;

// ---- a radiance call's block: one counter block per lane of the streaming pipeline, then the call's {rays, chunks redone}
constexpr int kRadianceRays = 0, kRadianceRedone = 1, kRadianceTotalWords = 2;
constexpr size_t radiance_lane_word(int lane) { return size_t(lane) * kCounterWords; }
constexpr size_t radiance_total_word(int lanes) { return size_t(lanes) * kCounterWords; }

// A block read back: its first kRayShardWord words as rtk_counters.  `stats`: the launch collected per-ray statistics (the fields
// are zero otherwise).  `primary` is left zero, and a frame's reader adds the shards to `rays`.
inline void counters_from_block(const unsigned long long *h, bool stats, rtk_counters *c) {
    *c = rtk_counters{};
    c->rays = h[kWordRays];
    if (!stats) return;
    c->hits = h[kWordHits]; c->nodes = h[kWordNodes]; c->boxpass = h[kWordBoxpass];
    c->leaves = h[kWordLeaves]; c->tris = h[kWordTris]; c->packets16 = h[kWordPackets16];
}

}  // namespace rtk
