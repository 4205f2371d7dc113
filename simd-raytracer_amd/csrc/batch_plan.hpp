// The host's share of the ray repacking (api_batch.hip, repack.hip): whether a batch is probed, forced into a sort or walked as
// it comes, how many of its waves the bounds passes look at, and what the probe's verdict words turn into -- sort or not, the
// strategy of the sorted walk, the key bits left unsorted.  None of it changes a hit, so no parity test sees it:
// tests/cpp/batch_plan_check.cpp pins it.  Plain structs and integers, no HIP, no accel: the launch path asks these, then
// issues what they say.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rtk.h"

namespace rtk {

constexpr size_t kRepackMinRays = size_t(1) << 18;      // RTK_TRACE_AUTO probes batches of at least this many rays
constexpr size_t kRepackRayLimit = size_t(1) << 32;     // the permutation holds 32-bit ray indices: fewer rays than this
constexpr size_t kRepackSampleWaves = 4096;             // a bounds pass looks at about this many waves of 64 rays
constexpr uint32_t kProbeMinStride = 16;                // ... the probe at every 16th at the most

struct BatchKnobs {
    bool repack;                       // RTK_REPACK
    bool repack_full_bounds;           // RTK_REPACK_FULL_BOUNDS
    int repack_skip_bits;              // RTK_REPACK_SKIP_BITS (0..14)
    int repack_skip_bits2;             // RTK_REPACK_SKIP_BITS2 (0..22)
    int repack_trace;                  // RTK_REPACK_TRACE (-1: by the probe)
};

inline size_t batch_waves(size_t n) { return (n + 63) / 64; }

// every how-many-th wave the probe looks at: ~4,096 waves, never fewer than every 16th
inline uint32_t probe_stride(size_t n) {
    const size_t s = (batch_waves(n) + kRepackSampleWaves - 1) / kRepackSampleWaves;
    return uint32_t(s > kProbeMinStride ? s : kProbeMinStride);
}
// ... and the bounds pass of a sort that no probe preceded (0 waves: 0, which launch_ray_bounds takes as 1)
inline uint32_t sample_stride(size_t n, bool full_bounds) {
    return full_bounds ? 1u : uint32_t((batch_waves(n) + kRepackSampleWaves - 1) / kRepackSampleWaves);
}

struct BatchPlan {
    int mode;                          // the strategy of a walk in the caller's order (RTK_TRACE_REPACK: RTK_TRACE_AUTO)
    bool big, forced, sortable, probe;
    bool workspace;                    // keys, permutation and bounds are needed: the batch is probed or sorted unasked
    uint32_t probe_stride;             // probe: launch_ray_bounds' wave stride
    uint32_t bounds_stride;            // no probe: the same of the sort's own bounds pass
    bool keys_ahead;                   // probe: k_ray_keys is launched behind the probe, before its verdict is known
};

inline BatchPlan plan_batch(size_t n, int mode, bool stats, const BatchKnobs &k) {
    BatchPlan p;
    p.big = n >= kRepackMinRays && n < kRepackRayLimit;
    p.forced = mode == RTK_TRACE_REPACK;
    p.mode = p.forced ? RTK_TRACE_AUTO : mode;
    p.sortable = !stats && n >= 2 && n < kRepackRayLimit;
    p.probe = !stats && !p.forced && p.mode == RTK_TRACE_AUTO && k.repack && p.big;
    p.workspace = (p.forced && p.sortable) || p.probe;
    p.probe_stride = probe_stride(n);
    p.bounds_stride = sample_stride(n, k.repack_full_bounds);
    p.keys_ahead = p.probe && !k.repack_full_bounds;
    return p;
}

struct SortPlan {
    bool sort;                         // the batch is walked through a permutation
    bool rebound;                      // a bounds pass of its own before the keys (no probe, or RTK_REPACK_FULL_BOUNDS)
    uint32_t bounds_stride;
    unsigned sort_from_bit;            // key bits [sort_from_bit, 30) are sorted
    int sorted_mode;                   // what the probe makes of the sorted walk
    int mode;                          // the strategy launched
};

// sort_word, dims_word: words 16 and 17 of the probe's result (repack.hpp); read only where the plan probes
inline SortPlan plan_sort(const BatchPlan &p, uint32_t sort_word, uint32_t dims_word, const BatchKnobs &k) {
    SortPlan s;
    s.sort = p.workspace && (p.probe ? sort_word != 0u : true);
    s.sort_from_bit = 0u;
    s.sorted_mode = RTK_TRACE_AUTO;                                          // any order: wave-cooperative with the per-lane fallback
    if (s.sort && p.probe && dims_word <= 3u) {
        s.sorted_mode = RTK_TRACE_WAVE;                                      // ten or fifteen bits per dimension: the sort makes tight waves
        // ... also when the lowest ones stay unsorted: one or two radix passes less (two dimensions: 8 of the 15 bits each)
        s.sort_from_bit = dims_word <= 2u ? unsigned(k.repack_skip_bits2) : unsigned(k.repack_skip_bits);
    }
    s.rebound = s.sort && (!p.probe || k.repack_full_bounds);
    s.bounds_stride = p.probe ? 1u : p.bounds_stride;
    s.mode = s.sort ? (k.repack_trace >= 0 ? k.repack_trace : s.sorted_mode) : p.mode;
    return s;
}

}  // namespace rtk
