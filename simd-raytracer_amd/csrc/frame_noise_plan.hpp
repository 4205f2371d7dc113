// Host plan of rtk_render_frame_noise (api_frame_noise.hip): what the call refuses and in which order, what its workspace costs,
// what a batch of samples does with the running sums, and the adaptive call that redoes a frame whose queues overflowed.  Plain
// integers, no HIP, no accel: tests/cpp/frame_noise_plan_check.cpp runs it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rtk.h"

namespace rtk {

// Pixels of a frame at most: the running sums are the adaptive render's (16 B per pixel), which a uint32_t pixel index addresses,
// and the overflow redo is an adaptive render, which takes no more (adaptive_plan.hpp kAdaptiveMaxPixels).
constexpr uint64_t kFrameNoiseMaxPixels = uint64_t(1) << 31;

// What the call refuses once rtk_render_frame's own checks of *p have passed (frame_geom), in the order rtk.h gives; nullptr = the
// call goes on to the device.  width, height: the frame's, as frame_geom resolved them.
inline const char *frame_noise_refusal(const rtk_render_params &p, uint32_t width, uint32_t height) {
    if (p.trace_mode != RTK_TRACE_AUTO && p.trace_mode != RTK_TRACE_STREAM)
        return "trace_mode of a frame with its noise plane must be RTK_TRACE_AUTO or RTK_TRACE_STREAM";
    if (p.spp < 2) return "a noise plane needs spp >= 2";
    if (p.sample_begin != 0 || p.sample_count != 0)
        return "a frame with its noise plane is not progressive: sample_begin and sample_count must be 0";
    if (p.collect_stats != 0) return "a frame with its noise plane collects no per-ray statistics";
    if (p.world_size > 1) return "a frame with its noise plane is not sharded";
    if (uint64_t(width) * height > kFrameNoiseMaxPixels) return "too many pixels for a frame with its noise plane";
    return nullptr;
}

// two planes of double
inline uint64_t frame_noise_workspace_bytes(uint64_t pixels) { return pixels * 2u * sizeof(double); }

// What the batch of samples [sample, sample + n_batch) of a frame of `spp` does with a pixel's running sums: it starts them at +0
// or loads them, and stores them back or writes the noise instead.
struct FrameNoiseBatch { bool starts, ends; };
inline FrameNoiseBatch frame_noise_batch(int32_t sample, uint32_t n_batch, int32_t spp) {
    return {sample == 0, int64_t(sample) + int64_t(n_batch) == int64_t(spp)};
}

// The call again as an adaptive render that judges nothing before the ceiling: every pixel takes all spp samples, the rgb is the
// frame's and the noise is the statistic at n = spp (rtk.h).
inline rtk_adaptive_params frame_noise_redo(const rtk_render_params &p) {
    rtk_adaptive_params ap;
    ap.min_samples = p.spp; ap.step = 1; ap.threshold = 0.0f; ap.floor = 1.0f;
    return ap;
}

}  // namespace rtk
