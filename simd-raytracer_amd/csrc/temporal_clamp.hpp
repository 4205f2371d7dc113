// rtk_temporal_accumulate_clamped: the argument block and the launcher of the kernel of temporal_clamp.hip, shared with
// api_temporal.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "temporal.hpp"
#include "temporal_clamp_plan.hpp"

namespace rtk {
namespace dev {

struct TemporalClampArgs {
    TemporalArgs t;                          // as the plain call's; o_rgb is not rgb and o_noise is not noise
    int32_t radius;                          // 1..3
    float gamma, history_keep;
};

}  // namespace dev

hipError_t launch_temporal_accumulate_clamped(const dev::TemporalClampArgs &A, hipStream_t s);

}  // namespace rtk
