// rtk_temporal_accumulate: the argument block and the launcher of the kernel of temporal.hip, shared with api_temporal.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "temporal_plan.hpp"

namespace rtk {
namespace dev {

struct TemporalArgs {
    // the new frame; noise and mesh may be null
    const float *rgb, *noise, *position, *normal, *depth;
    const uint32_t *mesh;
    // the history: all null without one (p_rgb decides); p_noise and p_mesh null as the new frame's are
    const float *p_rgb, *p_noise, *p_length, *p_position, *p_normal, *p_depth;
    const uint32_t *p_mesh;
    float *o_rgb, *o_noise, *o_length;       // o_noise null as noise is
    DnTiling tiling;                         // of one image
    tp::Consts k;
};

}  // namespace dev

hipError_t launch_temporal_accumulate(const dev::TemporalArgs &A, hipStream_t s);

}  // namespace rtk
