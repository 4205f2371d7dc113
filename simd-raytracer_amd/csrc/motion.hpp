// rtk_render_motion: the argument block and the launcher of the kernel of motion.hip, shared with api_motion.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "motion_plan.hpp"

namespace rtk {
namespace dev {

struct MotionArgs {
    const uint32_t *tri;                     // [h][w]
    const float *bary;                       // [h][w][2]
    const float *verts;                      // [n_verts][3]: the previous pose
    const uint32_t *index;                   // [n_tris][3]: global vertex ids of the accel's current topology
    uint32_t n_tris, n_verts;
    float *prev_position, *motion;           // either may be null, not both
    DnTiling tiling;                         // of one image
    tp::Consts k;                            // the previous view; read only with a motion plane
};

}  // namespace dev

hipError_t launch_motion(const dev::MotionArgs &A, hipStream_t s);

}  // namespace rtk
