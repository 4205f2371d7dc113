// The arithmetic of rtk_render_motion (rtk.h), one copy of each step: the point of a triangle of the previous pose at a pixel's
// barycentrics, and the screen-space motion of that point through the previous view (temporal_math.hpp place, the projection of
// rtk_temporal_accumulate up to its range test).  Plain inline functions for host and device: the kernel (motion.hip) and the host
// check program (tests/cpp/motion_math_check.cpp) both include it; tests/motion_model.py is the same arithmetic in numpy.
// Everything is float, in the order rtk.h writes it, and relies on -ffp-contract=off.  No HIP, no plan.
#pragma once

#include <cstdint>

#include "temporal_math.hpp"

namespace rtk {
namespace mv {

constexpr uint32_t kMissBits = 0x7FC00000u;                    // both words of a pixel's motion when there is none to report

// step 1 of rtk.h: the only ids anything is dereferenced with
RTK_TP_FN bool is_hit(uint32_t id, uint32_t n_triangles) { return id < n_triangles; }

// step 2: u weighs vertex 1 (B), v vertex 2 (C), w = (1 - u) - v vertex 0 (A); non-finite u, v propagate
RTK_TP_FN void surface_point(const float A[3], const float B[3], const float C[3], float u, float v, float P[3]) {
    const float w = (1.0f - u) - v;
    for (int i = 0; i < 3; ++i) P[i] = ((w * A[i]) + (u * B[i])) + (v * C[i]);
}

// step 3: previous place minus present place, in pixels; false = P is not in front of the previous camera (the miss bits are written)
RTK_TP_FN bool motion_of(const tp::Consts &k, const float P[3], uint32_t x, uint32_t y, float &mx, float &my) {
    float fx, fy;
    if (!tp::place(k, P, fx, fy)) return false;
    mx = fx - (float)x; my = fy - (float)y;
    return true;
}

}  // namespace mv
}  // namespace rtk
