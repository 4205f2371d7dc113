// Batched occlusion query (rtk_accel_occluded*): argument block and launcher shared by occluded.hip and api_batch.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace rtk {
namespace dev {

struct OccludedArgs {
    TreeView tree;
    const DevMaterial *materials;
    const rtk_ray *rays;
    const float *max_t;               // [n] is_occluded's max_t, in units of the ray parameter
    uint8_t *out;                     // [n] RTK_OCC_*
    size_t n;
    float shadow_bias;
    int has_refractive;               // 0: no transmissive material, a query may stop at the first answering hit (trace(), `exit_t`)
    unsigned long long *n_intersect;  // non-null: every wave adds the closest-hit queries its lanes made
};

}  // namespace dev

hipError_t launch_occluded(const dev::OccludedArgs &A, int mode, hipStream_t s);

}  // namespace rtk
