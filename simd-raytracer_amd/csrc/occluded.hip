// HIP kernel for gfx950: is_occluded(accel, ray, max_t) (render/render.hpp:110-131) for a batch.
// One query per lane, 256-thread workgroups (4 wave64), kd-tree nodes staged in LDS as k_intersect does.
#include <hip/hip_runtime.h>

#include "occluded.hpp"
#include "shade.hip.hpp"

namespace rtk {
namespace dev {

constexpr float kExitBelowMiss = 0x1.fffffcp+127f;    // the largest float below kFltMax, the t of a lane that has hit nothing

// The reference's loop, per lane, around ONE wave-wide closest-hit query per round (the shape of k_shadow's inner loop,
// stream.hip): a lane whose closest hit lies on a transmissive surface steps through it and asks again, the others have their
// answer and idle until the wave's last lane has one.  The reference's loop has no bound; this one gives up on a lane after
// RTK_OCCLUDED_MAX_STEPS queries and says so (RTK_OCC_STEP_LIMIT), so the kernel ends for every input.
template <int MODE, bool LDS_NODES>
__global__ __launch_bounds__(256) void k_occluded(OccludedArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevNode *lds_nodes = reinterpret_cast<DevNode *>(smem);
    if (LDS_NODES) stage_nodes(A.tree.nodes, A.tree.n_nodes, lds_nodes);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < A.n;
    Ray r;
    float max_t = 0.0f;
    if (active) {
        const float *p = reinterpret_cast<const float *>(A.rays + i);
        r = make_ray(mk(p[0], p[1], p[2]), mk(p[3], p[4], p[5]));
        max_t = A.max_t[i];
    } else {
        r = make_ray(mk(0.f, 0.f, 0.f), mk(1.f, 1.f, 1.f));
    }
    Stats st = {0, 0, 0, 0, 0, 0};
    __shared__ __attribute__((aligned(16))) float wave_bundles[4][kMaxBundles * kBundleFloats];
    SliceCtx sx = {nullptr, 0u, 0u, true, 0u, wave_bundles[(threadIdx.x >> 6) & 3u]};
    bool pending = active & (0.0f < max_t);                                  // the loop guard, render.hpp:114 (false for NaN)
    uint32_t answer = RTK_OCC_CLEAR;
    uint32_t queries = 0u;                                                   // closest-hit queries of this lane, <= RTK_OCCLUDED_MAX_STEPS
    while (wave_any(pending)) {
        // no transmissive material in the scene: the lane may stop at the first hit nearer than max_t (trace(), `exit_t`);
        // with them the closest hit is needed to know what was crossed
        // (a lane without a hit carries t = FLT_MAX: the exit is held below it, or max_t = inf or FLT_MAX would end the walk
        // before it began and answer "clear" whatever lay ahead)
        const float exit_t = A.has_refractive ? -1.0f : (max_t > kExitBelowMiss ? kExitBelowMiss : max_t);
        const Cand c = trace<MODE, false, LDS_NODES>(A.tree, lds_nodes, r, false, pending, st, sx, kAutoMinLanes, exit_t);
        if (pending) {
            queries += 1u;
            const OccStep os = occlusion_step(A.tree, A.materials, A.shadow_bias, A.has_refractive, c, r.o, r.d, max_t);
            r.o = os.o; max_t = os.max_t;
            answer = os.answer == OCC_OCCLUDED ? RTK_OCC_OCCLUDED : RTK_OCC_CLEAR;
            bool again = os.answer == OCC_AGAIN;
            if (again & (queries == (uint32_t)RTK_OCCLUDED_MAX_STEPS)) { answer = RTK_OCC_STEP_LIMIT; again = false; }
            pending = again;
        }
    }
    if (active) A.out[i] = (uint8_t)answer;
    if (A.n_intersect != nullptr) {
        const uint32_t total = wave_sum(queries);                            // <= 64 * RTK_OCCLUDED_MAX_STEPS
        if ((threadIdx.x & 63u) == 0u && total != 0u) atomicAdd(A.n_intersect, (unsigned long long)total);
    }
}

}  // namespace dev

namespace {

template <int MODE>
hipError_t launch_occluded_m(const dev::OccludedArgs &A, bool lds, size_t lds_bytes, hipStream_t s) {
    const unsigned blocks = (unsigned)((A.n + 255) / 256);
    if (blocks == 0) return hipSuccess;
    // only the per-lane walk reads the node array from LDS (launch_intersect_m)
    constexpr bool kNeedsNodes = (MODE == RTK_TRACE_LANE || MODE == RTK_TRACE_AUTO);
    if constexpr (kNeedsNodes) {
        if (lds) { hipLaunchKernelGGL((dev::k_occluded<MODE, true>), dim3(blocks), dim3(256), lds_bytes, s, A); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((dev::k_occluded<MODE, false>), dim3(blocks), dim3(256), 0, s, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_occluded(const dev::OccludedArgs &A, int mode, hipStream_t s) {
    const size_t lds_bytes = (size_t)A.tree.n_nodes * sizeof(DevNode);
    const bool lds = lds_bytes <= kMaxNodeLdsBytes;
    switch (mode) {
        case RTK_TRACE_LANE: return launch_occluded_m<RTK_TRACE_LANE>(A, lds, lds_bytes, s);
        case RTK_TRACE_WAVE: return launch_occluded_m<RTK_TRACE_WAVE>(A, lds, lds_bytes, s);
        default: return launch_occluded_m<RTK_TRACE_AUTO>(A, lds, lds_bytes, s);
    }
}

}  // namespace rtk
