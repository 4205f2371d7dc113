// rtk_accel_set_materials on a resident accel: which triangles are opaque, and the opaque-only occlusion tree of a
// RTK_TRAVERSAL_FAST accel (rtk.h; api.hip ensure_device makes it on the host, build.hip k_build_gather during an update), re-made
// from the ACTIVE tree when the set of refractive materials changes.  After an update the per-triangle and per-reference arrays
// exist on the device only, so this is device work; the host makes the few hundred nodes (api_update.hip, remake_occluders).
//
//   k_occl_flags    one thread per triangle: the flags later updates read (BuildArgs::opaque)
//   k_occl_count    one wave per leaf: how many of its references are opaque
//   k_occl_gather   one wave per leaf: those references' DevTri and id, in the leaf's order (ballot + mbcnt, as k_build_gather)
//
// A triangle is opaque unless its material is refractive; a material index out of range counts as opaque, as on the host
// (api.hip ensure_device, api_update.hip ensure_update_static).  None of this is on a frame's path.
#include <hip/hip_runtime.h>

#include "build.hpp"

namespace rtk {
namespace dev {
namespace {

__device__ __forceinline__ uint32_t lanes_below(const unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ bool is_opaque(const OcclArgs &O, const uint32_t tri) {
    if (tri >= O.n_tris) return true;
    const uint32_t m = O.shade[tri].material;
    return !(m < O.n_materials && O.materials[m].kind == RTK_MAT_REFRACTIVE);
}

__global__ __launch_bounds__(256) void k_occl_flags(const OcclArgs O) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < O.n_tris) O.opaque[i] = is_opaque(O, i) ? uint8_t(1) : uint8_t(0);
}

// Leaves hold up to several hundred references: passes of 64 with a running sum.
__global__ __launch_bounds__(64) void k_occl_count(const OcclArgs O) {
    const OcclLeaf L = O.leaves[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint32_t kept = 0u;
    for (uint32_t k0 = 0u; k0 < L.count; k0 += 64u) {
        const uint32_t r = L.first + k0 + lane;
        const bool keep = k0 + lane < L.count && r < O.n_refs && is_opaque(O, O.tri_ids[r]);
        kept += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(keep)));
    }
    if (lane == 0u) O.counts[blockIdx.x] = kept;
}

__global__ __launch_bounds__(64) void k_occl_gather(const OcclArgs O) {
    const OcclLeaf L = O.leaves[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint32_t kept = 0u;
    for (uint32_t k0 = 0u; k0 < L.count; k0 += 64u) {
        const uint32_t r = L.first + k0 + lane;
        uint32_t id = 0u;
        bool keep = k0 + lane < L.count && r < O.n_refs;
        if (keep) { id = O.tri_ids[r]; keep = is_opaque(O, id); }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        if (keep) {
            const uint32_t d = L.dst + kept + lanes_below(m);
            if (d < O.cap) { O.occl_tris[d] = O.tris[r]; O.occl_ids[d] = id; }
        }
        kept += uint32_t(__popcll(m));
    }
}

}  // namespace
}  // namespace dev

hipError_t launch_occl_flags(const dev::OcclArgs &O, hipStream_t s) {
    if (O.n_tris == 0u) return hipSuccess;
    hipLaunchKernelGGL(dev::k_occl_flags, dim3((O.n_tris + 255u) / 256u), dim3(256), 0, s, O);
    return hipGetLastError();
}

hipError_t launch_occl_count(const dev::OcclArgs &O, hipStream_t s) {
    if (O.n_leaves == 0u) return hipSuccess;
    hipLaunchKernelGGL(dev::k_occl_count, dim3(O.n_leaves), dim3(64), 0, s, O);
    return hipGetLastError();
}

hipError_t launch_occl_gather(const dev::OcclArgs &O, hipStream_t s) {
    if (O.n_leaves == 0u) return hipSuccess;
    hipLaunchKernelGGL(dev::k_occl_gather, dim3(O.n_leaves), dim3(64), 0, s, O);
    return hipGetLastError();
}

}  // namespace rtk
