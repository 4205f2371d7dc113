// rtk_render_gbuffer: what the camera rays hit, as planes.  One wave per 8x8 pixel block of one view, four waves to a workgroup;
// the camera ray, the root test, one wave-cooperative closest-hit query, the hit's reconstruction and the stores of the planes
// that are wanted.  Every device function is the one the frames and the batched intersect use (common.hip.hpp, trace.hip.hpp):
// the planes hold the bits of rtk_camera_rays + rtk_accel_intersect(cull = 1).
#include <hip/hip_runtime.h>

#include "gbuffer.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"    // (det_sincos: the GI rays' helper, static in the shared header)
#include "common.hip.hpp"
#pragma clang diagnostic pop

namespace rtk {
namespace dev {

__global__ __launch_bounds__(256) void k_gbuffer(GbufferArgs G) {
    const RenderArgs &A = G.r;
    // the wave index is wave-uniform: say so, and with it the unit, the view and the block's corner (trace.hip.hpp "Wave-uniform loads")
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t group = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint64_t unit64 = group * kGbWavesPerGroup + wave_in_wg;
    if (unit64 >= (uint64_t)A.n_units || A.units_per_view == 0u) return;        // the last workgroup's spare waves, the grid's spare workgroups
    const uint32_t unit = (uint32_t)unit64;
    // units are (view, block) pairs in view-major order: the workgroups straddle views, the view belongs to the wave
    const uint32_t view = (uint32_t)__builtin_amdgcn_readfirstlane((int)(unit / A.units_per_view));
    if (view >= A.n_views) return;                       // purely defensive: launch_gbuffer refuses a launch whose units are not n_views x units_per_view
    const uint32_t block = unit - view * A.units_per_view;
    const uint32_t blocks_x = (A.width + 7u) >> 3;
    const uint32_t row = block / blocks_x;
    const uint32_t lane = __lane_id();
    const uint32_t px = (block - row * blocks_x) * 8u + (lane & 7u), py = row * 8u + (lane >> 3);
    const bool valid = (px < A.width) & (py < A.height);

    // (the RNG key is the pixel's index inside ITS view, as for a frame: equal cameras give equal views)
    const uint32_t rkey = root_key(pcg_hash(A.seed), py * A.width + px, (uint32_t)G.sample);
    Ray ray;
    if (A.views != nullptr) {
        const float *cam = A.views + (size_t)view * 12u;                        // wave-uniform: fetched through the scalar cache
        ray = camera_ray_of(A, cam, cam + 3, px, py, rkey);
    } else {
        ray = camera_ray(A, px, py, rkey);
    }

    Cand c;
    c.t = kFltMax; c.u = 0.0f; c.v = 0.0f; c.k = kMiss;
    // most waves of most views look past the scene: the root box first, and nothing else is set up when no ray enters it
    const bool in_root = enters_root(A.tree, ray, valid);
    __shared__ __attribute__((aligned(16))) float wave_bundles[kGbWavesPerGroup][kMaxBundles * kBundleFloats];
    if (wave_any(in_root)) {
        Stats st = {0, 0, 0, 0, 0, 0};
        SliceCtx sx = {nullptr, 0u, 0u, true, 0u, wave_bundles[wave_in_wg & 3u]};
        // camera rays leave the camera: the apex of their pencil bundle (a hint for the culling, never a result)
        c = trace<RTK_TRACE_WAVE, false, false, 1, true>(A.tree, nullptr, ray, true, in_root, st, sx, kAutoMinLanes, -1.0f, kClsHasApex, ray.o);
    }
    if (!valid) return;

    // ---- the planes: miss values are k_intersect's (kernels.hip), the background for the albedo
    const bool hit = c.k != kMiss;
    float t = -1.0f, u = 0.0f, v = 0.0f;
    V3 P = mk(0.f, 0.f, 0.f), hn = mk(0.f, 0.f, 0.f);
    V3 alb = mk(A.background[0], A.background[1], A.background[2]);
    uint32_t tri = kMiss, mesh = kMiss, material = kMiss;
    if (hit) {
        const Surface s = reconstruct(A.tree, c);
        t = c.t; u = c.u; v = c.v;
        P = ray.o + (c.t * ray.d);                                              // kd_tree_simd.hpp:254
        hn = s.hit_normal;
        tri = s.tri; mesh = s.mesh; material = s.material;
        if ((G.mask & kGbAlbedo) != 0u) {
            const DevMaterial *mat = A.materials + s.material;
            if (mat->kind == RTK_MAT_TEXTURE && A.tri_uv != nullptr)            // texture_material: the colour color_hit lights (render.hpp:234-235)
                alb = sample_texture(A.textures + mat->texture, A.tri_uv + s.tri, c.u, c.v, A.tex_pixels);
            else
                alb = mk(mat->albedo[0], mat->albedo[1], mat->albedo[2]);
        }
    }
    // dword stores only (the planes are 4-byte aligned, no more), 64-bit indices
    const size_t i = ((size_t)view * A.height + py) * (size_t)A.width + px;
    if ((G.mask & kGbDepth) != 0u) G.depth[i] = t;
    if ((G.mask & kGbPosition) != 0u) { float *o = G.position + i * 3u; o[0] = P.x; o[1] = P.y; o[2] = P.z; }
    if ((G.mask & kGbNormal) != 0u) { float *o = G.normal + i * 3u; o[0] = hn.x; o[1] = hn.y; o[2] = hn.z; }
    if ((G.mask & kGbAlbedo) != 0u) { float *o = G.albedo + i * 3u; o[0] = alb.x; o[1] = alb.y; o[2] = alb.z; }
    if ((G.mask & kGbBary) != 0u) { float *o = G.bary + i * 2u; o[0] = u; o[1] = v; }
    if ((G.mask & kGbTri) != 0u) G.tri[i] = tri;
    if ((G.mask & kGbMesh) != 0u) G.mesh[i] = mesh;
    if ((G.mask & kGbMaterial) != 0u) G.material[i] = material;
}

}  // namespace dev

hipError_t launch_gbuffer(const dev::GbufferArgs &G, uint32_t grid_x, uint32_t grid_y, hipStream_t s) {
    const dev::RenderArgs &A = G.r;
    if (A.n_units == 0u) return hipSuccess;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    if (A.width == 0u || A.height == 0u || A.n_views == 0u || (G.mask & kGbAllPlanes) == 0u) return hipErrorInvalidValue;
    if (gbuffer_blocks(A.width, A.height) != (uint64_t)A.units_per_view || (uint64_t)A.units_per_view * A.n_views != (uint64_t)A.n_units)
        return hipErrorInvalidValue;
    if (A.views == nullptr && A.n_views != 1u) return hipErrorInvalidValue;
    if ((uint64_t)grid_x * grid_y < gbuffer_groups(A.n_units) || grid_x > kGbGridX || grid_y > 65535u) return hipErrorInvalidValue;
    const void *planes[kGbPlanes] = {G.depth, G.position, G.normal, G.albedo, G.bary, G.tri, G.mesh, G.material};
    for (int i = 0; i < kGbPlanes; ++i)
        if ((G.mask >> i & 1u) != 0u && (planes[i] == nullptr || (reinterpret_cast<uintptr_t>(planes[i]) & 3u) != 0u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_gbuffer, dim3(grid_x, grid_y), dim3(64u * kGbWavesPerGroup), 0, s, G);
    return hipGetLastError();
}

}  // namespace rtk
