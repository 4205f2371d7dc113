// rtk_render_gbuffer_specular: the first surface that is actually shaded behind mirrors and glass, as planes.  One wave per 8x8
// pixel block of one view, four waves to a workgroup, units and view fetch as k_gbuffer (gbuffer.hip).  Each lane follows the
// specular chain of its camera ray -- reflect_at off a mirror, refract_at's refraction ray through glass, its reflection ray
// under total internal reflection (shade.hip.hpp, as they stand) -- with one wave-cooperative closest-hit query per bounce for
// the lanes still on their way; a lane whose chain has ended stays in the wave as an inactive ray.  The chain's length L, the
// fold M of the mirror normals met, the end hit and the last ray are the lane's whole state; the planes are made from them after
// the loop (rtk.h has the contract).
#include <hip/hip_runtime.h>

#include "gbuffer_specular.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"    // (det_sincos: the GI rays' helper, static in the shared header)
#include "shade.hip.hpp"
#pragma clang diagnostic pop

namespace rtk {
namespace dev {

__global__ __launch_bounds__(256) void k_gbuffer_specular(GbufferSpecularArgs G) {
    const RenderArgs &A = G.r;
    // the wave index is wave-uniform: say so, and with it the unit, the view and the block's corner (trace.hip.hpp "Wave-uniform loads")
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t group = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint64_t unit64 = group * kGbWavesPerGroup + wave_in_wg;
    if (unit64 >= (uint64_t)A.n_units || A.units_per_view == 0u) return;        // the last workgroup's spare waves, the grid's spare workgroups
    const uint32_t unit = (uint32_t)unit64;
    const uint32_t view = (uint32_t)__builtin_amdgcn_readfirstlane((int)(unit / A.units_per_view));
    if (view >= A.n_views) return;                       // purely defensive: the launcher refuses units that are not n_views x units_per_view
    const uint32_t block = unit - view * A.units_per_view;
    const uint32_t blocks_x = (A.width + 7u) >> 3;
    const uint32_t row = block / blocks_x;
    const uint32_t lane = __lane_id();
    const uint32_t px = (block - row * blocks_x) * 8u + (lane & 7u), py = row * 8u + (lane >> 3);
    const bool valid = (px < A.width) & (py < A.height);

    // (the RNG key is the pixel's index inside ITS view, as for a frame: equal cameras give equal views)
    const uint32_t rkey = root_key(pcg_hash(A.seed), py * A.width + px, (uint32_t)G.sample);
    const float *cam = A.views != nullptr ? A.views + (size_t)view * 12u : nullptr;    // wave-uniform: fetched through the scalar cache
    Ray ray = cam != nullptr ? camera_ray_of(A, cam, cam + 3, px, py, rkey) : camera_ray(A, px, py, rkey);
    // the camera ray is wanted again for `position`: it waits in LDS, not in six registers across the traversal loops
    __shared__ float cam_park[kGbWavesPerGroup][6][64];
    {
        float *const park = &cam_park[wave_in_wg & 3u][0][lane];
        park[0 * 64] = ray.o.x; park[1 * 64] = ray.o.y; park[2 * 64] = ray.o.z;
        park[3 * 64] = ray.d.x; park[4 * 64] = ray.d.y; park[5 * 64] = ray.d.z;
    }

    // ---- the lane's chain state
    Cand c;                                              // the hit the chain stands on; at the end, the end hit (kMiss: no surface)
    c.t = kFltMax; c.u = 0.0f; c.v = 0.0f; c.k = kMiss;
    float L = 0.0f;
    float m00 = 1.0f, m01 = 0.0f, m02 = 0.0f, m10 = 0.0f, m11 = 1.0f, m12 = 0.0f, m20 = 0.0f, m21 = 0.0f, m22 = 1.0f;
    bool mirrored = false;
    bool glass = false;                                  // the chain went through a refraction: its rays no longer leave one point
    uint32_t k = 0u;
    bool live = valid;

    __shared__ __attribute__((aligned(16))) float wave_bundles[kGbWavesPerGroup][kMaxBundles * kBundleFloats];
    const uint32_t max_depth = (uint32_t)A.max_depth;    // <= kMaxRayDepth: the loop below ends after at most max_depth + 1 queries
    // `bounce` counts the queries of the wave; every live lane has k == bounce
    for (uint32_t bounce = 0u;; ++bounce) {
        // the root box first, and nothing else is set up when no live ray enters it
        ray.inv = mk((1.0f / ray.d.x), (1.0f / ray.d.y), (1.0f / ray.d.z));      // ray3.hpp:11-14 (make_ray's own three divisions)
        const bool in_root = enters_root(A.tree, ray, live);
        Cand got;
        got.t = kFltMax; got.u = 0.0f; got.v = 0.0f; got.k = kMiss;
        if (wave_any(in_root)) {
            Stats st = {0, 0, 0, 0, 0, 0};
            SliceCtx sx = {nullptr, 0u, 0u, true, 0u, wave_bundles[wave_in_wg & 3u]};
            // Camera rays leave the camera, and their reflections off planes leave its mirror image, L behind the ray's origin: the
            // apex of the pencil bundle (a hint for the culling, never a result).  Rays behind glass get none.
            uint32_t cls = bounce;
            V3 apex = ray.o;
            if (!glass) {
                cls |= kClsHasApex;
                if (bounce != 0u) apex = ray.o - ((L / length(ray.d)) * ray.d);
            }
            // camera rays cull back faces, secondary rays do not (render.hpp:64, :246)
            got = trace<RTK_TRACE_WAVE, false, false, 1, true>(A.tree, nullptr, ray, bounce == 0u, in_root, st, sx, kAutoMinLanes, -1.0f, cls, apex);
        }
        if (live) {
            c = got;
            if (c.k == kMiss) live = false;                                      // nothing there
            else if (k == max_depth) { c.k = kMiss; live = false; }              // color_hit returns the background, render.hpp:138-139
            else {
                const Surface s = reconstruct(A.tree, c);
                const DevMaterial *mat = A.materials + s.material;
                const int kind = mat->kind;
                if (kind == RTK_MAT_REFLECTIVE || kind == RTK_MAT_REFRACTIVE) {
                    L = L + c.t;
                    const V3 P = ray.o + (c.t * ray.d);
                    RayOD next;
                    V3 m = s.hit_normal;
                    bool fold = true;
                    if (kind == RTK_MAT_REFLECTIVE) {
                        next = reflect_at(P, s.hit_normal, ray.d, A.reflection_bias);          // render.hpp:240-242
                    } else {
                        const V3 n_shade = mat->smooth ? s.hit_normal : s.face_normal;
                        const Refraction rf = refract_at(A, mat, P, n_shade, ray.d);            // render.hpp:252-292
                        if (rf.tir) { next = rf.refl; m = normalized(n_shade); }               // the normal refract_at reflected off (up to its sign)
                        else { next = rf.refr; fold = false; glass = true; }
                    }
                    if (fold) {
                        const float w0 = (m00 * m.x + m01 * m.y) + m02 * m.z;
                        const float w1 = (m10 * m.x + m11 * m.y) + m12 * m.z;
                        const float w2 = (m20 * m.x + m21 * m.y) + m22 * m.z;
                        m00 = m00 - ((2.0f * w0) * m.x); m01 = m01 - ((2.0f * w0) * m.y); m02 = m02 - ((2.0f * w0) * m.z);
                        m10 = m10 - ((2.0f * w1) * m.x); m11 = m11 - ((2.0f * w1) * m.y); m12 = m12 - ((2.0f * w1) * m.z);
                        m20 = m20 - ((2.0f * w2) * m.x); m21 = m21 - ((2.0f * w2) * m.y); m22 = m22 - ((2.0f * w2) * m.z);
                        mirrored = true;
                    }
                    k += 1u;
                    ray.o = next.o; ray.d = next.d;
                } else {
                    live = false;                                                // the surface that is shaded: the chain ends ON it
                }
            }
        }
        if (!wave_any(live)) break;
    }
    if (!valid) return;

    // ---- the planes: the end hit's are k_gbuffer's (miss values included), over the chain's last ray
    const bool surface = c.k != kMiss;
    float depth = -1.0f, u = 0.0f, v = 0.0f;
    V3 vp = mk(0.f, 0.f, 0.f), vn = mk(0.f, 0.f, 0.f), P = mk(0.f, 0.f, 0.f), hn = mk(0.f, 0.f, 0.f);
    V3 alb = mk(A.background[0], A.background[1], A.background[2]);
    uint32_t tri = kMiss, mesh = kMiss, material = kMiss;
    if (surface) {
        const Surface s = reconstruct(A.tree, c);
        L = L + c.t;
        depth = L;
        u = c.u; v = c.v;
        P = ray.o + (c.t * ray.d);                                              // kd_tree_simd.hpp:254
        hn = s.hit_normal;
        tri = s.tri; mesh = s.mesh; material = s.material;
        if ((G.mask & kGsPosition) != 0u) {
            const float *const park = &cam_park[wave_in_wg & 3u][0][lane];
            const V3 o0 = mk(park[0 * 64], park[1 * 64], park[2 * 64]), d0 = mk(park[3 * 64], park[4 * 64], park[5 * 64]);
            vp = o0 + (L * d0);
        }
        vn = hn;
        if (mirrored)
            vn = mk((m00 * hn.x + m01 * hn.y) + m02 * hn.z, (m10 * hn.x + m11 * hn.y) + m12 * hn.z, (m20 * hn.x + m21 * hn.y) + m22 * hn.z);
        if ((G.mask & kGsAlbedo) != 0u) {
            const DevMaterial *mat = A.materials + s.material;
            if (mat->kind == RTK_MAT_TEXTURE && A.tri_uv != nullptr)            // texture_material: the colour color_hit lights (render.hpp:234-235)
                alb = sample_texture(A.textures + mat->texture, A.tri_uv + s.tri, c.u, c.v, A.tex_pixels);
            else
                alb = mk(mat->albedo[0], mat->albedo[1], mat->albedo[2]);
        }
    }
    // dword stores only (the planes are 4-byte aligned, no more), 64-bit indices
    const size_t i = ((size_t)view * A.height + py) * (size_t)A.width + px;
    if ((G.mask & kGsDepth) != 0u) G.depth[i] = depth;
    if ((G.mask & kGsPosition) != 0u) { float *o = G.position + i * 3u; o[0] = vp.x; o[1] = vp.y; o[2] = vp.z; }
    if ((G.mask & kGsNormal) != 0u) { float *o = G.normal + i * 3u; o[0] = vn.x; o[1] = vn.y; o[2] = vn.z; }
    if ((G.mask & kGsSurfacePosition) != 0u) { float *o = G.surface_position + i * 3u; o[0] = P.x; o[1] = P.y; o[2] = P.z; }
    if ((G.mask & kGsSurfaceNormal) != 0u) { float *o = G.surface_normal + i * 3u; o[0] = hn.x; o[1] = hn.y; o[2] = hn.z; }
    if ((G.mask & kGsAlbedo) != 0u) { float *o = G.albedo + i * 3u; o[0] = alb.x; o[1] = alb.y; o[2] = alb.z; }
    if ((G.mask & kGsBary) != 0u) { float *o = G.bary + i * 2u; o[0] = u; o[1] = v; }
    if ((G.mask & kGsTri) != 0u) G.tri[i] = tri;
    if ((G.mask & kGsMesh) != 0u) G.mesh[i] = mesh;
    if ((G.mask & kGsMaterial) != 0u) G.material[i] = material;
    if ((G.mask & kGsBounces) != 0u) G.bounces[i] = k;
    if ((G.mask & kGsLastRay) != 0u) {
        float *o = G.last_ray + i * 6u;
        o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z; o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z;
    }
}

}  // namespace dev

hipError_t launch_gbuffer_specular(const dev::GbufferSpecularArgs &G, uint32_t grid_x, uint32_t grid_y, hipStream_t s) {
    const dev::RenderArgs &A = G.r;
    if (A.n_units == 0u) return hipSuccess;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    if (A.width == 0u || A.height == 0u || A.n_views == 0u || (G.mask & kGsAllPlanes) == 0u) return hipErrorInvalidValue;
    if (A.max_depth < 0 || A.max_depth > kMaxRayDepth) return hipErrorInvalidValue;                 // the bound of the kernel's loop
    if (gbuffer_blocks(A.width, A.height) != (uint64_t)A.units_per_view || (uint64_t)A.units_per_view * A.n_views != (uint64_t)A.n_units)
        return hipErrorInvalidValue;
    if (A.views == nullptr && A.n_views != 1u) return hipErrorInvalidValue;
    if ((uint64_t)grid_x * grid_y < gbuffer_groups(A.n_units) || grid_x > kGbGridX || grid_y > 65535u) return hipErrorInvalidValue;
    const void *planes[kGsPlanes] = {G.depth, G.position, G.normal, G.surface_position, G.surface_normal, G.albedo, G.bary,
                                     G.tri, G.mesh, G.material, G.bounces, G.last_ray};
    for (int i = 0; i < kGsPlanes; ++i)
        if ((G.mask >> i & 1u) != 0u && (planes[i] == nullptr || (reinterpret_cast<uintptr_t>(planes[i]) & 3u) != 0u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_gbuffer_specular, dim3(grid_x, grid_y), dim3(64u * kGbWavesPerGroup), 0, s, G);
    return hipGetLastError();
}

}  // namespace rtk
