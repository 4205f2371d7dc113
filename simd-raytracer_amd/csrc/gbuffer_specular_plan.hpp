// Host plan of rtk_render_gbuffer_specular (api_gbuffer_specular.hip): the twelve planes of rtk_gbuffer_specular -- their mask
// bits, their dwords per pixel, how many elements each holds -- and what the call refuses.  Units, grids and the cut into launches
// of whole views are rtk_render_gbuffer's own (gbuffer_plan.hpp plan_gbuffer): the two kernels walk the same (view, block) units.
// Plain integers, no HIP, no accel: tests/cpp/gbuffer_specular_plan_check.cpp runs it.
#pragma once

#include "gbuffer_plan.hpp"

namespace rtk {

// the planes of rtk_gbuffer_specular, in the struct's order: bit i of a plane mask = plane i is wanted
enum : uint32_t {
    kGsDepth = 1u, kGsPosition = 2u, kGsNormal = 4u, kGsSurfacePosition = 8u, kGsSurfaceNormal = 16u, kGsAlbedo = 32u, kGsBary = 64u,
    kGsTri = 128u, kGsMesh = 256u, kGsMaterial = 512u, kGsBounces = 1024u, kGsLastRay = 2048u,
    kGsAllPlanes = 4095u
};
constexpr int kGsPlanes = 12;
constexpr uint32_t kGsComps[kGsPlanes] = {1u, 3u, 3u, 3u, 3u, 3u, 2u, 1u, 1u, 1u, 1u, 6u};   // dwords per pixel of each plane (112 B in all)
// the widest plane has 24 bytes per pixel: 2^56 pixels (kGbMaxPixels) of it stay inside a size_t and an int64
static_assert(kGbMaxPixels <= (UINT64_MAX >> 1) / 24u, "plane sizes must not wrap");

inline const void *gbuffer_specular_plane(const rtk_gbuffer_specular &o, int i) {
    switch (i) {
        case 0: return o.depth; case 1: return o.position; case 2: return o.normal; case 3: return o.surface_position;
        case 4: return o.surface_normal; case 5: return o.albedo; case 6: return o.bary; case 7: return o.tri;
        case 8: return o.mesh; case 9: return o.material; case 10: return o.bounces; default: return o.last_ray;
    }
}
inline uint32_t gbuffer_specular_mask(const rtk_gbuffer_specular &o) {
    uint32_t m = 0u;
    for (int i = 0; i < kGsPlanes; ++i)
        if (gbuffer_specular_plane(o, i) != nullptr) m |= 1u << i;
    return m;
}

// rtk_render_gbuffer's refusals in rtk_render_gbuffer's order (gbuffer_refusal), with "all twelve planes NULL" where that call has
// "all eight": whatever it refuses before the planes comes first, the size of the call after them.
inline const char *gbuffer_specular_refusal(const rtk_render_params &p, int32_t sample, bool views_null, int32_t n_views, uint32_t mask,
                                            uint32_t width, uint32_t height) {
    if ((mask & kGsAllPlanes) == 0u) {
        const char *before = gbuffer_refusal(p, sample, views_null, n_views, kGbAllPlanes, 1u, 1u);     // (1 x 1: never too many pixels)
        return before ? before : "no plane is wanted: at least one pointer of rtk_gbuffer_specular must be set";
    }
    return gbuffer_refusal(p, sample, views_null, n_views, kGbAllPlanes, width, height);
}

// elements (dwords) of plane i for n_views views; the refusal above keeps the product inside 64 bits
inline uint64_t gbuffer_specular_plane_elems(int plane, uint64_t n_views, uint32_t width, uint32_t height) {
    return n_views * width * height * kGsComps[plane];
}

}  // namespace rtk
