// Host plan of rtk_render_gbuffer (api_gbuffer.hip): what the call refuses and in which order, how many 8x8 pixel blocks a view
// has, how the (view, block) units of a call become workgroups and grids, how many elements each plane holds, and how a call whose
// units do not fit one launch is cut into launches of whole views.  Plain integers, no HIP, no accel:
// tests/cpp/gbuffer_plan_check.cpp runs it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rtk.h"

namespace rtk {

// the planes of rtk_gbuffer, in the struct's order: bit i of a plane mask = plane i is wanted
enum : uint32_t {
    kGbDepth = 1u, kGbPosition = 2u, kGbNormal = 4u, kGbAlbedo = 8u, kGbBary = 16u, kGbTri = 32u, kGbMesh = 64u, kGbMaterial = 128u,
    kGbAllPlanes = 255u
};
constexpr int kGbPlanes = 8;
constexpr uint32_t kGbComps[kGbPlanes] = {1u, 3u, 3u, 3u, 2u, 1u, 1u, 1u};      // dwords per pixel of each plane (60 B in all)

constexpr uint32_t kGbWavesPerGroup = 4;                      // k_gbuffer: one wave per unit, four to a workgroup
// Units of one launch at most.  A unit's number (view * units_per_view + block) is a uint32_t in the kernel; 2^30 leaves the sums
// around it far from wrapping.  A single view has at most 8192 x 8192 = 2^26 units, so a launch always holds whole views.
constexpr uint64_t kGbLaunchUnits = uint64_t(1) << 30;
// The grid of a launch is two-dimensional, x first: the runtime refuses more than 2^32 - 1 threads along a dimension, and 2^28
// workgroups of 256 threads are more than that.  gx <= 2^20 (2^28 threads), gy <= 2^8.
constexpr uint32_t kGbGridX = 1u << 20;
// pixels of a call at most: 12 bytes per pixel of the widest plane stay far inside a size_t and an int64
constexpr uint64_t kGbMaxPixels = uint64_t(1) << 56;

inline const void *gbuffer_plane(const rtk_gbuffer &o, int i) {
    switch (i) {
        case 0: return o.depth; case 1: return o.position; case 2: return o.normal; case 3: return o.albedo;
        case 4: return o.bary; case 5: return o.tri; case 6: return o.mesh; default: return o.material;
    }
}
inline uint32_t gbuffer_mask(const rtk_gbuffer &o) {
    uint32_t m = 0u;
    for (int i = 0; i < kGbPlanes; ++i)
        if (gbuffer_plane(o, i) != nullptr) m |= 1u << i;
    return m;
}

// What the call refuses once rtk_render_frame's own checks of *p have passed (frame_geom), in the order rtk.h gives; nullptr = the
// call goes on (to "n_views == 0 is RTK_OK", then to the device).  width, height: the frame's, as frame_geom resolved them.
inline const char *gbuffer_refusal(const rtk_render_params &p, int32_t sample, bool views_null, int32_t n_views, uint32_t mask,
                                   uint32_t width, uint32_t height) {
    if (sample < 0 || sample >= p.spp) return "sample must be in [0, spp)";
    if (p.world_size > 1) return "a g-buffer is not sharded: deal whole views to the ranks";
    if (p.collect_stats != 0) return "a g-buffer collects no per-ray statistics";
    if (n_views < 0) return "n_views must be >= 0";
    if (views_null && n_views != 1) return "without views the call renders the accel's camera: n_views must be 1";
    if ((mask & kGbAllPlanes) == 0u) return "no plane is wanted: at least one pointer of rtk_gbuffer must be set";
    if (uint64_t(n_views) * width * height > kGbMaxPixels) return "too many pixels for one call";     // (2^31 * 2^32 does not wrap)
    return nullptr;
}

inline uint32_t gbuffer_blocks_x(uint32_t width) { return (width + 7u) / 8u; }
inline uint64_t gbuffer_blocks(uint32_t width, uint32_t height) {                // 8x8 blocks of one view, anchored at its corner
    return uint64_t(gbuffer_blocks_x(width)) * ((height + 7u) / 8u);
}
inline uint64_t gbuffer_groups(uint64_t units) { return (units + kGbWavesPerGroup - 1u) / kGbWavesPerGroup; }

// elements (dwords) of plane i for n_views views; the refusal above keeps the product inside 64 bits
inline uint64_t gbuffer_plane_elems(int plane, uint64_t n_views, uint32_t width, uint32_t height) {
    return n_views * width * height * kGbComps[plane];
}

struct GbufferLaunch {
    uint64_t first_view;                                      // of the call
    uint32_t n_views, n_units;                                // whole views; n_units = n_views * units_per_view < 2^32
    uint32_t groups, grid_x, grid_y;                          // workgroups the units need, and a grid that covers them
};
struct GbufferPlan {
    uint32_t units_per_view = 0;
    uint64_t total_units = 0;
    std::vector<GbufferLaunch> launches;
};

// the grid of `groups` workgroups: grid_x * grid_y >= groups, the surplus workgroups of the last row return at once
inline void gbuffer_grid(uint64_t groups, uint32_t &gx, uint32_t &gy) {
    gx = groups < kGbGridX ? uint32_t(groups) : kGbGridX;
    gy = gx == 0u ? 0u : uint32_t((groups + gx - 1u) / gx);
}

// limit_units: units of one launch at most (kGbLaunchUnits; a test lowers it).  A view with more units than that still gets a
// launch, of its own.  Views are rendered in order, so launch c begins where launch c - 1 ended.
inline GbufferPlan plan_gbuffer(uint64_t n_views, uint32_t width, uint32_t height, uint64_t limit_units = kGbLaunchUnits) {
    GbufferPlan P;
    const uint64_t per_view = gbuffer_blocks(width, height);
    P.units_per_view = uint32_t(per_view);
    P.total_units = n_views * per_view;
    if (n_views == 0 || per_view == 0) return P;
    uint64_t per_launch = limit_units / per_view;
    if (per_launch == 0) per_launch = 1;
    for (uint64_t first = 0; first < n_views; first += per_launch) {
        GbufferLaunch L;
        L.first_view = first;
        L.n_views = uint32_t(n_views - first < per_launch ? n_views - first : per_launch);
        L.n_units = uint32_t(uint64_t(L.n_views) * per_view);
        const uint64_t groups = gbuffer_groups(L.n_units);
        L.groups = uint32_t(groups);
        gbuffer_grid(groups, L.grid_x, L.grid_y);
        P.launches.push_back(L);
    }
    return P;
}

}  // namespace rtk
