// C-ABI, rtk_render_gbuffer_specular: the planes of the first surface that is shaded behind mirrors and glass, for many cameras
// in one launch.  The call is rtk_render_gbuffer's (api_gbuffer.hip) with twelve planes: its refusals and planes are
// gbuffer_specular_plan.hpp, its units, grids and launches gbuffer_plan.hpp, its launch arguments gbuffer_scene_args; the kernel is
// gbuffer_specular.hip.  Nothing here touches the accel's camera, its cost tables or its counters.
#include <cstring>
#include <mutex>

#include "gbuffer_specular.hpp"
#include "render_internal.hpp"

using namespace rtk;

namespace {

// everything the call refuses, in the order rtk.h gives; on RTK_OK `g` is the frame's geometry and `mask` the planes wanted
int specular_check(const rtk_accel *a, const rtk_render_params *p, int32_t sample, const void *views, int32_t n_views,
                   const rtk_gbuffer_specular *out, FrameGeom &g, uint32_t &mask) {
    if (!a || !p || !out) return fail(RTK_ERR_INVALID, "null accel, params or plane table");
    RTK_TRY(frame_geom(a, p, g));
    mask = gbuffer_specular_mask(*out);
    if (const char *why = gbuffer_specular_refusal(*p, sample, views == nullptr, n_views, mask, g.width, g.height)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

// plane i of `planes`, `at` pixels on (null stays null)
template <typename T>
T *plane_at(T *base, uint64_t at, int plane) { return base ? base + at * kGsComps[plane] : nullptr; }

// The launches of a call: `d_views` null = the accel's camera (one view), `planes` on the device.  No allocation, no host block.
int specular_device_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, int32_t sample, const rtk_view *d_views, int32_t n_views,
                         const rtk_gbuffer_specular &planes, uint32_t mask, hipStream_t s) {
    dev::GbufferSpecularArgs G;
    std::memset(&G, 0, sizeof(G));
    dev::RenderArgs &A = G.r;
    gbuffer_scene_args(a, p, g, A);
    A.max_depth = p->max_ray_depth; A.reflection_bias = p->reflection_bias; A.refraction_bias = p->refraction_bias;    // the chain's
    G.sample = sample; G.mask = mask;
    const GbufferPlan plan = plan_gbuffer(uint64_t(n_views), g.width, g.height);
    const uint64_t view_pixels = uint64_t(g.width) * g.height;
    for (const GbufferLaunch &L : plan.launches) {
        A.views = d_views ? reinterpret_cast<const float *>(d_views + L.first_view) : nullptr;
        A.n_views = L.n_views; A.units_per_view = plan.units_per_view; A.n_units = L.n_units;
        const uint64_t at = L.first_view * view_pixels;                  // pixels of the views before this launch
        G.depth = plane_at(planes.depth, at, 0); G.position = plane_at(planes.position, at, 1); G.normal = plane_at(planes.normal, at, 2);
        G.surface_position = plane_at(planes.surface_position, at, 3); G.surface_normal = plane_at(planes.surface_normal, at, 4);
        G.albedo = plane_at(planes.albedo, at, 5); G.bary = plane_at(planes.bary, at, 6);
        G.tri = plane_at(planes.tri, at, 7); G.mesh = plane_at(planes.mesh, at, 8); G.material = plane_at(planes.material, at, 9);
        G.bounces = plane_at(planes.bounces, at, 10); G.last_ray = plane_at(planes.last_ray, at, 11);
        RTK_HIP_AS(launch_gbuffer_specular(G, L.grid_x, L.grid_y, s), "launch k_gbuffer_specular");
    }
    return RTK_OK;
}

}  // namespace

int rtk_render_gbuffer_specular_device(rtk_accel *a, const rtk_render_params *p, int32_t sample, const rtk_view *d_views, int32_t n_views,
                                       const rtk_gbuffer_specular *out, void *stream) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        uint32_t mask = 0u;
        RTK_TRY(specular_check(a, p, sample, d_views, n_views, out, g, mask));
        if (n_views == 0) return RTK_OK;
        for (int i = 0; i < kGsPlanes; ++i)
            if ((reinterpret_cast<uintptr_t>(gbuffer_specular_plane(*out, i)) & 3u) != 0u) return fail(RTK_ERR_INVALID, "plane pointers must be 4-byte aligned");
        if ((reinterpret_cast<uintptr_t>(d_views) & 3u) != 0u) return fail(RTK_ERR_INVALID, "the view table must be 4-byte aligned");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return specular_device_impl(a, p, g, sample, d_views, n_views, *out, mask, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_gbuffer_specular(rtk_accel *a, const rtk_render_params *p, int32_t sample, const rtk_view *views, int32_t n_views,
                                const rtk_gbuffer_specular *out) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        uint32_t mask = 0u;
        RTK_TRY(specular_check(a, p, sample, views, n_views, out, g, mask));
        if (n_views == 0) return RTK_OK;
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        // the wanted planes (plane i of rtk_gbuffer_specular is plane i of the stage), then the view table
        const uint64_t n = uint64_t(n_views);
        HostStage &st = a->stage;
        StageLayout L;
        for (int i = 0; i < kGsPlanes; ++i) L.add(gbuffer_specular_plane_elems(i, n, g.width, g.height), (mask >> i & 1u) != 0u);
        const int tab = L.add(n * (sizeof(rtk_view) / 4), views != nullptr);
        RTK_MEM(st.reserve(L));
        RTK_HIP(st.upload(tab, views));
        const rtk_gbuffer_specular d = {st.at<float>(0), st.at<float>(1), st.at<float>(2), st.at<float>(3), st.at<float>(4), st.at<float>(5),
                                        st.at<float>(6), st.at<uint32_t>(7), st.at<uint32_t>(8), st.at<uint32_t>(9), st.at<uint32_t>(10),
                                        st.at<float>(11)};
        RTK_TRY(specular_device_impl(a, p, g, sample, st.at<rtk_view>(tab), n_views, d, mask, nullptr));
        void *const host[kGsPlanes] = {out->depth, out->position, out->normal, out->surface_position, out->surface_normal, out->albedo,
                                       out->bary, out->tri, out->mesh, out->material, out->bounces, out->last_ray};
        for (int i = 0; i < kGsPlanes; ++i) RTK_HIP(st.download(i, host[i]));   // (a copy on the null stream is behind the kernel and blocks the host)
        return RTK_OK;
    });
}
