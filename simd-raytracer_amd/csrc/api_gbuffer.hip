// C-ABI, rtk_render_gbuffer: the first hit of every camera ray as planes (depth, position, normal, albedo, barycentrics, ids), for
// many cameras in one launch.  The arithmetic of the call -- refusals, units, grids, the cut into launches -- is gbuffer_plan.hpp;
// the kernel is gbuffer.hip.  Nothing here touches the accel's camera, its cost tables or its counters.
#include <cstring>
#include <mutex>

#include "gbuffer.hpp"
#include "render_internal.hpp"

using namespace rtk;

namespace {

// everything the call refuses, in the order rtk.h gives; on RTK_OK `g` is the frame's geometry and `mask` the planes wanted
int gbuffer_check(const rtk_accel *a, const rtk_render_params *p, int32_t sample, const void *views, int32_t n_views, const rtk_gbuffer *out,
                  FrameGeom &g, uint32_t &mask) {
    if (!a || !p || !out) return fail(RTK_ERR_INVALID, "null accel, params or plane table");
    RTK_TRY(frame_geom(a, p, g));
    mask = gbuffer_mask(*out);
    if (const char *why = gbuffer_refusal(*p, sample, views == nullptr, n_views, mask, g.width, g.height)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

// The launches of a call: `d_views` null = the accel's camera (one view), `planes` on the device.  No allocation, no host block.
int gbuffer_device_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, int32_t sample, const rtk_view *d_views, int32_t n_views,
                        const rtk_gbuffer &planes, uint32_t mask, hipStream_t s) {
    dev::GbufferArgs G;
    std::memset(&G, 0, sizeof(G));
    dev::RenderArgs &A = G.r;
    gbuffer_scene_args(a, p, g, A);
    G.sample = sample; G.mask = mask;
    const GbufferPlan plan = plan_gbuffer(uint64_t(n_views), g.width, g.height);
    const uint64_t view_pixels = uint64_t(g.width) * g.height;
    for (const GbufferLaunch &L : plan.launches) {
        A.views = d_views ? reinterpret_cast<const float *>(d_views + L.first_view) : nullptr;
        A.n_views = L.n_views; A.units_per_view = plan.units_per_view; A.n_units = L.n_units;
        const uint64_t at = L.first_view * view_pixels;                  // pixels of the views before this launch
        G.depth = planes.depth ? planes.depth + at : nullptr;
        G.position = planes.position ? planes.position + at * 3u : nullptr;
        G.normal = planes.normal ? planes.normal + at * 3u : nullptr;
        G.albedo = planes.albedo ? planes.albedo + at * 3u : nullptr;
        G.bary = planes.bary ? planes.bary + at * 2u : nullptr;
        G.tri = planes.tri ? planes.tri + at : nullptr;
        G.mesh = planes.mesh ? planes.mesh + at : nullptr;
        G.material = planes.material ? planes.material + at : nullptr;
        RTK_HIP_AS(launch_gbuffer(G, L.grid_x, L.grid_y, s), "launch k_gbuffer");
    }
    return RTK_OK;
}

}  // namespace

namespace rtk {

void gbuffer_scene_args(const rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A) {
    A.tree = tree_view(a);
    A.tree.scalar_surv = a->knobs.batch_scalar_surv ? 1 : 0;            // (as the batched intersect walks it)
    A.materials = a->d_materials.get();
    A.textures = a->d_textures.get(); A.tri_uv = a->topo.tri_uv.get(); A.tex_pixels = a->d_tex_pixels.get();
    std::memcpy(A.background, a->scene.background, sizeof(A.background));
    camera_args(accel_camera(a), p, g, A);                              // (with views the camera in the arguments is not read)
    A.world = 1;
}

}  // namespace rtk

int rtk_render_gbuffer_device(rtk_accel *a, const rtk_render_params *p, int32_t sample, const rtk_view *d_views, int32_t n_views,
                              const rtk_gbuffer *out, void *stream) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        uint32_t mask = 0u;
        RTK_TRY(gbuffer_check(a, p, sample, d_views, n_views, out, g, mask));
        if (n_views == 0) return RTK_OK;
        for (int i = 0; i < kGbPlanes; ++i)
            if ((reinterpret_cast<uintptr_t>(gbuffer_plane(*out, i)) & 3u) != 0u) return fail(RTK_ERR_INVALID, "plane pointers must be 4-byte aligned");
        if ((reinterpret_cast<uintptr_t>(d_views) & 3u) != 0u) return fail(RTK_ERR_INVALID, "the view table must be 4-byte aligned");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return gbuffer_device_impl(a, p, g, sample, d_views, n_views, *out, mask, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_gbuffer(rtk_accel *a, const rtk_render_params *p, int32_t sample, const rtk_view *views, int32_t n_views, const rtk_gbuffer *out) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        uint32_t mask = 0u;
        RTK_TRY(gbuffer_check(a, p, sample, views, n_views, out, g, mask));
        if (n_views == 0) return RTK_OK;
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        // the wanted planes (plane i of rtk_gbuffer is plane i of the stage), then the view table
        const uint64_t n = uint64_t(n_views);
        HostStage &st = a->stage;
        StageLayout L;
        for (int i = 0; i < kGbPlanes; ++i) L.add(gbuffer_plane_elems(i, n, g.width, g.height), (mask >> i & 1u) != 0u);
        const int tab = L.add(n * (sizeof(rtk_view) / 4), views != nullptr);
        RTK_MEM(st.reserve(L));
        RTK_HIP(st.upload(tab, views));
        const rtk_gbuffer d = {st.at<float>(0), st.at<float>(1), st.at<float>(2), st.at<float>(3), st.at<float>(4),
                               st.at<uint32_t>(5), st.at<uint32_t>(6), st.at<uint32_t>(7)};
        RTK_TRY(gbuffer_device_impl(a, p, g, sample, st.at<rtk_view>(tab), n_views, d, mask, nullptr));
        void *const host[kGbPlanes] = {out->depth, out->position, out->normal, out->albedo, out->bary, out->tri, out->mesh, out->material};
        for (int i = 0; i < kGbPlanes; ++i) RTK_HIP(st.download(i, host[i]));   // (a copy on the null stream is behind the kernel and blocks the host)
        return RTK_OK;
    });
}
