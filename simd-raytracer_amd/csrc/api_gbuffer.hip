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
    A.tree = tree_view(a);
    A.tree.scalar_surv = a->knobs.batch_scalar_surv ? 1 : 0;            // (as the batched intersect walks it)
    A.materials = a->d_materials.get();
    A.textures = a->d_textures.get(); A.tri_uv = a->topo.tri_uv.get(); A.tex_pixels = a->d_tex_pixels.get();
    std::memcpy(A.background, a->scene.background, sizeof(A.background));
    camera_args(accel_camera(a), p, g, A);                              // (with views the camera in the arguments is not read)
    A.world = 1;
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
        // the wanted planes one behind the other in one staging buffer of dwords
        const uint64_t n = uint64_t(n_views);
        uint64_t off[kGbPlanes + 1] = {0};
        for (int i = 0; i < kGbPlanes; ++i) off[i + 1] = off[i] + ((mask >> i & 1u) ? gbuffer_plane_elems(i, n, g.width, g.height) : 0u);
        RTK_MEM(a->gb_out.reserve(size_t(off[kGbPlanes]), grow_bytes()));
        if (views) {
            RTK_MEM(a->gb_views.reserve(size_t(n), grow_half<4>()));
            RTK_HIP(hipMemcpy(a->gb_views.get(), views, size_t(n) * sizeof(rtk_view), hipMemcpyHostToDevice));
        }
        uint32_t *const base = a->gb_out.get();
        const auto at = [&](int i) -> uint32_t * { return (mask >> i & 1u) ? base + off[i] : nullptr; };
        rtk_gbuffer d;
        d.depth = reinterpret_cast<float *>(at(0)); d.position = reinterpret_cast<float *>(at(1)); d.normal = reinterpret_cast<float *>(at(2));
        d.albedo = reinterpret_cast<float *>(at(3)); d.bary = reinterpret_cast<float *>(at(4));
        d.tri = at(5); d.mesh = at(6); d.material = at(7);
        RTK_TRY(gbuffer_device_impl(a, p, g, sample, views ? a->gb_views.get() : nullptr, n_views, d, mask, nullptr));
        void *const host[kGbPlanes] = {out->depth, out->position, out->normal, out->albedo, out->bary, out->tri, out->mesh, out->material};
        for (int i = 0; i < kGbPlanes; ++i)                              // (a copy on the null stream is behind the kernel and blocks the host)
            if (mask >> i & 1u) RTK_HIP(hipMemcpy(host[i], base + off[i], size_t(off[i + 1] - off[i]) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return RTK_OK;
    });
}
