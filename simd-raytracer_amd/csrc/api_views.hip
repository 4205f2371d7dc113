// C-ABI, rtk_render_views and the accel's own camera (rtk_accel_get_camera / _set_camera): many cameras in one launch of the
// megakernel, or view after view through the other engines.
#include <cstring>
#include <mutex>

#include "render_internal.hpp"

using namespace rtk;

namespace {

// Units (8x8 pixel blocks of all views) of one views launch; a call with more is cut into launches of whole views.  The order
// of a launch is made by ONE workgroup (k_order_by_cost, ~2 us per 1,000 units: 66 us for the 32,400 of a 1920x1080 frame), so
// this keeps the sort near a quarter of a millisecond in front of a launch that itself takes a multiple of that; and four
// full-HD views are already 25 times more workgroups than the chip holds at once: a longer list overlaps no further tails.
// The number is rtk_knobs::views_launch_units (131,072; RTK_VIEWS_LAUNCH_UNITS lowers it, so that a test reaches the cut).

// the megakernel engines, without per-ray statistics, take all views in one launch; everything else goes view after view
bool views_one_launch(const rtk_accel *a, const rtk_render_params *p) {
    if (p->collect_stats != 0) return false;
    if (p->trace_mode == RTK_TRACE_GROUP4 || p->trace_mode == RTK_TRACE_GROUP8 || p->trace_mode == RTK_TRACE_GROUP16) return true;
    return p->trace_mode == RTK_TRACE_AUTO && !scene_forks(a, p->diffuse_rays);
}

int views_check(const rtk_accel *a, const rtk_render_params *p, const void *views, int32_t n_views, const void *out, FrameGeom &g) {
    RTK_TRY(frame_geom(a, p, g));
    if (n_views < 0) return fail(RTK_ERR_INVALID, "n_views must be >= 0");
    if (p->world_size > 1) return fail(RTK_ERR_INVALID, "views are not sharded: deal whole views to the ranks");
    if (n_views > 0 && (!views || !out)) return fail(RTK_ERR_INVALID, "null views or output buffer");
    return RTK_OK;
}

// `h_views`: the views in host memory, or null when the caller has them on the device only (`d_views`, always set).
int render_views_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view *h_views, const rtk_view *d_views,
                      int32_t n_views, float *d_out, hipStream_t s) {
    const size_t stride = size_t(g.width) * g.height * 3;
    const size_t n = size_t(n_views);
    if (views_one_launch(a, p)) {
        const size_t per_view = g.blocks();                                                       // <= 2^26: a launch of one view fits 31 bits
        const ViewsLaunches cut = views_launches(n, per_view, a->knobs.views_launch_units);
        const size_t per_launch = cut.per_launch;
        RTK_TRY(render_parts(a, a->fb_views, cut.n_parts, p, g, s, [&](size_t c) {
            const size_t first = c * per_launch, cnt = n - first < per_launch ? n - first : per_launch;
            dev::RenderArgs A = frame_args(a, p, g, accel_camera(a), d_out + first * stride);     // (the camera in the arguments is not read)
            A.views = reinterpret_cast<const float *>(d_views + first);
            A.n_views = uint32_t(cnt); A.units_per_view = uint32_t(per_view); A.view_stride = stride;
            return A;
        }));
    } else {
        std::vector<rtk_view> back;
        if (!h_views) {                          // the engines of this path take the camera in their launch arguments: fetch the views
            back.resize(n);
            RTK_HIP(hipMemcpyAsync(back.data(), d_views, n * sizeof(rtk_view), hipMemcpyDeviceToHost, s));
            RTK_HIP(hipStreamSynchronize(s));
            h_views = back.data();
        }
        CallCounters cc{a, n > 1, s};
        RTK_TRY(cc.begin());
        for (size_t v = 0; v < n; ++v) {
            RTK_TRY(render_frame_impl(a, p, g, h_views[v], d_out + v * stride, s, false));
            RTK_TRY(cc.after_part());
        }
        RTK_TRY(cc.end());
    }
    record_last(a, s, p->collect_stats != 0, primary_rays_of_rank(g) * uint64_t(n));
    return RTK_OK;
}

}  // namespace

extern "C" {

int rtk_accel_get_camera(const rtk_accel *a, rtk_view *out) {
    return abi_guard([&]() -> int {
        if (!a || !out) return fail(RTK_ERR_INVALID, "null accel or view");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        *out = accel_camera(a);
        return RTK_OK;
    });
}

int rtk_accel_set_camera(rtk_accel *a, const rtk_view *view) {
    return abi_guard([&]() -> int {
        if (!a || !view) return fail(RTK_ERR_INVALID, "null accel or view");
        std::lock_guard<std::mutex> lock(a->mu);
        std::memcpy(a->scene.cam_pos, view->position, sizeof(a->scene.cam_pos));
        std::memcpy(a->scene.cam_mat, view->matrix, sizeof(a->scene.cam_mat));
        // The launch order learnt under the previous camera changes no result, only the order.  It starts over (the first-frame prior,
        // then the new camera's costs), as after an update of the geometry: measured, neither choice wins every run on the first
        // frame, and the third takes 0.20 ms against 0.30 under a kept order, which is served until its next re-sort (rtk.h;
        // RTK_CAMERA_KEEPS_ORDER=1 keeps it).  RTK_TRACE_AUTO's
        // engine verdict stays: started over at every move, the trial of a camera in motion would never end.
        // (rectangles are seen from the accel's camera; views bring their own)
        if (!a->knobs.camera_keeps_order) forget_orders(a, kKeepViewOrders | kKeepTrial);
        return RTK_OK;
    });
}

int rtk_render_views_device(rtk_accel *a, const rtk_render_params *p, const rtk_view *d_views, int32_t n_views, float *d_out, void *stream) {
    return abi_guard([&]() -> int {
        if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
        FrameGeom g;
        RTK_TRY(views_check(a, p, d_views, n_views, d_out, g));
        if (n_views == 0) return RTK_OK;
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return render_views_impl(a, p, g, nullptr, d_views, n_views, d_out, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_views(rtk_accel *a, const rtk_render_params *p, const rtk_view *views, int32_t n_views, float *rgb, rtk_counters *counters) {
    return abi_guard([&]() -> int {
        if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
        FrameGeom g;
        RTK_TRY(views_check(a, p, views, n_views, rgb, g));
        if (n_views == 0) return RTK_OK;
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            const uint64_t n = uint64_t(n_views);
            HostStage &st = a->stage;
            StageLayout L;
            const int tab = L.add(n * (sizeof(rtk_view) / 4)), o_rgb = L.add(n * g.width * g.height * 3);
            RTK_MEM(st.reserve(L));
            RTK_HIP(st.upload(tab, views));
            // a later pass of progressive views continues the running per-pixel sums the previous pass left in `rgb`
            if (p->sample_begin > 0) RTK_HIP(st.upload(o_rgb, rgb));
            RTK_TRY(render_views_impl(a, p, g, views, st.at<rtk_view>(tab), n_views, st.at<float>(o_rgb), nullptr));
            RTK_HIP(st.download(o_rgb, rgb));
        }
        if (counters) return rtk_render_last_counters(a, counters);
        return RTK_OK;
    });
}

}  // extern "C"
