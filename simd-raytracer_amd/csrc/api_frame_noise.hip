// C-ABI, rtk_render_frame_noise: a frame of a fixed sample count together with the noise plane rtk_denoise_frame weights by.  The
// frame is an RTK_TRACE_STREAM frame (launch_stream_frame, the launches render_stream makes: api_stream.hip), with k_frame_moments
// (frame_noise.hip) behind every batch's depth-0 k_combine; the refusals and the workspace are frame_noise_plan.hpp.  A frame whose
// queues overflowed is not handed to the megakernel, which has no statistic: the call reads the overflow word back and redoes
// itself as an adaptive render that never stops early (api_adaptive.hip), which gives the same rgb, noise, rays and primary.
// Nothing here touches the accel's camera, its cost tables, the regions table or RTK_TRACE_AUTO's trial and verdict; the counters
// are left as an RTK_TRACE_STREAM frame leaves them.
#include <mutex>

#include "frame_noise_plan.hpp"
#include "render_internal.hpp"

using namespace rtk;

namespace {

// everything the call refuses, in the order rtk.h gives; on RTK_OK `g` is the frame's geometry
int frame_noise_check(const rtk_accel *a, const rtk_render_params *p, const void *rgb, const void *noise, FrameGeom &g) {
    if (!a || !p || !rgb || !noise) return fail(RTK_ERR_INVALID, "null accel, params, rgb or noise");
    RTK_TRY(frame_geom(a, p, g));
    if (const char *why = frame_noise_refusal(*p, g.width, g.height)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

// The running sums are the adaptive render's (the redo uses them anyway): room for `pixels` of each.  Growing frees what a call on
// another stream may still use, so the device is idle first.
int ensure_moments_ws(rtk_accel *a, size_t pixels) {
    RTK_MEM(a->fn_overflow_host.reserve(1));
    if (a->ad_s1.capacity() >= pixels && a->ad_s2.capacity() >= pixels) return RTK_OK;
    RTK_HIP(hipDeviceSynchronize());
    RTK_MEM(a->ad_s1.reserve(pixels, grow_half<0>()));
    RTK_MEM(a->ad_s2.reserve(pixels, grow_half<0>()));
    return RTK_OK;
}

// The streamed frame with its statistic, everything enqueued on `s` and its lanes; `*overflowed`: what the queues said, read back
// behind the join (the one host wait of the call).
int stream_frame_noise(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, float *d_rgb, float *d_noise, hipStream_t s,
                       bool *overflowed) {
    const size_t pixels = size_t(g.width) * g.height;
    RTK_TRY(ensure_moments_ws(a, pixels));
    // the counters: what an RTK_TRACE_STREAM frame does with them (render_frame_body): no steady frame behind it, one fill
    (void)a->cnt.frame(s, false);
    RTK_HIP(zero_counters(a, s));
    StreamMoments M;
    M.s1 = a->ad_s1.get(); M.s2 = a->ad_s2.get(); M.noise = d_noise; M.n_pixels = uint32_t(pixels);
    // the sums belong to the accel, as the queues do: their previous user finishes first, on the device, before the lanes fork from `s`
    RTK_HIP(a->ad_last.wait_previous(s));
    RTK_TRY(launch_stream_frame(a, p, g, frame_args(a, p, g, accel_camera(a), d_rgb), scene_forks(a, p->diffuse_rays), true, nullptr, M, s));
    // tail: lane 0's overflow word, which now stands for all lanes, on its way to the host.  No megakernel behind it: it has no statistic.
    RTK_HIP(hipMemcpyAsync(a->fn_overflow_host.get(), a->stream.ws.ctrl + dev::kCtrlOverflow, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RTK_TRY(release_stream_ws(a->stream, s));
    RTK_HIP(a->ad_last.record(s));
    record_last(a, s, false, uint64_t(pixels) * uint64_t(g.sample_end - g.sample_begin));
    RTK_HIP(hipStreamSynchronize(s));
    *overflowed = *a->fn_overflow_host.get() != 0u;
    return RTK_OK;
}

int render_frame_noise_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, float *d_rgb, float *d_noise, hipStream_t s) {
    bool overflowed = false;
    int rc = stream_frame_noise(a, p, g, d_rgb, d_noise, s, &overflowed);
    if (rc == RTK_OK && overflowed) {
        const rtk_adaptive_params ap = frame_noise_redo(*p);
        rc = adaptive_device_impl(a, p, &ap, g, d_rgb, nullptr, d_noise, s);
        if (rc == RTK_OK) a->noise_fallbacks += 1;
    }
    if (rc != RTK_OK) a->cnt.forget();                                   // (the state ran ahead of the launches)
    return rc;
}

}  // namespace

extern "C" {

int rtk_render_frame_noise_device(rtk_accel *a, const rtk_render_params *p, float *d_rgb, float *d_noise, void *stream) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        RTK_TRY(frame_noise_check(a, p, d_rgb, d_noise, g));
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return render_frame_noise_impl(a, p, g, d_rgb, d_noise, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_frame_noise(rtk_accel *a, const rtk_render_params *p, float *rgb, float *noise, rtk_counters *counters) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        RTK_TRY(frame_noise_check(a, p, rgb, noise, g));
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            const uint64_t n = uint64_t(g.width) * g.height;
            HostStage &st = a->stage;
            StageLayout L;
            const int o_rgb = L.add(n * 3), o_noise = L.add(n);
            RTK_MEM(st.reserve(L));
            RTK_TRY(render_frame_noise_impl(a, p, g, st.at<float>(o_rgb), st.at<float>(o_noise), nullptr));
            // (a copy on the null stream is behind the kernels and blocks the host)
            RTK_HIP(st.download(o_rgb, rgb));
            RTK_HIP(st.download(o_noise, noise));
        }
        if (counters) return rtk_render_last_counters(a, counters);
        return RTK_OK;
    });
}

int rtk_debug_noise_fallbacks(rtk_accel *a, uint64_t *count) {
    return abi_guard([&]() -> int {
        if (!a || !count) return fail(RTK_ERR_INVALID, "null accel or count");
        std::lock_guard<std::mutex> lock(a->mu);
        *count = a->noise_fallbacks;
        return RTK_OK;
    });
}

}  // extern "C"
