// C-ABI, rtk_render_frame_noise: a frame of a fixed sample count together with the noise plane rtk_denoise_frame weights by.  The
// frame is an RTK_TRACE_STREAM frame (render_stream's plan, lanes, fork and join: api_frame.hip), with k_frame_moments
// (frame_noise.hip) behind every batch's depth-0 k_combine; the refusals and the workspace are frame_noise_plan.hpp.  A frame whose
// queues overflowed is not handed to the megakernel, which has no statistic: the call reads the overflow word back and redoes
// itself as an adaptive render that never stops early (api_adaptive.hip), which gives the same rgb, noise, rays and primary.
// Nothing here touches the accel's camera, its cost tables, the regions table or RTK_TRACE_AUTO's trial and verdict; the counters
// are left as an RTK_TRACE_STREAM frame leaves them.
#include <mutex>

#include "accel.hpp"
#include "frame_noise_plan.hpp"
#include "stream_plan.hpp"

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
    const bool forks = scene_forks(a, p->diffuse_rays);
    // the counters: what an RTK_TRACE_STREAM frame does with them (render_frame_body): no steady frame behind it, one fill
    (void)a->cnt.frame(s, false);
    RTK_HIP(zero_counters(a, s));
    const dev::RenderArgs A = frame_args(a, p, g, accel_camera(a), d_rgb);
    StreamSetup u = stream_args(a, A, p->diffuse_rays, forks);
    const size_t n_root = g.blocks() * 64;
    const size_t nodes_per_sample = n_root * u.factor + 4096;
    const FramePlan plan = plan_frame_batches(g.sample_end - g.sample_begin, nodes_per_sample, u.node_bytes, u.budget,
                                              a->knobs.stream_lanes, a->knobs.stream_batch);
    const int batch = plan.batch, lanes = plan.lanes;
    RTK_TRY(ensure_stream_ws(a, pixels, nodes_per_sample * size_t(batch), a->scene.lights.size(), true, lanes));
    dev::StreamArgs &S = u.S;
    S.ws = a->ws; S.n_root = uint32_t(n_root); S.n_level0 = uint32_t(n_root);
    S.n_lanes = uint32_t(lanes);
    for (int j = 0; j < dev::kStreamLanes; ++j) S.lane_overflow[j] = a->ws_lane[j < lanes ? j : 0].ctrl + dev::kCtrlOverflow;
    StreamMoments M;
    M.s1 = a->ad_s1.get(); M.s2 = a->ad_s2.get(); M.noise = d_noise; M.n_pixels = uint32_t(pixels);
    // the queues and the sums belong to the accel: their previous users finish first, on the device, before the lanes fork from `s`
    RTK_TRY(claim_stream_ws(a, s));
    RTK_HIP(a->ad_last.wait_previous(s));
    for (int j = 0; j < lanes; ++j) RTK_HIP(hipMemsetAsync(a->ws_lane[j].ctrl, 0, dev::kCtrlWords * sizeof(uint32_t), s));
    RTK_TRY(fork_lanes(a, lanes, s));
    const bool side = a->knobs.stream_side && lanes <= 2 && batch * lanes <= a->knobs.stream_side_below;
    for (int i = 0; i < plan.n_launch; ++i) {
        const int j = i % lanes;
        S.sample = g.sample_begin + i * batch;
        S.n_batch = uint32_t(g.sample_end - S.sample < batch ? g.sample_end - S.sample : batch);
        S.n_level0 = uint32_t(n_root) * S.n_batch;
        S.ws = a->ws_lane[j];
        const hipStream_t ls = j == 0 ? s : a->lane_stream[j];
        // ordering events: a batch's depth-0 k_combine and k_frame_moments wait for the previous batch's, so sums and statistic stay in sample order
        const hipEvent_t wait = (lanes > 1 && i > 0) ? a->lane_done[(i - 1) % lanes].get() : nullptr;
        const hipEvent_t done = lanes > 1 ? a->lane_done[j].get() : nullptr;
        RTK_HIP_AS(launch_stream_sample(S, false, u.deep_level, u.deep_mode, u.sort_from, ls, wait, done, side ? &a->lane_side[j] : nullptr,
                                        u.slices, M), "launch streaming pipeline");
    }
    RTK_TRY(join_lanes(a, lanes, s));
    S.ws = a->ws;
    // tail: the lanes' overflow words folded into lane 0's (the counters of an overflowed frame mean nothing and are zeroed), and that
    // word on its way to the host.  No megakernel behind it: it has no statistic.
    RTK_HIP_AS(launch_stream_overflow_reset(S, s), "launch overflow reset");
    RTK_HIP(hipMemcpyAsync(a->fn_overflow_host.get(), a->ws.ctrl + dev::kCtrlOverflow, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RTK_TRY(release_stream_ws(a, s));
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
            // rgb and noise one behind the other in one staging buffer
            const size_t n = size_t(g.width) * g.height;
            RTK_MEM(a->fn_out.reserve(n * 4, grow_bytes()));
            float *const base = a->fn_out.get();
            RTK_TRY(render_frame_noise_impl(a, p, g, base, base + n * 3, nullptr));
            // (a copy on the null stream is behind the kernels and blocks the host)
            RTK_HIP(hipMemcpy(rgb, base, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
            RTK_HIP(hipMemcpy(noise, base + n * 3, n * sizeof(float), hipMemcpyDeviceToHost));
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
