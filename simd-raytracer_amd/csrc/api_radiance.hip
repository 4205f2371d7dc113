// C-ABI, rtk_accel_radiance: the colours of caller-supplied rays, the streaming pipeline's second client.  The same batches carry
// a frame's own camera rays on the streaming path of rtk_render_regions and in rtk_render_adaptive (radiance_frame_chunk).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "render_internal.hpp"
#include "stream_plan.hpp"

namespace rtk {

namespace {

int radiance_check(const rtk_accel *a, const void *rays, const void *ids, size_t n, const rtk_radiance_params *p, const void *rgb) {
    if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
    if (p->trace_mode != RTK_TRACE_AUTO && p->trace_mode != RTK_TRACE_STREAM)
        return fail(RTK_ERR_INVALID, "trace_mode of a radiance batch must be RTK_TRACE_AUTO or RTK_TRACE_STREAM");
    if (p->max_ray_depth < 0 || p->max_ray_depth > kMaxRayDepth) return fail(RTK_ERR_INVALID, "max_ray_depth must be in [0, 16]");
    if (p->diffuse_rays < 0 || p->diffuse_rays > 32767) return fail(RTK_ERR_INVALID, "diffuse_rays must be in [0, 32767]");
    if (p->sample < 0) return fail(RTK_ERR_INVALID, "sample must be >= 0");
    if (!std::isfinite(p->shadow_bias) || !std::isfinite(p->reflection_bias) || !std::isfinite(p->refraction_bias))
        return fail(RTK_ERR_INVALID, "shadow_bias, reflection_bias and refraction_bias must be finite");
    if (n > (size_t(1) << 38)) return fail(RTK_ERR_INVALID, "too many rays for one call");
    if (n > 0 && (!rays || !rgb)) return fail(RTK_ERR_INVALID, "null ray or colour buffer");
    if (!ids && n > (size_t(1) << 32)) return fail(RTK_ERR_INVALID, "more than 2^32 rays need explicit ids");
    return RTK_OK;
}

}  // namespace

// The batch cut into chunks, every chunk one run of the streaming pipeline (level 0 = the chunk's rays) on one of the accel's
// lanes, followed by its counter fold and its overflow fallback.  Nothing here waits on the host.
int radiance_device_impl(rtk_accel *a, const rtk_ray *d_rays, const uint32_t *d_ids, size_t n, const rtk_radiance_params *p,
                         float *d_rgb, hipStream_t s, uint32_t *n_chunks_out) {
    a->cnt.forget();                                     // (no steady frame: frame_plan.hpp CounterState)
    dev::RenderArgs A = scene_args(a, 0);
    // one colour per ray: "sample 0 of 1" for k_combine, whatever sample the RNG keys name
    A.spp = 1; A.sample_begin = 0; A.sample_end = 1; A.spp_f = 1.0f;
    A.max_depth = p->max_ray_depth; A.diffuse_rays = p->diffuse_rays; A.seed = p->seed;
    A.gi_div_f = static_cast<float>(p->diffuse_rays + 1);
    A.shadow_bias = p->shadow_bias; A.reflection_bias = p->reflection_bias; A.refraction_bias = p->refraction_bias;
    A.world = 1;
    const bool forks = scene_forks(a, p->diffuse_rays);
    StreamSetup u = stream_args(a, A, p->diffuse_rays, forks);
    const RadiancePlan plan = plan_radiance_chunks(n, u.factor, u.node_bytes, u.budget, a->knobs.stream_lanes);
    const int lanes = plan.lanes;
    if (n_chunks_out) *n_chunks_out = uint32_t(plan.n_chunks);
    StreamWorkspace &w = a->stream;
    RTK_TRY(ensure_stream_ws(w, a->device, 0, plan.nodes, a->scene.lights.size(), false, lanes));
    RTK_MEM(a->d_rad_counters.reserve(radiance_total_word(dev::kStreamLanes) + kRadianceTotalWords));
    unsigned long long *const total = a->d_rad_counters.get() + radiance_total_word(dev::kStreamLanes);
    RTK_TRY(claim_stream_ws(w, s));
    RTK_HIP(hipMemsetAsync(total, 0, kRadianceTotalWords * sizeof(unsigned long long), s));
    dev::StreamArgs &S = u.S;
    S.n_lanes = 1;                                       // overflow words: a chunk is judged on its own lane's alone (k_combine, depth 0)
    S.user_sample = uint32_t(p->sample); S.user_cull = p->cull ? 1u : 0u;
    RTK_TRY(fork_lanes(w, lanes, s));
    const bool side = a->knobs.stream_side && lanes <= 2 && lanes <= a->knobs.stream_side_below;      // (a frame counts samples in flight, a batch chunks)
    for (size_t i = 0; i < plan.n_chunks; ++i) {
        const int j = int(i % size_t(lanes));
        const hipStream_t ls = j == 0 ? s : w.lane_stream[j];
        const size_t first = i * plan.chunk, cn = n - first < plan.chunk ? n - first : plan.chunk;
        S.ws = w.lane_ws[j];
        for (int k = 0; k < dev::kStreamLanes; ++k) S.lane_overflow[k] = S.ws.ctrl + dev::kCtrlOverflow;
        S.user_rays = d_rays + first; S.user_ids = d_ids ? d_ids + first : nullptr;
        S.user_n = uint32_t(cn); S.user_id0 = uint32_t(first);
        S.n_root = uint32_t((cn + 63) / 64 * 64); S.n_level0 = S.n_root;
        S.r.out = d_rgb + first * 3;
        S.r.counters = a->d_rad_counters.get() + radiance_lane_word(j);
        // ctrl: a chunk zeroes its lane's and its counter block on the lane's stream (the overflow word included: it is the chunk's)
        RTK_HIP(hipMemsetAsync(S.ws.ctrl, 0, dev::kCtrlWords * sizeof(uint32_t), ls));
        RTK_HIP(hipMemsetAsync(S.r.counters, 0, kCounterWords * sizeof(unsigned long long), ls));
        // ordering events: none between chunks (each writes its own colours); lane_done is recorded here, for the join
        hipError_t e = launch_stream_sample(S, false, u.deep_level, u.deep_mode, u.sort_from, ls, nullptr, nullptr, side ? &w.lane_side[j] : nullptr, u.slices);
        // tail: the chunk's rays into the call's total, and the per-ray fallback if its queues overflowed
        if (e == hipSuccess) e = launch_radiance_fold(S, total, ls);
        if (e == hipSuccess) e = launch_radiance_fallback(S, total, ls);
        if (e != hipSuccess) return hip_fail(e, "launch radiance chunk");
        if (j != 0) RTK_HIP(hipEventRecord(w.lane_done[j].get(), ls));
    }
    RTK_TRY(join_lanes(w, lanes, s));
    return release_stream_ws(w, s);
}

rtk_radiance_params frame_radiance_params(const rtk_render_params *p) {
    rtk_radiance_params rp;
    rp.max_ray_depth = p->max_ray_depth; rp.diffuse_rays = p->diffuse_rays; rp.seed = p->seed; rp.sample = 0;
    rp.shadow_bias = p->shadow_bias; rp.reflection_bias = p->reflection_bias; rp.refraction_bias = p->refraction_bias;
    rp.cull = 1; rp.trace_mode = RTK_TRACE_STREAM;
    return rp;
}

int radiance_frame_chunk(rtk_accel *a, const rtk_ray *d_rays, const uint32_t *d_ids, size_t n, const rtk_radiance_params *rp, float *d_rgb,
                         hipStream_t s) {
    RTK_TRY(radiance_device_impl(a, d_rays, d_ids, n, rp, d_rgb, s, nullptr));
    RTK_HIP_AS(launch_add_word(counters_now(a), a->d_rad_counters.get() + radiance_total_word(dev::kStreamLanes) + kRadianceRays, s), "launch k_add_word");
    return RTK_OK;
}

}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_accel_radiance_device(rtk_accel *a, const rtk_ray *d_rays, const uint32_t *d_ids, size_t n, const rtk_radiance_params *p,
                              float *d_rgb, void *stream) {
    return abi_guard([&]() -> int {
        RTK_TRY(radiance_check(a, d_rays, d_ids, n, p, d_rgb));
        if (n == 0) return RTK_OK;
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return radiance_device_impl(a, d_rays, d_ids, n, p, d_rgb, static_cast<hipStream_t>(stream), nullptr);
    });
}

int rtk_accel_radiance(rtk_accel *a, const rtk_ray *rays, const uint32_t *ids, size_t n, const rtk_radiance_params *p, float *rgb,
                       rtk_counters *counters) {
    return abi_guard([&]() -> int {
        RTK_TRY(radiance_check(a, rays, ids, n, p, rgb));
        if (n == 0) {
            if (counters) std::memset(counters, 0, sizeof(*counters));
            return RTK_OK;
        }
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        HostStage &st = a->stage;
        StageLayout L;
        const int i_rays = L.add(uint64_t(n) * (sizeof(rtk_ray) / 4)), i_ids = L.add(n, ids != nullptr), o_rgb = L.add(uint64_t(n) * 3);
        RTK_MEM(st.reserve(L));
        RTK_HIP(st.upload(i_rays, rays));
        RTK_HIP(st.upload(i_ids, ids));
        uint32_t n_chunks = 0;
        RTK_TRY(radiance_device_impl(a, st.at<rtk_ray>(i_rays), st.at<uint32_t>(i_ids), n, p, st.at<float>(o_rgb), nullptr, &n_chunks));
        RTK_HIP(st.download(o_rgb, rgb));
        unsigned long long h[kRadianceTotalWords] = {};
        RTK_HIP(hipMemcpy(h, a->d_rad_counters.get() + radiance_total_word(dev::kStreamLanes), sizeof(h), hipMemcpyDeviceToHost));
        if (counters) {
            std::memset(counters, 0, sizeof(*counters));
            counters->rays = h[kRadianceRays]; counters->primary = n;
        }
        if (a->knobs.stream_debug)
            std::fprintf(stderr, "[rtk radiance] rays %zu chunks %u redone %llu node_cap %u\n", n, n_chunks, h[kRadianceRedone], a->stream.ws.node_cap);
        return RTK_OK;
    });
}

}  // extern "C"
