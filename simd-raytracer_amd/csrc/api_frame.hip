// C-ABI, frames: a frame's geometry and launch arguments, the counters of the last call, RTK_TRACE_AUTO's engine trial, rtk_render_frame
// and camera rays.  The engines are api_stream.hip's (render_stream) and api_order.hip's (render_megakernel).
#include <cmath>
#include <cstring>
#include <mutex>

#include "camera_plan.hpp"
#include "render_internal.hpp"

namespace rtk {

int frame_geom(const rtk_accel *a, const rtk_render_params *p, FrameGeom &g) {
    if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
    const int64_t w = p->width > 0 ? p->width : a->scene.width;
    const int64_t h = p->height > 0 ? p->height : a->scene.height;
    if (w <= 0 || h <= 0 || w > 65536 || h > 65536) return fail(RTK_ERR_INVALID, "image size must be in [1, 65536]");
    if (p->spp < 1) return fail(RTK_ERR_INVALID, "spp must be >= 1");
    if (p->max_ray_depth < 0 || p->max_ray_depth > kMaxRayDepth)
        return fail(RTK_ERR_INVALID, "max_ray_depth must be in [0, 16]");
    if (p->diffuse_rays < 0 || p->diffuse_rays > 32767) return fail(RTK_ERR_INVALID, "diffuse_rays must be in [0, 32767]");
    if (!valid_frame_mode(p->trace_mode)) return fail(RTK_ERR_INVALID, "unknown trace_mode");
    if (p->sample_begin < 0 || p->sample_count < 0 || p->sample_begin >= p->spp ||
        int64_t(p->sample_begin) + p->sample_count > p->spp)
        return fail(RTK_ERR_INVALID, "sample_begin / sample_count must select samples inside [0, spp)");
    if (p->sample_count == 0 && p->sample_begin != 0) return fail(RTK_ERR_INVALID, "sample_count == 0 means all samples: sample_begin must be 0");
    g.sample_begin = p->sample_begin;
    g.sample_end = p->sample_count == 0 ? p->spp : p->sample_begin + p->sample_count;
    g.world = p->world_size > 1 ? p->world_size : 1;
    g.rank = p->world_size > 1 ? p->rank : 0;
    if (g.rank < 0 || g.rank >= g.world) return fail(RTK_ERR_INVALID, "rank must be in [0, world_size)");
    g.width = uint32_t(w); g.height = uint32_t(h);
    g.bucket = uint32_t(a->scene.bucket_size > 0 ? a->scene.bucket_size : 64);
    g.tiles_x = (g.width + g.bucket - 1) / g.bucket;
    g.tiles_y = (g.height + g.bucket - 1) / g.bucket;
    g.n_buckets = g.tiles_x * g.tiles_y;
    g.blocks_side = (g.bucket + 7) / 8;
    g.buckets_per_rank = (g.n_buckets + uint32_t(g.world) - 1) / uint32_t(g.world);
    g.skew_q = (g.world > 1 && g.tiles_x % uint32_t(g.world) == 0u) ? g.tiles_x / uint32_t(g.world) : 0u;
    return RTK_OK;
}

// output pixels of this rank: the whole frame, or its buckets (padded so that every rank has equal length) of a sharded one
size_t out_pixels(const FrameGeom &g) {
    return g.world > 1 ? size_t(g.buckets_per_rank) * g.bucket * g.bucket : size_t(g.width) * g.height;
}

// primary rays of this rank: pixels of its buckets x samples of this call
uint64_t primary_rays_of_rank(const FrameGeom &g) {
    uint64_t pixels = 0;
    for (uint32_t j = 0; j < g.buckets_per_rank; ++j) {
        const uint32_t b = dev::rank_bucket(uint32_t(g.rank), j, uint32_t(g.world), g.skew_q);
        if (b >= g.n_buckets) continue;
        const uint32_t bx = (b % g.tiles_x) * g.bucket, by = (b / g.tiles_x) * g.bucket;
        const uint32_t w = (bx + g.bucket <= g.width) ? g.bucket : g.width - bx;
        const uint32_t h = (by + g.bucket <= g.height) ? g.bucket : g.height - by;
        pixels += uint64_t(w) * h;
    }
    return pixels * uint64_t(g.sample_end - g.sample_begin);
}

// What a frame and a radiance batch share: zeroed arguments with the scene as the device holds it and the way occlusion
// queries are answered.  `stats_mode`: rtk_render_params.collect_stats; a radiance batch passes 0.
dev::RenderArgs scene_args(const rtk_accel *a, int stats_mode) {
    dev::RenderArgs A;
    std::memset(&A, 0, sizeof(A));
    A.tree = tree_view(a);
    A.materials = a->d_materials.get(); A.lights = a->d_lights.get();
    A.textures = a->d_textures.get(); A.tri_uv = a->topo.tri_uv.get(); A.tex_pixels = a->d_tex_pixels.get();
    A.n_lights = int(a->scene.lights.size());
    A.has_refractive = a->has_refractive ? 1 : 0;
    std::memcpy(A.background, a->scene.background, sizeof(A.background));
    A.slice_min_tris = a->knobs.slice_min_tris;
    // Occlusion queries (is_occluded) may stop at the first hit nearer than the light when no material is transmissive: the
    // frame is bit-identical (trace.hip.hpp, `exit_t`), only the per-ray work counters shrink.  collect_stats == 1 counts the
    // reference's work (every ray traced to the end), collect_stats == 2 the work of the production path.
    A.shadow_exit = (a->knobs.shadow_exit && !a->has_refractive && stats_mode != 1) ? 1 : 0;
    // Likewise an occlusion query whose light contribution is +-0 in every channel is counted in `rays` but not traced
    // (common.hip.hpp, unlit_query): the same frame and ray count, less work under collect_stats 0 and 2.
    A.skip_unlit = (a->knobs.skip_unlit_shadow && !a->has_refractive && stats_mode != 1) ? 1 : 0;
    A.occl_on = (a->occl_on && stats_mode == 0) ? 1 : 0;
    A.occl = A.tree;
    if (A.occl_on) {
        A.occl.nodes = a->geom.occl_nodes.get(); A.occl.leaves = a->geom.occl_leaves.get(); A.occl.leaves_fast = nullptr; A.occl.n_leaves = a->occl_n_leaves;
        A.occl.tris = a->geom.occl_tris.get(); A.occl.tri_ids = a->geom.occl_ids.get();
    }
    return A;
}

namespace {

// the counters of a frame or a part of a call start at zero, with the tail behind them (counters.hpp): the block in use is filled
hipError_t fill_counters(rtk_accel *a, hipStream_t s) {
    a->counter_fills += 1;
    return hipMemsetAsync(counters_now(a), 0, kCounterAllocWords * sizeof(unsigned long long), s);
}

}  // namespace

// ... by everyone but a steady frame (render_frame_impl), whose block the frame before it cleared: what that frame knew is forgotten
hipError_t zero_counters(rtk_accel *a, hipStream_t s) {
    a->cnt.forget();
    return fill_counters(a, s);
}

// what rtk_render_last_counters and rtk_render_last_critical_path go by
void record_last(rtk_accel *a, hipStream_t s, bool stats, uint64_t primary) {
    a->last_stream = s;
    a->last_stats = stats;
    a->last_primary = primary;
}

// the accel's own camera: the scene's at rtk_accel_build, then whatever rtk_accel_set_camera stored there
rtk_view accel_camera(const rtk_accel *a) {
    rtk_view v;
    std::memcpy(v.position, a->scene.cam_pos, sizeof(v.position));
    std::memcpy(v.matrix, a->scene.cam_mat, sizeof(v.matrix));
    return v;
}

// the camera half: what k_camera_rays and the frame kernels make camera rays from
void camera_args(const rtk_view &cam, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A) {
    std::memcpy(A.cam_pos, cam.position, sizeof(A.cam_pos));
    std::memcpy(A.cam_mat, cam.matrix, sizeof(A.cam_mat));
    A.width = g.width; A.height = g.height;
    const CameraScalars c = camera_scalars(g.width, g.height, p->fov_degrees);               // (camera_plan.hpp: the one copy)
    A.aspect = c.aspect;
    A.tan_half_fov = c.tan_half_fov;
    A.spp = p->spp; A.seed = p->seed;
    A.width_f = c.width_f; A.height_f = c.height_f; A.spp_f = static_cast<float>(p->spp);
}

// what every engine's launch arguments hold for a frame of shape `g` seen from `cam` into `d_out`
dev::RenderArgs frame_args(const rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view &cam, float *d_out) {
    dev::RenderArgs A = scene_args(a, p->collect_stats);
    camera_args(cam, p, g, A);
    A.max_depth = p->max_ray_depth; A.diffuse_rays = p->diffuse_rays;
    A.gi_div_f = static_cast<float>(p->diffuse_rays + 1);
    A.sample_begin = g.sample_begin; A.sample_end = g.sample_end;
    A.shadow_bias = p->shadow_bias; A.reflection_bias = p->reflection_bias; A.refraction_bias = p->refraction_bias;
    A.bucket = g.bucket; A.tiles_x = g.tiles_x; A.tiles_y = g.tiles_y; A.n_buckets = g.n_buckets;
    A.blocks_per_bucket_side = g.blocks_side; A.buckets_per_rank = g.buckets_per_rank;
    A.rank = g.rank; A.world = g.world; A.compact = g.world > 1 ? 1 : 0; A.skew_q = g.skew_q;
    A.out = d_out; A.counters = counters_now(a);
    return A;
}

namespace {

// RTK_TRACE_AUTO for frames: fork-free scenes go through the GROUP4 megakernel; on scenes whose ray
// trees fork (refraction, diffuse GI) which engine wins depends on how much of the frame forks, so both are timed on the first
// frames of a shape (frame_plan.hpp EngineTrial), then the verdict as soon as the events have completed (hipEventQuery, never a
// host wait).  `trial`: {start, end} to record around the engine, or null.
int choose_engine(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, bool forks, bool &stream, hipEvent_t trial[2]) {
    stream = p->trace_mode == RTK_TRACE_STREAM || (p->trace_mode == RTK_TRACE_AUTO && forks);
    if (!EngineTrial::applies(p->trace_mode, forks, p->collect_stats != 0)) return RTK_OK;
    uint64_t tsig[3];
    shape_sig(g, p->spp, p->max_ray_depth, p->diffuse_rays, tsig);
    if (a->knobs.auto_trials) {
        for (TimedEvent &e : a->trial_ev) RTK_MEM(e.ensure());
        if (a->trial.waiting(tsig)) {                                       // both timed: is the verdict in?
            float t_stream = 0.f, t_mega = 0.f;
            if (hipEventQuery(a->trial_ev[1].get()) == hipSuccess && hipEventQuery(a->trial_ev[3].get()) == hipSuccess &&
                hipEventElapsedTime(&t_stream, a->trial_ev[0].get(), a->trial_ev[1].get()) == hipSuccess &&
                hipEventElapsedTime(&t_mega, a->trial_ev[2].get(), a->trial_ev[3].get()) == hipSuccess)
                a->trial.verdict(t_stream, t_mega);
            else (void)hipGetLastError();                                   // not ready yet: clear the sticky "not ready"
        }
    }
    const EngineTrial::Step step = a->trial.next(tsig, a->knobs.auto_trials);
    stream = step.stream;
    if (step.record != EngineTrial::kNoRecord) { trial[0] = a->trial_ev[step.record].get(); trial[1] = a->trial_ev[step.record + 1].get(); }
    return RTK_OK;
}

// `steady`: a frame of its own (not a view of a views call, whose counters are folded part by part): a megakernel frame without
// statistics then counts into the block the frame before it cleared and clears the other one for the next (frame_plan.hpp CounterState).
int render_frame_body(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view &cam, float *d_out, hipStream_t s, bool steady) {
    // the megakernel comes in two builds: the lean one (diffuse / reflective / constant materials only) and the general one
    // (template FORKS: + refraction, diffuse GI, textures), so that the lean one does not carry the general one's registers
    const bool forks = scene_forks(a, p->diffuse_rays), general = scene_general(a, p->diffuse_rays);
    bool stream = false;
    hipEvent_t trial[2] = {nullptr, nullptr};
    RTK_TRY(choose_engine(a, p, g, forks, stream, trial));
    // The counters start at zero.  In the steady state no fill is issued for that: the blocks change places, and this frame's kernel
    // clears the one the previous frame counted into.  Everything else fills the block in use, as every other user of the counters does.
    const CounterState::Step cs = a->cnt.frame(s, steady && !stream && p->collect_stats == 0);
    if (cs.fill) RTK_HIP(fill_counters(a, s));
    dev::RenderArgs A = frame_args(a, p, g, cam, d_out);                 // (A.counters: the block in use, now that it is chosen)
    if (cs.carry) A.zero_next = counters_other(a);
    // buckets past the end of the frame (padding so that every rank has equal length) stay zero
    if (g.world > 1 && g.sample_begin == 0) RTK_HIP(hipMemsetAsync(d_out, 0, out_pixels(g) * 3 * sizeof(float), s));
    // (the streaming pipeline starts its trial itself, behind its workspace allocation)
    if (trial[0] && !stream) RTK_HIP(hipEventRecord(trial[0], s));
    // (the retired two-pass engine's mode keeps its refusal; its frames are GROUP4's: frame_plan.hpp OrderState::frame_mode)
    if (p->trace_mode == RTK_TRACE_TWOPASS && p->spp != 1) return fail(RTK_ERR_UNSUPPORTED, "RTK_TRACE_TWOPASS needs spp == 1");
    if (stream) RTK_TRY(render_stream(a, p, g, A, forks, general, trial, s));
    else RTK_TRY(render_megakernel(a, a->fb, p, g, A, general, s));
    if (trial[1]) RTK_HIP(hipEventRecord(trial[1], s));
    record_last(a, s, p->collect_stats != 0, primary_rays_of_rank(g));
    return RTK_OK;
}

}  // namespace

// One frame seen from `cam` (the accel's own camera, or a view of rtk_render_views' view-after-view path): the camera is part
// of the launch arguments, so frames already enqueued keep theirs.
int render_frame_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view &cam, float *d_out, hipStream_t s, bool steady) {
    const int rc = render_frame_body(a, p, g, cam, d_out, s, steady);
    if (rc != RTK_OK) a->cnt.forget();                                   // (the state ran ahead of the launches)
    return rc;
}

namespace {

int render_device_impl(rtk_accel *a, const rtk_render_params *p, float *d_out, hipStream_t s) {
    FrameGeom g;
    RTK_TRY(frame_geom(a, p, g));
    if (!d_out) return fail(RTK_ERR_INVALID, "null output buffer");
    return render_frame_impl(a, p, g, accel_camera(a), d_out, s, true);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_render_output_floats(const rtk_accel *a, const rtk_render_params *p, size_t *n_floats) {
    return abi_guard([&]() -> int {
        if (!n_floats) return fail(RTK_ERR_INVALID, "null n_floats");
        FrameGeom g;
        RTK_TRY(frame_geom(a, p, g));
        *n_floats = out_pixels(g) * 3;
        return RTK_OK;
    });
}

int rtk_render_frame_device(rtk_accel *a, const rtk_render_params *p, float *d_out, void *stream) {
    return abi_guard([&]() -> int {
        if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return render_device_impl(a, p, d_out, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_last_counters(rtk_accel *a, rtk_counters *c) {
    return abi_guard([&]() -> int {
        if (!a || !c) return fail(RTK_ERR_INVALID, "null accel or counters");
        std::lock_guard<std::mutex> lock(a->mu);
        if (!a->on_device) return fail(RTK_ERR_INVALID, "no frame has been rendered on this accel");
        RTK_HIP(hipSetDevice(a->device));
        RTK_HIP(hipStreamSynchronize(a->last_stream));
        unsigned long long h[kCounterWords];
        RTK_HIP(hipMemcpy(h, counters_now(a), sizeof(h), hipMemcpyDeviceToHost));
        counters_from_block(h, a->last_stats, c);
        for (int i = 0; i < kRayCounterShards; ++i) c->rays += h[kRayShardWord + i];      // the frame kernel shards its ray counter
        c->primary = a->last_primary;
        return RTK_OK;
    });
}

int rtk_render_last_critical_path(rtk_accel *a, double *ms) {
    return abi_guard([&]() -> int {
        if (!a || !ms) return fail(RTK_ERR_INVALID, "null accel or ms");
        std::lock_guard<std::mutex> lock(a->mu);
        if (!a->on_device) return fail(RTK_ERR_INVALID, "no frame has been rendered on this accel");
        RTK_HIP(hipSetDevice(a->device));
        RTK_HIP(hipStreamSynchronize(a->last_stream));
        unsigned long long shard[kRayCounterShards], ticks = 0;
        RTK_HIP(hipMemcpy(shard, counters_now(a) + kCriticalWord, sizeof(shard), hipMemcpyDeviceToHost));
        for (unsigned long long t : shard) ticks = t > ticks ? t : ticks;
        *ms = double(ticks) * 1.0e-5;                                        // s_memrealtime counts at 100 MHz; 0 = no block took 10 us
        return RTK_OK;
    });
}

int rtk_debug_counter_fills(rtk_accel *a, uint64_t *fills) {
    return abi_guard([&]() -> int {
        if (!a || !fills) return fail(RTK_ERR_INVALID, "null accel or fills");
        std::lock_guard<std::mutex> lock(a->mu);
        *fills = a->counter_fills;
        return RTK_OK;
    });
}

int rtk_render_frame(rtk_accel *a, const rtk_render_params *p, float *rgb, rtk_counters *counters) {
    return abi_guard([&]() -> int {
        if (!a || !p || !rgb) return fail(RTK_ERR_INVALID, "null accel, params or rgb");
        if (p->world_size > 1) return fail(RTK_ERR_INVALID, "rtk_render_frame renders whole frames; use rtk_render_frame_device for sharded output");
        size_t nf = 0;
        RTK_TRY(rtk_render_output_floats(a, p, &nf));
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            HostStage stage;                         // (the call's own: freed when the block is left)
            StageLayout L;
            const int o_rgb = L.add(nf);
            RTK_MEM(stage.reserve(L));
            // a later pass of a progressive frame continues the running per-pixel sums the previous pass left in `rgb`
            if (p->sample_begin > 0) RTK_HIP_AS(stage.upload(o_rgb, rgb), "upload of the running sums");
            RTK_TRY(render_device_impl(a, p, stage.at<float>(o_rgb), nullptr));
            RTK_HIP_AS(stage.download(o_rgb, rgb), "frame copy");
        }
        if (counters) return rtk_render_last_counters(a, counters);
        return RTK_OK;
    });
}

int rtk_tiles_assemble_device(const rtk_accel *a, const rtk_render_params *p, const float *d_gathered, float *d_rgb, void *stream) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        RTK_TRY(frame_geom(a, p, g));
        if (!d_gathered || !d_rgb) return fail(RTK_ERR_INVALID, "null buffer");
        dev::AssembleArgs A;
        A.gathered = d_gathered; A.rgb = d_rgb; A.width = g.width; A.height = g.height; A.bucket = g.bucket;
        A.tiles_x = g.tiles_x; A.world = uint32_t(g.world); A.buckets_per_rank = g.buckets_per_rank; A.skew_q = g.skew_q;
        RTK_HIP_AS(launch_assemble(A, static_cast<hipStream_t>(stream)), "launch k_assemble");
        return RTK_OK;
    });
}

// ---------------------------------------------------------------- camera rays

int rtk_camera_rays_device(rtk_accel *a, const rtk_render_params *p, int32_t sample, rtk_ray *d_rays, void *stream) {
    return abi_guard([&]() -> int {
        if (!a || !p || !d_rays) return fail(RTK_ERR_INVALID, "null accel, params or ray buffer");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        FrameGeom g;
        RTK_TRY(frame_geom(a, p, g));
        if (sample < 0 || sample >= p->spp) return fail(RTK_ERR_INVALID, "sample must be in [0, spp)");
        dev::RenderArgs A;
        std::memset(&A, 0, sizeof(A));
        camera_args(accel_camera(a), p, g, A);
        RTK_HIP_AS(launch_camera_rays(A, sample, d_rays, static_cast<hipStream_t>(stream)), "launch k_camera_rays");
        return RTK_OK;
    });
}

int rtk_camera_rays(rtk_accel *a, const rtk_render_params *p, int32_t sample, rtk_ray *rays) {
    return abi_guard([&]() -> int {
        if (!a || !p || !rays) return fail(RTK_ERR_INVALID, "null accel, params or ray buffer");
        FrameGeom g;
        RTK_TRY(frame_geom(a, p, g));
        HostStage stage;                             // (the call's own: freed when it returns)
        StageLayout L;
        const int o_rays = L.add(uint64_t(g.width) * g.height * (sizeof(rtk_ray) / 4));
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            RTK_MEM(stage.reserve(L));
        }
        RTK_TRY(rtk_camera_rays_device(a, p, sample, stage.at<rtk_ray>(o_rays), nullptr));
        RTK_HIP_AS(stage.download(o_rays, rays), "camera ray copy");
        return RTK_OK;
    });
}

}  // extern "C"
