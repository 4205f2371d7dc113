// C-ABI, everything that shades: frames, the radiance batch (the streaming pipeline's second client) and camera rays.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "accel.hpp"
#include "stream_plan.hpp"

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

namespace {

// The streams the streaming pipeline's lanes (and their k_shadow side kernels) run on belong to the PROCESS and are made once
// per device, in the order the first accel needs them: made per accel, a second accel's lanes shared hardware queues.
struct LaneStreams {
    hipStream_t lane[rtk::dev::kStreamLanes] = {};
    hipStream_t side[rtk::dev::kStreamLanes][2] = {};
};
std::mutex g_lane_mu;
LaneStreams g_lane_streams[16];

hipError_t lane_streams_for(int device, int lanes, LaneStreams **out) {
    if (device < 0 || device >= 16) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_lane_mu);
    LaneStreams &L = g_lane_streams[device];
    for (int j = 0; j < lanes && j < rtk::dev::kStreamLanes; ++j) {
        hipError_t e = hipSuccess;
        if (j > 0 && !L.lane[j]) e = hipStreamCreateWithFlags(&L.lane[j], hipStreamNonBlocking);
        for (int par = 0; par < 2 && e == hipSuccess; ++par)
            if (!L.side[j][par]) e = hipStreamCreateWithFlags(&L.side[j][par], hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    *out = &L;
    return hipSuccess;
}

}  // namespace

void free_stream_ws(rtk_accel *a) {
    a->ws_sumbuf.reset();
    for (int j = 0; j < dev::kStreamLanes; ++j) { a->ws_bufs[j].reset(); a->ws_lane[j] = dev::StreamWs{}; }
    a->ws = a->ws_lane[0];
    a->ws_shape = StreamWsShape{};
}

// (Re)allocates the streaming workspace for `pixels` output pixels.  Allocation synchronises the device, so it only
// happens when a larger frame (or more lights / multi-sample) is requested than ever before on this accel.
int ensure_stream_ws(rtk_accel *a, size_t pixels, size_t nodes, size_t lights, bool need_sum, int lanes) {
    StreamWsShape request;
    request.pixels = pixels; request.nodes = nodes; request.lights = lights; request.lanes = lanes; request.sum = need_sum;
    if (a->ws_shape.covers(request)) return RTK_OK;
    const StreamWsShape shape = a->ws_shape.grown(request);
    if (shape.refused()) return fail(RTK_ERR_INVALID, "frame too large for the streaming pipeline's 32-bit node ids");
    RTK_HIP(hipDeviceSynchronize());
    free_stream_ws(a);
    const size_t np = shape.pixels, nn = shape.nodes, nl = shape.lights, nh = StreamWsShape::hit_cap(nn);
    const int nlanes = shape.lanes;
    if (shape.sum) RTK_MEM(a->ws_sumbuf.reserve(np * 3));
    for (int j = 0; j < nlanes; ++j) {
        StreamBufs &b = a->ws_bufs[j];
        RTK_MEM(b.rays.reserve(nn));
        RTK_MEM(b.nodes.reserve(nn));
        RTK_MEM(b.hits.reserve(nh));
        RTK_MEM(b.contrib.reserve(nh * nl));
        RTK_MEM(b.ctrl.reserve(dev::kCtrlWords));
        RTK_MEM(b.node_bins.reserve(dev::kSortBins));
        RTK_MEM(b.hit_bins.reserve(dev::kSortBins));
        RTK_MEM(b.node_order.reserve(nn));
        RTK_MEM(b.hit_order.reserve(nh));
        a->ws_lane[j] = dev::StreamWs{b.rays.get(), b.nodes.get(), b.hits.get(), b.contrib.get(), a->ws_sumbuf.get(), b.ctrl.get(), uint32_t(nn), uint32_t(nh),
                                      b.node_bins.get(), b.hit_bins.get(), b.node_order.get(), b.hit_order.get()};
        RTK_MEM(a->lane_done[j].ensure());
        for (int par = 0; par < 2; ++par) {
            RTK_MEM(a->lane_side_ev[j].ready[par].ensure());
            RTK_MEM(a->lane_side_ev[j].done[par].ensure());
            a->lane_side[j].ready[par] = a->lane_side_ev[j].ready[par].get(); a->lane_side[j].done[par] = a->lane_side_ev[j].done[par].get();
        }
    }
    RTK_MEM(a->lane_fork.ensure());
    LaneStreams *L = nullptr;                // the process's lane streams (see LaneStreams); the events that order them stay this accel's own
    RTK_HIP(lane_streams_for(a->device, nlanes, &L));
    for (int j = 0; j < nlanes; ++j) {
        a->lane_stream[j] = L->lane[j];
        a->lane_side[j].stream[0] = L->side[j][0]; a->lane_side[j].stream[1] = L->side[j][1];
    }
    a->ws = a->ws_lane[0];
    a->ws_shape = shape;
    return RTK_OK;
}

namespace {

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

// the counters of a frame or a part of a call start at zero, with the tail behind them (counters.hpp): the block in use is filled
hipError_t fill_counters(rtk_accel *a, hipStream_t s) {
    a->counter_fills += 1;
    return hipMemsetAsync(counters_now(a), 0, kCounterAllocWords * sizeof(unsigned long long), s);
}

}  // namespace

// (these two are api_adaptive.hip's as well: accel.hpp)
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

// (these two are api_gbuffer.hip's as well: accel.hpp)
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
    A.aspect = static_cast<float>(g.width) / static_cast<float>(g.height);                    // render.hpp:26
    // render.hpp:55-57: `const F fov_radians = degrees_to_radians(fov_degrees)` is evaluated in double (fov_degrees is a
    // double constant, utils/convert.hpp:4-6) and ROUNDED TO FLOAT by the declaration; `std::tan(fov_radians / F(2))` is
    // then the float overload (tanf), and `screen_x *=` a float multiply (common.hip.hpp camera_ray).
    const float fov_radians = static_cast<float>(p->fov_degrees * (3.14159265358979323846 / 180.0));
    A.tan_half_fov = std::tan(fov_radians / 2.0f);
    A.spp = p->spp; A.seed = p->seed;
    A.width_f = static_cast<float>(g.width); A.height_f = static_cast<float>(g.height); A.spp_f = static_cast<float>(p->spp);
}

// ---------------------------------------------------------------- the streaming pipeline's setup, for all of its clients
// (these six are api_frame_noise.hip's as well: accel.hpp, where StreamSetup is)

// Zeroed StreamArgs with what does not depend on the client: a frame and a radiance chunk then set only what is theirs.
StreamSetup stream_args(const rtk_accel *a, const dev::RenderArgs &A, int diffuse_rays, bool forks) {
    StreamSetup u = {};
    u.S.r = A; u.S.r.tree.scalar_surv = a->knobs.stream_scalar_surv ? 1 : 0;
    u.S.key_dirs = diffuse_rays > 0 ? 1u : 0u; u.S.n_batch = 1; u.S.auto_min_lanes = a->knobs.auto_min_lanes;
    const DevNode &root = a->tree.dev_nodes[0];
    for (int k = 0; k < 3; ++k) {
        const float ext = root.hi[k] - root.lo[k];
        u.S.grid_lo[k] = root.lo[k];
        u.S.grid_scale[k] = (ext > 0.f && ext < 3.0e38f) ? 16.0f / ext : 0.f;
    }
    // measured on MI355X: the workgroup-cooperative wave walk beats the per-lane walk at every depth, even for the
    // incoherent rays behind refractive surfaces, so no level switches strategy by default
    u.deep_level = a->knobs.stream_deep_level; u.deep_mode = a->knobs.stream_deep_mode;
    // fork-free trees stay coherent; sorting them would only add launches
    u.sort_from = a->knobs.stream_sort_from >= 0 ? a->knobs.stream_sort_from : (forks ? 1 : 99);
    u.slices = a->knobs.stream_slices > 0 ? a->knobs.stream_slices : a->stream_slices_auto;
    // Ray-tree nodes per level-0 ray: the ray itself plus room for the secondary rays.  Refractive scenes fork (two children per
    // interface), so they get more head room; an overflow is caught on the device and the frame (the chunk) redone by the fallback.
    u.factor = a->knobs.stream_node_factor > 0 ? size_t(a->knobs.stream_node_factor) : (forks ? 8 : 3);
    u.node_bytes = stream_bytes_per_node(sizeof(dev::RayRec), sizeof(dev::NodeRes), sizeof(dev::HitRec), sizeof(float2), a->scene.lights.size());
    u.budget = size_t(a->knobs.stream_mem_gb) << 30;
    return u;
}

// the queues belong to the accel: whoever used them last (a STREAM frame, a batch on another stream) finishes first, on the device
int claim_stream_ws(rtk_accel *a, hipStream_t s) { RTK_HIP(a->ws_last.wait_previous(s)); return RTK_OK; }
int release_stream_ws(rtk_accel *a, hipStream_t s) { RTK_HIP(a->ws_last.record(s)); return RTK_OK; }

// fork: lane 0 is the caller's stream, the other lanes wait for everything enqueued on it so far
int fork_lanes(rtk_accel *a, int lanes, hipStream_t s) {
    if (lanes > 1) RTK_HIP(hipEventRecord(a->lane_fork.get(), s));
    for (int j = 1; j < lanes; ++j) RTK_HIP(hipStreamWaitEvent(a->lane_stream[j], a->lane_fork.get(), 0));
    return RTK_OK;
}
// join: the caller's stream continues behind the last launch of every lane
int join_lanes(rtk_accel *a, int lanes, hipStream_t s) {
    for (int j = 1; j < lanes; ++j) RTK_HIP(hipStreamWaitEvent(s, a->lane_done[j].get(), 0));
    return RTK_OK;
}

namespace {

// fresh queues: their first use is not what a frame costs -- time the pipeline on the next frame instead
void trial_abandon(rtk_accel *a, hipEvent_t trial[2]) { trial[0] = trial[1] = nullptr; a->trial.abandon(); }

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

// `trial[0]` is recorded here, behind the workspace allocation, which is not what a frame costs.
int render_stream(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const dev::RenderArgs &A, bool forks, bool general,
                  hipEvent_t trial[2], hipStream_t s) {
    StreamSetup u = stream_args(a, A, p->diffuse_rays, forks);
    const size_t n_root = g.blocks() * 64;
    const size_t nodes_per_sample = n_root * u.factor + 4096;
    const FramePlan plan = plan_frame_batches(g.sample_end - g.sample_begin, nodes_per_sample, u.node_bytes, u.budget,
                                              a->knobs.stream_lanes, a->knobs.stream_batch);
    const int batch = plan.batch, lanes = plan.lanes;
    const StreamWsShape ws_before = a->ws_shape;
    RTK_TRY(ensure_stream_ws(a, out_pixels(g), nodes_per_sample * size_t(batch), a->scene.lights.size(), p->spp > 1, lanes));
    if (trial[0] && (a->ws_shape.nodes != ws_before.nodes || a->ws_shape.lanes != ws_before.lanes)) trial_abandon(a, trial);
    if (trial[0]) RTK_HIP(hipEventRecord(trial[0], s));
    dev::StreamArgs &S = u.S;
    S.ws = a->ws; S.n_root = uint32_t(n_root); S.n_level0 = uint32_t(n_root);
    // overflow words: a frame is judged on those of all its lanes (unused slots point at lane 0's)
    S.n_lanes = uint32_t(lanes);
    for (int j = 0; j < dev::kStreamLanes; ++j) S.lane_overflow[j] = a->ws_lane[j < lanes ? j : 0].ctrl + dev::kCtrlOverflow;
    RTK_TRY(claim_stream_ws(a, s));
    // ctrl: a frame zeroes all its lanes' on the caller's stream, before the fork
    for (int j = 0; j < lanes; ++j) RTK_HIP(hipMemsetAsync(a->ws_lane[j].ctrl, 0, dev::kCtrlWords * sizeof(uint32_t), s));
    RTK_TRY(fork_lanes(a, lanes, s));
    // side streams: while few SAMPLES are in flight (a radiance batch counts chunks).  They help while few rays are in flight:
    // spp 1 16.7 -> 9.1 ms on config 3; with four lanes the GPU is full already and they cost 20 %
    const bool side = a->knobs.stream_side && lanes <= 2 && batch * lanes <= a->knobs.stream_side_below;
    for (int i = 0; i < plan.n_launch; ++i) {
        const int j = i % lanes;
        S.sample = g.sample_begin + i * batch;
        S.n_batch = uint32_t(g.sample_end - S.sample < batch ? g.sample_end - S.sample : batch);
        S.n_level0 = uint32_t(n_root) * S.n_batch;
        S.ws = a->ws_lane[j];
        const hipStream_t ls = j == 0 ? s : a->lane_stream[j];
        // ordering events: the depth-0 k_combine of a batch waits for the previous batch's, so the pixel sums stay in sample order
        const hipEvent_t wait = (lanes > 1 && i > 0) ? a->lane_done[(i - 1) % lanes].get() : nullptr;
        const hipEvent_t done = lanes > 1 ? a->lane_done[j].get() : nullptr;
        RTK_HIP_AS(launch_stream_sample(S, p->collect_stats != 0, u.deep_level, u.deep_mode, u.sort_from, ls, wait, done,
                                        side ? &a->lane_side[j] : nullptr, u.slices), "launch streaming pipeline");
    }
    RTK_TRY(join_lanes(a, lanes, s));
    S.ws = a->ws;
    // tail: the safety net -- if any queue overflowed, the megakernel renders the frame again (a no-op otherwise)
    RTK_HIP_AS(launch_stream_overflow_reset(S, s), "launch overflow reset");
    dev::RenderArgs F = A;
    F.only_if = a->ws.ctrl + dev::kCtrlOverflow;
    RTK_HIP_AS(launch_render(F, RTK_TRACE_GROUP4, p->collect_stats != 0, general, s), "launch fallback k_render");
    RTK_TRY(release_stream_ws(a, s));
    if (a->knobs.stream_debug) {
        uint32_t h[dev::kCtrlWords];
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(h, a->ws.ctrl, sizeof(h), hipMemcpyDeviceToHost);
        std::fprintf(stderr, "[rtk stream] node_cap %u hit_cap %u overflow %u; nodes per level:", a->ws.node_cap, a->ws.hit_cap, h[dev::kCtrlOverflow]);
        for (int l = 0; l <= p->max_ray_depth + 1; ++l) std::fprintf(stderr, " %u", l == 0 ? unsigned(n_root) : h[dev::kCtrlNodeCount + l]);
        std::fprintf(stderr, "; hits:");
        for (int l = 0; l <= p->max_ray_depth; ++l) std::fprintf(stderr, " %u", h[dev::kCtrlHitCount + l]);
        std::fprintf(stderr, "\n");
    }
    return RTK_OK;
}

// (capacity, never shrunk)
int ensure_feedback_ws(rtk_accel *a, rtk_cost_feedback &fb, const FrameGeom &g, size_t units, hipStream_t s) {
    if (fb.judge.get() == nullptr) {                                  // the judge block (order_judge.hpp) starts at zero, once per table
        RTK_MEM(fb.judge.reserve(kJudgeWords));
        RTK_HIP(hipMemsetAsync(fb.judge.get(), 0, kJudgeWords * sizeof(uint32_t), s));
    }
    if (fb.state.units >= units) return RTK_OK;
    const uint32_t bk = g.bucket;
    const uint64_t tx = (uint64_t(a->scene.width > 0 ? a->scene.width : 0) + bk - 1) / bk, ty = (uint64_t(a->scene.height > 0 ? a->scene.height : 0) + bk - 1) / bk;
    const size_t cap = fb.state.capacity(units, &fb == &a->fb, g.blocks_of(tx * ty));
    RTK_MEM(fb.cost.reserve(cap));
    RTK_MEM(fb.order.reserve(2 * (2 * cap + 4) + 8));                 // two sets (OrderState) of order, header, workgroup list
    RTK_MEM(fb.bins.reserve(cap));
    fb.state.units = cap;
    return RTK_OK;
}

// Set k of a table's two sets of launch lists (frame_plan.hpp OrderState): order [units], header [4], workgroup list [units].
struct ListSet { uint32_t *order, *hdr, *wg_list; };
ListSet list_set(rtk_cost_feedback &fb, int k, size_t units) {
    uint32_t *const order = fb.order.get() + size_t(k) * (2 * fb.state.units + 4);
    return {order, order + units, order + units + 4};
}

// how many workgroups set k's list has: known on the host a frame or two later; until then the launch covers every block
int read_back_count(rtk_cost_feedback &fb, const ListSet &L, hipStream_t s) {
    RTK_MEM(fb.nwgs_host.reserve(1));
    RTK_MEM(fb.nwgs_ev.ensure());
    RTK_HIP(hipMemcpyAsync(fb.nwgs_host.get(), L.hdr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RTK_HIP(hipEventRecord(fb.nwgs_ev.get(), s));
    return RTK_OK;
}

// k_order_by_cost from the costs the last frame stored, into set k, and the read-back of the list's length behind it.
// `champion`: what becomes of the champion's score (kernels.hpp kChampion*) -- behind the last frame of a segment that frame's time.
int launch_sort(rtk_accel *a, rtk_cost_feedback &fb, int k, int frame_mode, size_t units, hipStream_t s, int champion) {
    const ListSet L = list_set(fb, k, units);
    // blocks that cost less than light_cycles (background, a handful of nodes) are packed four to a workgroup: GROUP4 only
    RTK_HIP_AS(launch_order_by_cost(fb.cost.get(), fb.bins.get(), L.order, L.wg_list, L.hdr, uint32_t(units),
                                    frame_mode == RTK_TRACE_GROUP4 ? a->knobs.light_cycles >> 4 : 0u, a->knobs.order_floor_cycles >> 4, 4u, s,
                                    a->knobs.judge ? fb.judge.get() : nullptr, champion),
               "launch k_order_by_cost");
    fb.sorts += 1;
    return read_back_count(fb, L, s);
}

// Keep or take (order_judge.hpp), behind the first frame of the list in `read_set`: k_judge_order leaves the faster of that list and
// the one the frames ran before (still in the other set) in read_set.  Which one, the host does not learn: the length read back
// behind the sort may be the wrong one now, so the count is pending again (OrderState::rearm_count) and read back behind the judge;
// the launches cover every block until that copy has been seen complete.
int launch_judge(rtk_accel *a, rtk_cost_feedback &fb, int read_set, size_t units, hipStream_t s) {
    const ListSet R = list_set(fb, read_set, units), O = list_set(fb, read_set ^ 1, units);
    RTK_HIP_AS(launch_judge_order(fb.judge.get(), R.order, O.order, uint32_t(2 * units + 4), a->knobs.judge_force, s), "launch k_judge_order");
    fb.judges += 1;
    fb.state.rearm_count();
    return read_back_count(fb, R, s);
}

// The launch order of a megakernel launch of `units` units: what fb.state (frame_plan.hpp OrderState) says is launched in front of
// the frame is launched here, and the set of lists the frame reads is handed to the kernel in A.  `step`: the decisions, for the
// caller, which launches the re-sort that goes BEHIND the frame.
int order_launch(rtk_accel *a, rtk_cost_feedback &fb, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A, int frame_mode,
                 size_t units, hipStream_t s, OrderState::Step &step) {
    uint64_t sig[5];
    shape_sig(g, p->spp, p->max_ray_depth, p->diffuse_rays, sig);
    sig[3] = (uint64_t(uint32_t(g.bucket)) << 32) | (uint64_t(uint32_t(g.sample_end - g.sample_begin) & 0xFFFFu) << 16) | uint32_t(p->trace_mode);
    sig[4] = A.regions ? ((1ull << 63) | (uint64_t(A.n_regions) << 32) | uint64_t(A.n_units))   // (its list is compared by the caller)
                       : (A.views ? uint64_t(A.n_views) : 0ull);                                // (0: a frame; a views launch of one view is not one)
    RTK_TRY(ensure_feedback_ws(a, fb, g, units, s));
    step = fb.state.step(sig, frame_mode, p->collect_stats != 0, A.regions != nullptr,
                         {a->knobs.first_frame_prior, a->knobs.resort_every, a->knobs.resort_max});
    fb.list_units = units;
    const ListSet L = list_set(fb, step.read_set, units);
    // (k_block_prior: background blocks packed four to a workgroup, the others by what their centre ray looks at.  A one-shot
    // render is exactly this frame: the reference CLI renders one, src/main.cpp:13-25)
    if (step.prior)
        RTK_HIP_AS(launch_block_prior(A, fb.bins.get(), L.order, L.wg_list, L.hdr,
                                      reinterpret_cast<uint32_t *>(A.counters + kPriorScratchWord), 4u, s), "launch k_block_prior");
    // (a shape's first sort: the later ones were launched behind the frame before, into the set this frame now reads.  No frame has
    // run under a list made from costs yet: no champion)
    if (step.sort_front) RTK_TRY(launch_sort(a, fb, step.read_set, frame_mode, units, s, kChampionNone));
    if (step.use_order) { A.order_in = L.order; A.order_hdr = L.hdr; A.wg_list = L.wg_list; }
    if (&fb == &a->fb) a->cnt.after_order(step);
    A.cost_out = fb.cost.get();
    return RTK_OK;
}

// The megakernel with cost feedback: the frame time is set by the few pixel blocks whose rays graze the mesh (hundreds of
// microseconds each, against ~3 for a background block).  Started late they are the tail of the frame, so every block reports
// its cycle count and the next frame of the same shape starts them most-expensive-first.  Only the launch order
// changes: every block is rendered in full, every frame.  RTK_COST_FEEDBACK=0 turns it off.
// A.views != null (rtk_render_views): the units are the blocks of A.n_views views, all in this one launch, ordered and packed
// together; `fb` is then that launch's own set of tables.
int render_megakernel(rtk_accel *a, rtk_cost_feedback &fb, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A, bool general,
                      hipStream_t s) {
    // (a regions launch, rtk_render_regions, comes with its units counted: the blocks of its rectangles)
    const size_t units = A.regions ? size_t(A.n_units) : (A.views ? g.blocks() * A.n_views : g.blocks());
    A.n_units = uint32_t(units);
    const int frame_mode = OrderState::frame_mode(p->trace_mode, units, a->knobs.group8_below);
    OrderState::Step step = {};
    if (a->knobs.cost_feedback && units > 0 && units <= 0x7FFFFFFFull) {
        const int rc = order_launch(a, fb, p, g, A, frame_mode, units, s, step);
        if (rc != RTK_OK) { fb.forget(); return rc; }                     // (the state ran ahead of the launches)
    }
    unsigned n_wgs = 0;
    if (A.wg_list != nullptr) {
        bool ready = false;
        if (fb.state.awaits_count() && !(ready = hipEventQuery(fb.nwgs_ev.get()) == hipSuccess)) (void)hipGetLastError();   // not ready: clear the sticky status
        n_wgs = fb.state.workgroups(ready, fb.nwgs_host.get());
    }
    int rc = RTK_OK;
    // This frame is the first of a new list, and the other set still holds the list before it: the judge goes behind it.
    const bool judged = step.judge && a->knobs.judge && units <= 0x7FFFFFF0ull / 2;
    // The two frames a comparison is made of -- the last of a segment, with the sort behind it, and the challenger's first, with the
    // judge behind it -- start behind a stamp (k_stamp): both are scored from there to the start of the kernel behind them.
    if (a->knobs.judge && (judged || step.sort_behind)) {
        // ... and both are launched over every block: the challenger's first frame usually is anyway (the host has not seen its list's
        // length yet), so the champion's frame must not have the shorter launch to its advantage
        n_wgs = 0;
        const hipError_t es = launch_stamp(fb.judge.get(), s);
        if (es != hipSuccess) rc = hip_fail(es, "launch k_stamp");
    }
    const hipError_t e = rc == RTK_OK ? launch_render(A, frame_mode, p->collect_stats != 0, general, s, n_wgs) : hipSuccess;
    if (e != hipSuccess) rc = hip_fail(e, "launch k_render");
    // (the judge leaves the faster of this frame's list and the one before it in the read set)
    if (rc == RTK_OK && judged) rc = launch_judge(a, fb, step.read_set, units, s);
    // The next frame of this shape starts a new list: it is sorted here, behind this frame and from the costs it has just stored, into
    // the set no frame reads (the pinned length is this frame's no more: it has been read above).
    // (behind a judge -- RTK_COST_RESORT_EVERY=1 -- this frame's time is the challenger's and the judge has left the winner's score)
    if (rc == RTK_OK && step.sort_behind)
        rc = launch_sort(a, fb, step.write_set, frame_mode, units, s, judged ? kChampionLeave : kChampionScore);
    if (rc != RTK_OK) fb.forget();
    return rc;
}

}  // namespace

// what every engine's launch arguments hold for a frame of shape `g` seen from `cam` into `d_out`
// (api_frame_noise.hip's as well: accel.hpp)
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

// One frame seen from `cam` (the accel's own camera, or a view of rtk_render_views' view-after-view path): the camera is part
// of the launch arguments, so frames already enqueued keep theirs.
int render_frame_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view &cam, float *d_out, hipStream_t s, bool steady) {
    const int rc = render_frame_body(a, p, g, cam, d_out, s, steady);
    if (rc != RTK_OK) a->cnt.forget();                                   // (the state ran ahead of the launches)
    return rc;
}

int render_device_impl(rtk_accel *a, const rtk_render_params *p, float *d_out, hipStream_t s) {
    FrameGeom g;
    RTK_TRY(frame_geom(a, p, g));
    if (!d_out) return fail(RTK_ERR_INVALID, "null output buffer");
    return render_frame_impl(a, p, g, accel_camera(a), d_out, s, true);
}

// ---------------------------------------------------------------- rtk_render_views

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

// A call of several launches ("parts": launches of views or regions, or whole frames) with one set of counters: each part counts
// from zero in d_counters (an engine may reset its counters: the streaming pipeline's overflow fallback does) and is folded into
// the call's totals on the device; d_counters holds them at the end.  A call of one part needs, and issues, none of this.
struct CallCounters {
    rtk_accel *a;
    bool many;
    hipStream_t s;
    int begin() {
        if (!many) return RTK_OK;
        RTK_MEM(a->d_views_counters.reserve(kCounterWords));
        RTK_HIP(hipMemsetAsync(a->d_views_counters.get(), 0, kCounterWords * sizeof(unsigned long long), s));
        return RTK_OK;
    }
    int zero_part() { RTK_HIP(zero_counters(a, s)); return RTK_OK; }   // (a frame zeroes its own)
    int after_part() { if (many) RTK_HIP_AS(launch_counters_fold(counters_now(a), a->d_views_counters.get(), s), "launch k_counters_fold"); return RTK_OK; }
    int end() {
        if (many) RTK_HIP(hipMemcpyAsync(counters_now(a), a->d_views_counters.get(), kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
        return RTK_OK;
    }
};

// The parts of a call that the megakernel takes as launches of many units (views, rectangles): each with cost tables of its own
// (`tables`, grown to the part count) and folded into the call's totals.  `part_args(c)`: the launch arguments of part c.
template <typename PartArgs>
int render_parts(rtk_accel *a, std::vector<rtk_cost_feedback> &tables, size_t n_parts, const rtk_render_params *p, const FrameGeom &g,
                 hipStream_t s, PartArgs part_args) {
    if (tables.size() < n_parts) tables.resize(n_parts);
    const bool general = scene_general(a, p->diffuse_rays);
    CallCounters cc{a, n_parts > 1, s};
    RTK_TRY(cc.begin());
    for (size_t c = 0; c < n_parts; ++c) {
        dev::RenderArgs A = part_args(c);
        RTK_TRY(cc.zero_part());
        RTK_TRY(render_megakernel(a, tables[c], p, g, A, general, s));
        RTK_TRY(cc.after_part());
    }
    return cc.end();
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
// (api_adaptive.hip's as well: accel.hpp)
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
    RTK_TRY(ensure_stream_ws(a, 0, plan.nodes, a->scene.lights.size(), false, lanes));
    RTK_MEM(a->d_rad_counters.reserve(radiance_total_word(dev::kStreamLanes) + kRadianceTotalWords));
    unsigned long long *const total = a->d_rad_counters.get() + radiance_total_word(dev::kStreamLanes);
    RTK_TRY(claim_stream_ws(a, s));
    RTK_HIP(hipMemsetAsync(total, 0, kRadianceTotalWords * sizeof(unsigned long long), s));
    dev::StreamArgs &S = u.S;
    S.n_lanes = 1;                                       // overflow words: a chunk is judged on its own lane's alone (k_combine, depth 0)
    S.user_sample = uint32_t(p->sample); S.user_cull = p->cull ? 1u : 0u;
    RTK_TRY(fork_lanes(a, lanes, s));
    const bool side = a->knobs.stream_side && lanes <= 2 && lanes <= a->knobs.stream_side_below;      // (a frame counts samples in flight, a batch chunks)
    for (size_t i = 0; i < plan.n_chunks; ++i) {
        const int j = int(i % size_t(lanes));
        const hipStream_t ls = j == 0 ? s : a->lane_stream[j];
        const size_t first = i * plan.chunk, cn = n - first < plan.chunk ? n - first : plan.chunk;
        S.ws = a->ws_lane[j];
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
        hipError_t e = launch_stream_sample(S, false, u.deep_level, u.deep_mode, u.sort_from, ls, nullptr, nullptr, side ? &a->lane_side[j] : nullptr, u.slices);
        // tail: the chunk's rays into the call's total, and the per-ray fallback if its queues overflowed
        if (e == hipSuccess) e = launch_radiance_fold(S, total, ls);
        if (e == hipSuccess) e = launch_radiance_fallback(S, total, ls);
        if (e != hipSuccess) return hip_fail(e, "launch radiance chunk");
        if (j != 0) RTK_HIP(hipEventRecord(a->lane_done[j].get(), ls));
    }
    RTK_TRY(join_lanes(a, lanes, s));
    return release_stream_ws(a, s);
}

namespace {

// ---------------------------------------------------------------- rtk_render_regions

// Pixels of one chunk of the streaming path: rays, ids and colours are 40 B per pixel, so a chunk's workspace is 40 MB however
// large the rectangles are; a chunk is also one radiance batch, which likes a few hundred thousand rays at least.
constexpr uint64_t kRegionChunkPixels = uint64_t(1) << 20;

// everything the call refuses, in the order rtk.h gives
int regions_check(const rtk_accel *a, const rtk_render_params *p, const rtk_rect *rects, int32_t n_rects, int layout, const void *out,
                  FrameGeom &g) {
    RTK_TRY(frame_geom(a, p, g));
    if (p->trace_mode == RTK_TRACE_LANE || p->trace_mode == RTK_TRACE_WAVE || p->trace_mode == RTK_TRACE_TWOPASS)
        return fail(RTK_ERR_INVALID, "regions run through RTK_TRACE_AUTO, _GROUP4 / 8 / 16 or _STREAM");
    if (p->collect_stats != 0) return fail(RTK_ERR_INVALID, "regions collect no per-ray statistics");
    if (p->world_size > 1) return fail(RTK_ERR_INVALID, "regions are not sharded: deal rectangles to the ranks");
    if (n_rects < 0 || n_rects > kMaxRegions) return fail(RTK_ERR_INVALID, "n_rects must be in [0, 65536]");
    if (layout != RTK_REGIONS_IN_FRAME && layout != RTK_REGIONS_PACKED) return fail(RTK_ERR_INVALID, "unknown layout");
    if (n_rects > 0 && (!rects || !out)) return fail(RTK_ERR_INVALID, "null rectangles or output buffer");
    for (int32_t i = 0; i < n_rects; ++i)
        if (!region_valid(rects[i], g.width, g.height)) return fail(RTK_ERR_INVALID, "rectangle " + std::to_string(i) + " is not inside the frame");
    if (layout == RTK_REGIONS_IN_FRAME && regions_overlap(rects, size_t(n_rects)))
        return fail(RTK_ERR_INVALID, "rectangles overlap: RTK_REGIONS_IN_FRAME needs them pairwise disjoint");
    return RTK_OK;
}

uint64_t regions_pixels(const rtk_rect *rects, int32_t n_rects) {
    uint64_t px = 0;
    for (int32_t i = 0; i < n_rects; ++i) px += region_area(rects[i]);
    return px;
}

// The plan of the call and its table on the device.  A call whose list, layout, frame width and launch limit equal the previous
// call's finds both in place (a re-render loop uploads nothing and keeps its measured launch order); any other list is planned
// and uploaded on `s`, behind the previous call's last kernel, and every launch of it starts without an order.
int regions_table(rtk_accel *a, const FrameGeom &g, const rtk_rect *rects, size_t n, int layout, hipStream_t s) {
    const size_t limit = a->knobs.views_launch_units;
    if (a->rg_table_valid && a->rg_layout == layout && a->rg_width == g.width && a->rg_limit == limit && a->rg_rects.size() == n &&
        std::memcmp(a->rg_rects.data(), rects, n * sizeof(rtk_rect)) == 0) return RTK_OK;
    a->rg_table_valid = false;
    for (rtk_cost_feedback &f : a->fb_regions) f.forget();
    a->rg_plan = plan_regions(rects, n, layout, g.width, limit);
    const size_t n_entries = a->rg_plan.entries.size();
    if (a->rg_table.capacity() < n_entries) {
        RTK_HIP(hipDeviceSynchronize());
        RTK_MEM(a->rg_table.reserve(n_entries, grow_table()));
    } else {
        RTK_HIP(a->rg_last.wait_previous(s));                               // a call on another stream may still be reading the old table
    }
    RTK_HIP(hipMemcpyAsync(a->rg_table.get(), a->rg_plan.entries.data(), n_entries * sizeof(RegionEntry), hipMemcpyHostToDevice, s));
    a->rg_rects.assign(rects, rects + n);
    a->rg_layout = layout; a->rg_width = g.width; a->rg_limit = limit;
    a->rg_table_valid = true;
    return RTK_OK;
}

// (the rectangles have pixels: the callers return before this for a call without any)
int render_regions_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_rect *rects, int32_t n_rects, int layout,
                        float *d_out, hipStream_t s) {
    RTK_TRY(regions_table(a, g, rects, size_t(n_rects), layout, s));
    const RegionsPlan &P = a->rg_plan;
    const bool forks = scene_forks(a, p->diffuse_rays);
    const bool stream = p->trace_mode == RTK_TRACE_STREAM || (p->trace_mode == RTK_TRACE_AUTO && forks);
    dev::RenderArgs A = frame_args(a, p, g, accel_camera(a), d_out);
    if (!stream) {
        // the megakernel: one launch per RegionLaunch, each with cost tables of its own; several are folded into the call's totals
        RTK_TRY(render_parts(a, a->fb_regions, P.launches.size(), p, g, s, [&](size_t c) {
            const RegionLaunch &L = P.launches[c];
            dev::RenderArgs R = A;
            R.regions = a->rg_table.get() + L.first_entry; R.n_regions = L.n_entries; R.n_units = L.n_units;
            return R;
        }));
    } else {
        // sample by sample and chunk by chunk: camera rays + frame pixel indices, the radiance pipeline, the sums.  All of a
        // pixel's launches are on `s` (the pipeline forks onto its lanes and joins `s` again), so its sum stays in sample order.
        uint64_t largest = 0;
        for (const RegionLaunch &L : P.launches) largest = L.n_pixels > largest ? L.n_pixels : largest;
        const size_t chunk = size_t(largest < kRegionChunkPixels ? largest : kRegionChunkPixels);
        if (a->rg_rays.capacity() < chunk || a->rg_ids.capacity() < chunk || a->rg_rgb.capacity() < chunk * 3) {
            const grow_capped rule{size_t(kRegionChunkPixels)};
            RTK_HIP(hipDeviceSynchronize());
            RTK_MEM(a->rg_rays.reserve(chunk, rule));
            RTK_MEM(a->rg_ids.reserve(chunk, rule));
            RTK_MEM(a->rg_rgb.reserve(rule(chunk, 0) * 3));
        }
        rtk_radiance_params rp;
        rp.max_ray_depth = p->max_ray_depth; rp.diffuse_rays = p->diffuse_rays; rp.seed = p->seed; rp.sample = 0;
        rp.shadow_bias = p->shadow_bias; rp.reflection_bias = p->reflection_bias; rp.refraction_bias = p->refraction_bias;
        rp.cull = 1; rp.trace_mode = RTK_TRACE_STREAM;
        RTK_HIP(zero_counters(a, s));
        for (const RegionLaunch &L : P.launches) {
            A.regions = a->rg_table.get() + L.first_entry; A.n_regions = L.n_entries; A.n_units = L.n_units;
            for (uint64_t first = 0; first < L.n_pixels; first += chunk) {
                const uint32_t cn = uint32_t(L.n_pixels - first < chunk ? L.n_pixels - first : chunk);
                for (int smp = g.sample_begin; smp < g.sample_end; ++smp) {
                    RTK_HIP_AS(launch_region_rays(A, smp, first, cn, a->rg_rays.get(), a->rg_ids.get(), s), "launch k_region_rays");
                    rp.sample = smp;
                    RTK_TRY(radiance_device_impl(a, a->rg_rays.get(), a->rg_ids.get(), cn, &rp, a->rg_rgb.get(), s, nullptr));
                    RTK_HIP_AS(launch_add_word(counters_now(a), a->d_rad_counters.get() + radiance_total_word(dev::kStreamLanes) + kRadianceRays, s), "launch k_add_word");
                    RTK_HIP_AS(launch_region_accumulate(A, first, cn, a->rg_rgb.get(), smp == 0, p->spp != 1 && smp + 1 == p->spp, s), "launch k_region_accumulate");
                }
            }
        }
    }
    RTK_HIP(a->rg_last.record(s));
    record_last(a, s, false, P.total_pixels * uint64_t(g.sample_end - g.sample_begin));
    return RTK_OK;
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

int rtk_debug_order_judge(rtk_accel *a, int32_t table, int32_t index, rtk_order_judge_stats *st) {
    return abi_guard([&]() -> int {
        if (!a || !st) return fail(RTK_ERR_INVALID, "null accel or stats");
        if (table < RTK_ORDER_TABLE_FRAMES || table > RTK_ORDER_TABLE_REGIONS || index < 0) return fail(RTK_ERR_INVALID, "unknown table or negative index");
        std::lock_guard<std::mutex> lock(a->mu);
        std::memset(st, 0, sizeof(*st));
        const std::vector<rtk_cost_feedback> *many = table == RTK_ORDER_TABLE_VIEWS ? &a->fb_views : table == RTK_ORDER_TABLE_REGIONS ? &a->fb_regions : nullptr;
        if (many ? size_t(index) >= many->size() : index != 0) return RTK_OK;       // (a launch that has not run yet: zeros)
        const rtk_cost_feedback &fb = many ? (*many)[size_t(index)] : a->fb;
        st->sorts = fb.sorts; st->judges = fb.judges;
        st->units = uint32_t(fb.list_units); st->read_set = fb.state.set;
        if (!a->on_device || fb.judge.get() == nullptr) return RTK_OK;
        RTK_HIP(hipSetDevice(a->device));
        RTK_HIP(hipStreamSynchronize(a->last_stream));
        uint32_t h[kJudgeWords];
        RTK_HIP(hipMemcpy(h, fb.judge.get(), sizeof(h), hipMemcpyDeviceToHost));
        st->taken = h[kJudgeTaken]; st->rejected = h[kJudgeRejected];
        st->champion_ticks = h[kJudgeChampion]; st->challenger_ticks = h[kJudgeChallenger];
        return RTK_OK;
    });
}

int rtk_debug_order_lists(rtk_accel *a, int32_t set, uint32_t *words, size_t capacity, size_t *n_words) {
    return abi_guard([&]() -> int {
        if (!a || !n_words) return fail(RTK_ERR_INVALID, "null accel or n_words");
        if (set != 0 && set != 1) return fail(RTK_ERR_INVALID, "set must be 0 or 1");
        std::lock_guard<std::mutex> lock(a->mu);
        rtk_cost_feedback &fb = a->fb;
        const size_t units = fb.list_units;
        if (!a->on_device || units == 0 || fb.state.units < units || fb.order.get() == nullptr) { *n_words = 0; return RTK_OK; }
        *n_words = 2 * units + 4;
        if (!words) return RTK_OK;
        if (capacity < *n_words) return fail(RTK_ERR_INVALID, "capacity is below 2 * units + 4 words");
        RTK_HIP(hipSetDevice(a->device));
        RTK_HIP(hipStreamSynchronize(a->last_stream));
        RTK_HIP(hipMemcpy(words, list_set(fb, set, units).order, *n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
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
            DevBuf<float> d_out;                     // (the call's own: freed when the block is left)
            RTK_MEM(d_out.reserve(nf));
            // a later pass of a progressive frame continues the running per-pixel sums the previous pass left in `rgb`
            if (p->sample_begin > 0) RTK_HIP_AS(hipMemcpy(d_out.get(), rgb, nf * sizeof(float), hipMemcpyHostToDevice), "upload of the running sums");
            RTK_TRY(render_device_impl(a, p, d_out.get(), nullptr));
            RTK_HIP_AS(hipMemcpy(rgb, d_out.get(), nf * sizeof(float), hipMemcpyDeviceToHost), "frame copy");
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

// ---------------------------------------------------------------- batched radiance

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
        RTK_MEM(a->rad_rays.reserve(n));
        RTK_MEM(a->rad_ids.reserve(n));
        RTK_MEM(a->rad_rgb.reserve(n * 3));
        RTK_HIP(hipMemcpy(a->rad_rays.get(), rays, n * sizeof(rtk_ray), hipMemcpyHostToDevice));
        if (ids) RTK_HIP(hipMemcpy(a->rad_ids.get(), ids, n * sizeof(uint32_t), hipMemcpyHostToDevice));
        uint32_t n_chunks = 0;
        RTK_TRY(radiance_device_impl(a, a->rad_rays.get(), ids ? a->rad_ids.get() : nullptr, n, p, a->rad_rgb.get(), nullptr, &n_chunks));
        RTK_HIP(hipMemcpy(rgb, a->rad_rgb.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
        unsigned long long h[kRadianceTotalWords] = {};
        RTK_HIP(hipMemcpy(h, a->d_rad_counters.get() + radiance_total_word(dev::kStreamLanes), sizeof(h), hipMemcpyDeviceToHost));
        if (counters) {
            std::memset(counters, 0, sizeof(*counters));
            counters->rays = h[kRadianceRays]; counters->primary = n;
        }
        if (a->knobs.stream_debug)
            std::fprintf(stderr, "[rtk radiance] rays %zu chunks %u redone %llu node_cap %u\n", n, n_chunks, h[kRadianceRedone], a->ws.node_cap);
        return RTK_OK;
    });
}

// ---------------------------------------------------------------- camera and views

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
            const size_t n = size_t(n_views), nf = n * g.width * g.height * 3;
            RTK_MEM(a->views_tab.reserve(n));
            RTK_MEM(a->views_out.reserve(nf));
            RTK_HIP(hipMemcpy(a->views_tab.get(), views, n * sizeof(rtk_view), hipMemcpyHostToDevice));
            // a later pass of progressive views continues the running per-pixel sums the previous pass left in `rgb`
            if (p->sample_begin > 0) RTK_HIP(hipMemcpy(a->views_out.get(), rgb, nf * sizeof(float), hipMemcpyHostToDevice));
            RTK_TRY(render_views_impl(a, p, g, views, a->views_tab.get(), n_views, a->views_out.get(), nullptr));
            RTK_HIP(hipMemcpy(rgb, a->views_out.get(), nf * sizeof(float), hipMemcpyDeviceToHost));
        }
        if (counters) return rtk_render_last_counters(a, counters);
        return RTK_OK;
    });
}

// ---------------------------------------------------------------- regions

int rtk_render_regions_device(rtk_accel *a, const rtk_render_params *p, const rtk_rect *rects, int32_t n_rects, int layout, float *d_out,
                              void *stream) {
    return abi_guard([&]() -> int {
        if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
        FrameGeom g;
        RTK_TRY(regions_check(a, p, rects, n_rects, layout, d_out, g));
        if (n_rects == 0 || regions_pixels(rects, n_rects) == 0) return RTK_OK;
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return render_regions_impl(a, p, g, rects, n_rects, layout, d_out, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_regions(rtk_accel *a, const rtk_render_params *p, const rtk_rect *rects, int32_t n_rects, int layout, float *rgb,
                       rtk_counters *counters) {
    return abi_guard([&]() -> int {
        if (!a || !p) return fail(RTK_ERR_INVALID, "null accel or params");
        FrameGeom g;
        RTK_TRY(regions_check(a, p, rects, n_rects, layout, rgb, g));
        const uint64_t pixels = n_rects > 0 ? regions_pixels(rects, n_rects) : 0;
        if (pixels == 0) return RTK_OK;
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            // what the layout needs: the packed buffer, or the whole frame up and down, so that the caller's pixels outside the
            // rectangles come back with the bits they went up with
            const bool packed = layout == RTK_REGIONS_PACKED;
            const size_t nf = packed ? size_t(pixels) * 3 : size_t(g.width) * g.height * 3;
            RTK_MEM(a->rg_out.reserve(nf));
            if (!packed || p->sample_begin > 0) RTK_HIP(hipMemcpy(a->rg_out.get(), rgb, nf * sizeof(float), hipMemcpyHostToDevice));
            RTK_TRY(render_regions_impl(a, p, g, rects, n_rects, layout, a->rg_out.get(), nullptr));
            RTK_HIP(hipMemcpy(rgb, a->rg_out.get(), nf * sizeof(float), hipMemcpyDeviceToHost));
        }
        if (counters) return rtk_render_last_counters(a, counters);
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
        const size_t n = size_t(g.width) * g.height;
        DevBuf<rtk_ray> d;
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            RTK_MEM(d.reserve(n));
        }
        RTK_TRY(rtk_camera_rays_device(a, p, sample, d.get(), nullptr));
        RTK_HIP_AS(hipMemcpy(rays, d.get(), n * sizeof(rtk_ray), hipMemcpyDeviceToHost), "camera ray copy");
        return RTK_OK;
    });
}

}  // extern "C"
