// C-ABI, the streaming pipeline's host side: the workspace of an accel with its lanes, the setup all of its clients share, and the
// launches of a streamed frame (RTK_TRACE_STREAM; rtk_render_frame_noise takes the same launches with its statistic).
#include <cstdio>
#include <mutex>

#include "render_internal.hpp"
#include "stream_plan.hpp"

namespace rtk {

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

void free_stream_ws(StreamWorkspace &w) {
    w.sumbuf.reset();
    for (int j = 0; j < dev::kStreamLanes; ++j) { w.bufs[j].reset(); w.lane_ws[j] = dev::StreamWs{}; }
    w.ws = w.lane_ws[0];
    w.shape = StreamWsShape{};
}

// (Re)allocates the streaming workspace for `pixels` output pixels.  Allocation synchronises the device, so it only
// happens when a larger frame (or more lights / multi-sample) is requested than ever before on this accel.
int ensure_stream_ws(StreamWorkspace &w, int device, size_t pixels, size_t nodes, size_t lights, bool need_sum, int lanes) {
    StreamWsShape request;
    request.pixels = pixels; request.nodes = nodes; request.lights = lights; request.lanes = lanes; request.sum = need_sum;
    if (w.shape.covers(request)) return RTK_OK;
    const StreamWsShape shape = w.shape.grown(request);
    if (shape.refused()) return fail(RTK_ERR_INVALID, "frame too large for the streaming pipeline's 32-bit node ids");
    RTK_HIP(hipDeviceSynchronize());
    free_stream_ws(w);
    const size_t np = shape.pixels, nn = shape.nodes, nl = shape.lights, nh = StreamWsShape::hit_cap(nn);
    const int nlanes = shape.lanes;
    if (shape.sum) RTK_MEM(w.sumbuf.reserve(np * 3));
    for (int j = 0; j < nlanes; ++j) {
        StreamBufs &b = w.bufs[j];
        RTK_MEM(b.rays.reserve(nn));
        RTK_MEM(b.nodes.reserve(nn));
        RTK_MEM(b.hits.reserve(nh));
        RTK_MEM(b.contrib.reserve(nh * nl));
        RTK_MEM(b.ctrl.reserve(dev::kCtrlWords));
        RTK_MEM(b.node_bins.reserve(dev::kSortBins));
        RTK_MEM(b.hit_bins.reserve(dev::kSortBins));
        RTK_MEM(b.node_order.reserve(nn));
        RTK_MEM(b.hit_order.reserve(nh));
        w.lane_ws[j] = dev::StreamWs{b.rays.get(), b.nodes.get(), b.hits.get(), b.contrib.get(), w.sumbuf.get(), b.ctrl.get(), uint32_t(nn), uint32_t(nh),
                                     b.node_bins.get(), b.hit_bins.get(), b.node_order.get(), b.hit_order.get()};
        RTK_MEM(w.lane_done[j].ensure());
        for (int par = 0; par < 2; ++par) {
            RTK_MEM(w.lane_side_ev[j].ready[par].ensure());
            RTK_MEM(w.lane_side_ev[j].done[par].ensure());
            w.lane_side[j].ready[par] = w.lane_side_ev[j].ready[par].get(); w.lane_side[j].done[par] = w.lane_side_ev[j].done[par].get();
        }
    }
    RTK_MEM(w.lane_fork.ensure());
    LaneStreams *L = nullptr;                // the process's lane streams (see LaneStreams); the events that order them stay this accel's own
    RTK_HIP(lane_streams_for(device, nlanes, &L));
    for (int j = 0; j < nlanes; ++j) {
        w.lane_stream[j] = L->lane[j];
        w.lane_side[j].stream[0] = L->side[j][0]; w.lane_side[j].stream[1] = L->side[j][1];
    }
    w.ws = w.lane_ws[0];
    w.shape = shape;
    return RTK_OK;
}

// the queues belong to the accel: whoever used them last (a STREAM frame, a batch on another stream) finishes first, on the device
int claim_stream_ws(StreamWorkspace &w, hipStream_t s) { RTK_HIP(w.last.wait_previous(s)); return RTK_OK; }
int release_stream_ws(StreamWorkspace &w, hipStream_t s) { RTK_HIP(w.last.record(s)); return RTK_OK; }

// fork: lane 0 is the caller's stream, the other lanes wait for everything enqueued on it so far
int fork_lanes(StreamWorkspace &w, int lanes, hipStream_t s) {
    if (lanes > 1) RTK_HIP(hipEventRecord(w.lane_fork.get(), s));
    for (int j = 1; j < lanes; ++j) RTK_HIP(hipStreamWaitEvent(w.lane_stream[j], w.lane_fork.get(), 0));
    return RTK_OK;
}
// join: the caller's stream continues behind the last launch of every lane
int join_lanes(StreamWorkspace &w, int lanes, hipStream_t s) {
    for (int j = 1; j < lanes; ++j) RTK_HIP(hipStreamWaitEvent(s, w.lane_done[j].get(), 0));
    return RTK_OK;
}

// ---------------------------------------------------------------- the streaming pipeline's setup, for all of its clients

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

// ---------------------------------------------------------------- a streamed frame

namespace {
// fresh queues: their first use is not what a frame costs -- time the pipeline on the next frame instead
void trial_abandon(rtk_accel *a, hipEvent_t trial[2]) { trial[0] = trial[1] = nullptr; a->trial.abandon(); }
}  // namespace

// (declared with its contract in render_internal.hpp)  `trial[0]` is recorded here, behind the workspace allocation, which is not what a frame costs.
int launch_stream_frame(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const dev::RenderArgs &A, bool forks, bool need_sum,
                        hipEvent_t trial[2], const StreamMoments &M, hipStream_t s) {
    StreamWorkspace &w = a->stream;
    StreamSetup u = stream_args(a, A, p->diffuse_rays, forks);
    const size_t n_root = g.blocks() * 64;
    const size_t nodes_per_sample = n_root * u.factor + 4096;
    const FramePlan plan = plan_frame_batches(g.sample_end - g.sample_begin, nodes_per_sample, u.node_bytes, u.budget,
                                              a->knobs.stream_lanes, a->knobs.stream_batch);
    const int batch = plan.batch, lanes = plan.lanes;
    const StreamWsShape ws_before = w.shape;
    RTK_TRY(ensure_stream_ws(w, a->device, out_pixels(g), nodes_per_sample * size_t(batch), a->scene.lights.size(), need_sum, lanes));
    if (trial && trial[0] && (w.shape.nodes != ws_before.nodes || w.shape.lanes != ws_before.lanes)) trial_abandon(a, trial);
    if (trial && trial[0]) RTK_HIP(hipEventRecord(trial[0], s));
    dev::StreamArgs &S = u.S;
    S.ws = w.ws; S.n_root = uint32_t(n_root); S.n_level0 = uint32_t(n_root);
    // overflow words: a frame is judged on those of all its lanes (unused slots point at lane 0's)
    S.n_lanes = uint32_t(lanes);
    for (int j = 0; j < dev::kStreamLanes; ++j) S.lane_overflow[j] = w.lane_ws[j < lanes ? j : 0].ctrl + dev::kCtrlOverflow;
    RTK_TRY(claim_stream_ws(w, s));
    // ctrl: a frame zeroes all its lanes' on the caller's stream, before the fork
    for (int j = 0; j < lanes; ++j) RTK_HIP(hipMemsetAsync(w.lane_ws[j].ctrl, 0, dev::kCtrlWords * sizeof(uint32_t), s));
    RTK_TRY(fork_lanes(w, lanes, s));
    // side streams: while few SAMPLES are in flight (a radiance batch counts chunks).  They help while few rays are in flight:
    // spp 1 16.7 -> 9.1 ms on config 3; with four lanes the GPU is full already and they cost 20 %
    const bool side = a->knobs.stream_side && lanes <= 2 && batch * lanes <= a->knobs.stream_side_below;
    for (int i = 0; i < plan.n_launch; ++i) {
        const int j = i % lanes;
        S.sample = g.sample_begin + i * batch;
        S.n_batch = uint32_t(g.sample_end - S.sample < batch ? g.sample_end - S.sample : batch);
        S.n_level0 = uint32_t(n_root) * S.n_batch;
        S.ws = w.lane_ws[j];
        const hipStream_t ls = j == 0 ? s : w.lane_stream[j];
        // ordering events: the depth-0 k_combine (and k_frame_moments) of a batch waits for the previous batch's, so the pixel sums
        // and the statistic stay in sample order
        const hipEvent_t wait = (lanes > 1 && i > 0) ? w.lane_done[(i - 1) % lanes].get() : nullptr;
        const hipEvent_t done = lanes > 1 ? w.lane_done[j].get() : nullptr;
        RTK_HIP_AS(launch_stream_sample(S, p->collect_stats != 0, u.deep_level, u.deep_mode, u.sort_from, ls, wait, done,
                                        side ? &w.lane_side[j] : nullptr, u.slices, M), "launch streaming pipeline");
    }
    RTK_TRY(join_lanes(w, lanes, s));
    S.ws = w.ws;
    // the lanes' overflow words folded into lane 0's (the counters of an overflowed frame mean nothing and are zeroed)
    RTK_HIP_AS(launch_stream_overflow_reset(S, s), "launch overflow reset");
    return RTK_OK;
}

int render_stream(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const dev::RenderArgs &A, bool forks, bool general,
                  hipEvent_t trial[2], hipStream_t s) {
    RTK_TRY(launch_stream_frame(a, p, g, A, forks, p->spp > 1, trial, StreamMoments(), s));
    const dev::StreamWs &ws = a->stream.ws;
    // tail: the safety net -- if any queue overflowed, the megakernel renders the frame again (a no-op otherwise)
    dev::RenderArgs F = A;
    F.only_if = ws.ctrl + dev::kCtrlOverflow;
    RTK_HIP_AS(launch_render(F, RTK_TRACE_GROUP4, p->collect_stats != 0, general, s), "launch fallback k_render");
    RTK_TRY(release_stream_ws(a->stream, s));
    if (a->knobs.stream_debug) {
        uint32_t h[dev::kCtrlWords];
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(h, ws.ctrl, sizeof(h), hipMemcpyDeviceToHost);
        std::fprintf(stderr, "[rtk stream] node_cap %u hit_cap %u overflow %u; nodes per level:", ws.node_cap, ws.hit_cap, h[dev::kCtrlOverflow]);
        for (int l = 0; l <= p->max_ray_depth + 1; ++l) std::fprintf(stderr, " %u", l == 0 ? unsigned(g.blocks() * 64) : h[dev::kCtrlNodeCount + l]);
        std::fprintf(stderr, "; hits:");
        for (int l = 0; l <= p->max_ray_depth; ++l) std::fprintf(stderr, " %u", h[dev::kCtrlHitCount + l]);
        std::fprintf(stderr, "\n");
    }
    return RTK_OK;
}

}  // namespace rtk
