// C-ABI, the megakernel's launch order: the cost-feedback tables of a launch with their sort, judge and stamp, and the megakernel
// launch itself.  The decisions are frame_plan.hpp's and order_judge.hpp's; the loop over the launches of a views or regions call
// (render_parts) is a template and so lives in render_internal.hpp.
#include <cstring>
#include <mutex>

#include "render_internal.hpp"

namespace rtk {

namespace {

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

}  // namespace

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

}  // namespace rtk

using namespace rtk;

extern "C" {

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

}  // extern "C"
