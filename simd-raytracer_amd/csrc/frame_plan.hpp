// The launch decisions of a frame (api_frame.hip, api_stream.hip, api_order.hip, api_views.hip): which engine RTK_TRACE_AUTO times and picks, when the launch order gets the
// camera-ray prior, is re-sorted and may shorten the launch, how a views call is cut, when the streaming workspace is re-made.
// None of them changes a pixel, so no frame test sees them: tests/cpp/frame_plan_check.cpp pins them.  Plain structs and
// integers, no HIP, no accel, no heap: the launch path asks these, then issues what they say.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/rtk.h"

namespace rtk {

struct FrameGeom {
    uint32_t width, height, bucket, tiles_x, tiles_y, n_buckets, blocks_side, buckets_per_rank;
    uint32_t skew_q;                   // kernels.hpp rank_bucket(): 0 = round robin, else tiles_x / world (diagonal deal)
    int rank, world;
    int sample_begin, sample_end;      // this call renders samples [sample_begin, sample_end) (rtk_render_params.sample_begin/_count)
    uint64_t blocks_of(uint64_t buckets) const { return buckets * blocks_side * blocks_side; }
    size_t blocks() const { return size_t(blocks_of(buckets_per_rank)); }     // 8x8 pixel blocks of this rank's buckets
};

// What the engine trial and the cost tables both key a frame's shape by: width|height, rank|world, spp|depth|gi.
inline void shape_sig(const FrameGeom &g, int spp, int max_ray_depth, int diffuse_rays, uint64_t out[3]) {
    out[0] = (uint64_t(uint32_t(g.width)) << 32) | uint32_t(g.height);
    out[1] = (uint64_t(uint32_t(g.rank)) << 32) | uint32_t(g.world);
    out[2] = (uint64_t(uint32_t(spp)) << 32) | (uint64_t(uint32_t(max_ray_depth)) << 16) | uint32_t(diffuse_rays);
}

// RTK_TRACE_AUTO on a scene whose ray trees fork: both engines are timed on the first frames of a shape -- frame 1 the pipeline,
// frames 2-3 the megakernel (the second one with its cost-feedback order, and timed) -- then the faster one is kept.  The four
// timed events are the caller's: `record` names the pair to record around the engine, verdict() takes what they measured.
// Frames with per-ray statistics, other trace modes and fork-free scenes neither read nor advance this (applies()).
struct EngineTrial {
    enum { kNoRecord = -1, kPipelinePair = 0, kMegakernelPair = 2 };        // first event of the pair
    struct Step { bool stream; int record; };
    uint64_t sig[3] = {0, 0, 0};
    int state = 0;                     // 0-2: the frames above; 3: both timed, events pending; 4: the pipeline won; 5: the megakernel

    static bool applies(int trace_mode, bool forks, bool stats) { return trace_mode == RTK_TRACE_AUTO && forks && !stats; }
    bool same(const uint64_t s[3]) const { return std::memcmp(s, sig, sizeof(sig)) == 0; }
    // both engines of shape `s` are timed: the caller queries its events and, once they have completed, gives the verdict
    bool waiting(const uint64_t s[3]) const { return state == 3 && same(s); }
    void verdict(float t_stream, float t_mega) { state = t_mega < t_stream ? 5 : 4; }     // a tie keeps the pipeline
    // fresh queues: their first use is not what a frame costs -- time the pipeline on the next frame instead
    void abandon() { state = 0; }
    // The engine of this frame.  A new shape starts over, with the trials off too; without trials the pipeline renders every frame.
    Step next(const uint64_t s[3], bool trials_on) {
        if (!same(s)) { std::memcpy(sig, s, sizeof(sig)); state = 0; }
        if (!trials_on) return {true, kNoRecord};
        switch (state) {
            case 0: state = 1; return {true, kPipelinePair};
            case 1: state = 2; return {false, kNoRecord};                    // first megakernel frame: records the block costs
            case 2: state = 3; return {false, kMegakernelPair};
            case 5: return {false, kNoRecord};
            default: return {true, kNoRecord};                               // 3 (waiting for the events), 4 (pipeline won)
        }
    }
};

// The HIP-free half of a set of cost-feedback tables (rtk_cost_feedback): what they hold and how old it is.
struct OrderState {
    // resort_max: the largest number of frames between two sorts.  Above resort_every, the interval doubles with every sort from the
    // shape's third on until it gets there (resort_every 16: sorts at frames 2, 18, 34, 66, 130, ...): the first lists of a shape are
    // made from the costs of its first frames, a list that has been judged against its successors a few times is worth keeping
    // longer (order_judge.hpp).  0, or not above resort_every: every resort_every frames, as before.
    struct Knobs { bool first_frame_prior; unsigned resort_every; unsigned resort_max = 0; };
    // prior: launch k_block_prior (into set 0).  resort: this frame is the first of a new list -- k_order_by_cost is launched in front of
    // it into read_set (sort_front), unless the frame before launched it behind itself.  use_order: give the kernel set read_set's lists.
    // sort_behind: the next frame of this shape starts a new list: launch k_order_by_cost behind this frame's kernel, into write_set.
    // judge: this frame is the first of a list that was sorted behind the frame before (the challenger), and the other set still holds
    // the list that frame ran (the champion): the caller launches the judge behind this frame (order_judge.hpp) and calls rearm_count().
    struct Step { bool prior, resort, use_order, sort_front, sort_behind; int read_set, write_set; bool judge = false; };
    size_t units = 0;                  // capacity of the tables, never shrunk
    uint64_t sig[5] = {0, 0, 0, 0, 0};
    bool valid = false;                // cost holds the costs of a frame of shape sig
    bool order_valid = false;          // order was made from such costs
    unsigned age = 0;                  // frames rendered with the current order
    // the number of workgroups in order's workgroup list is read back behind the sort that made it
    bool nwgs_pending = false, nwgs_known = false;
    // The tables hold two sets of lists (order, header, workgroup list).  A re-sort is launched behind the last frame of the old list,
    // from the costs that frame has just stored, into the set no frame reads; the frame after it changes sets.  It then sits behind a
    // frame instead of in front of one (same stream, same ~50 us every resort_every frames: a caller that looks at a frame as soon as
    // its kernel is done no longer waits for a sort first).  Only a shape's first sort, which has no list to go on with, is in front.
    int set = 0;                       // the set the frames read
    bool presorted = false;            // the other set's list was launched behind the previous frame
    unsigned sorts = 0;                // sorts of this shape since its schedule started over (forget(), another shape)

    void forget() { valid = false; order_valid = false; age = 0; nwgs_pending = false; nwgs_known = false; set = 0; presorted = false; sorts = 0; }

    // The costs have changed under a list that stays in use (lights moved or re-coloured at an equal count: api_state.hip): the
    // intervals start over at resort_every, but nothing is forgotten: the order, the sets and the known count stay.  The call can
    // bring a sort nearer and never puts one off, however often it comes (an animated light calls it before every frame): the
    // list's age stays, and a list already older than resort_every is sorted behind the very next frame, from the costs that
    // frame stores under the new lights.  (A sort already launched behind the previous frame is taken by the next frame as planned.)
    void restart_schedule(unsigned resort_every) {
        sorts = 0;
        if (!presorted && resort_every > 0 && age >= resort_every) age = resort_every - 1;
    }

    // frames the current list is used for
    unsigned interval(const Knobs &k) const {
        uint64_t iv = k.resort_every;
        for (unsigned i = 3; i <= sorts && iv < k.resort_max; ++i) iv *= 2;
        return (k.resort_max > k.resort_every && iv > k.resort_max) ? k.resort_max : unsigned(iv);
    }

    // RTK_TRACE_AUTO for the megakernel: four waves per pixel block when there are enough blocks to fill the chip several times
    // over, eight when there are few (a rank of a sharded frame, a small image: the frame is then as long as its most expensive block).
    // Measured on config 2 (tools/rank_times.py): 32,400 blocks 0.44 ms (GROUP4) vs 0.87 (GROUP8); 4,050 blocks 0.43 vs 0.32.
    // (A views launch counts the blocks of all its views: many small views get the four-wave workgroups.)
    // RTK_TRACE_TWOPASS named an engine that the cost feedback superseded: its frames are GROUP4's.
    static int frame_mode(int trace_mode, size_t n_units, size_t group8_below) {
        if (trace_mode == RTK_TRACE_TWOPASS) return RTK_TRACE_GROUP4;
        return trace_mode != RTK_TRACE_AUTO ? trace_mode : (n_units < group8_below ? RTK_TRACE_GROUP8 : RTK_TRACE_GROUP4);
    }

    // Units the tables must have room for; `units` if they have.  Otherwise they hold nothing any more (units == 0) until the caller
    // has re-made them and stored the capacity.  The first allocation of the frames' tables also covers the scene's own frame
    // size (`native` blocks), so that a small frame rendered first -- a warm-up -- does not leave three allocations, ~0.1 ms, in
    // front of the first full-size frame.
    size_t capacity(size_t n_units, bool is_frame_table, uint64_t native) {
        if (units >= n_units) return units;
        size_t cap = n_units;
        if (is_frame_table && units == 0 && native > cap && native <= (1ull << 24)) cap = size_t(native);
        units = 0; valid = false; order_valid = false;
        return cap;
    }

    // One frame of shape `s`.  The first frame of a shape has no costs to go by: a prior from the camera rays alone stands in
    // for them (GROUP4 only; not with per-ray statistics; a new rectangle list runs in the natural order, k_block_prior maps
    // units through the buckets).  From the second on the order comes from the newest costs, refreshed every few frames only:
    // the sort is one small workgroup whose ~50 us sit between two frames, and an order a few frames old is as good.  A re-sort
    // is launched behind the last frame of the old list into the other set of lists (sort_behind), a shape's first sort in front.
    // A caller whose launches then fail calls forget().
    Step step(const uint64_t s[5], int mode, bool stats, bool regions, const Knobs &k) {
        const bool same_shape = valid && std::memcmp(s, sig, sizeof(sig)) == 0;
        if (!same_shape) { order_valid = false; set = 0; presorted = false; sorts = 0; }
        Step r = {!same_shape && k.first_frame_prior && mode == RTK_TRACE_GROUP4 && !stats && !regions, false, false, false, false, 0, 0, false};
        if (same_shape) {
            r.resort = !order_valid || age >= interval(k);
            // (how many workgroups the new list has is known on the host a frame or two later)
            if (r.resort) {
                r.sort_front = !presorted;
                r.judge = presorted;
                if (presorted) set ^= 1;
                presorted = false;
                order_valid = true; age = 0; nwgs_known = false; nwgs_pending = true;
                sorts += 1;
            }
            age += 1;
            r.sort_behind = age >= interval(k);      // (the next frame of this shape re-sorts: its list is made behind this one)
            presorted = r.sort_behind;
        }
        r.use_order = r.prior || same_shape;
        r.read_set = set; r.write_set = set ^ 1;
        std::memcpy(sig, s, sizeof(sig));
        valid = true;
        return r;
    }

    // A judge has been enqueued behind this frame: it may put the champion's list, of another length, back into the set the frames
    // read, so the length read back behind the sort says nothing any more.  The caller enqueues a fresh read-back behind the judge;
    // until that one is seen complete the launches cover every block again -- a launch shorter than the list would skip blocks.
    void rearm_count() { if (order_valid) { nwgs_pending = true; nwgs_known = false; } }

    // a frame that uses the order: is the read-back of its workgroup count still to be seen complete (one event query)?
    bool awaits_count() const { return order_valid && nwgs_pending; }
    // Workgroups of a launch that uses the order, or 0: the launch covers every block.  Non-zero only with a measured order whose
    // read-back has been seen complete (`ready`: the query's answer), so not on the prior's frame and not before the sort has run.
    unsigned workgroups(bool ready, const uint32_t *host_word) {
        if (!order_valid) return 0;
        if (nwgs_pending && ready) { nwgs_pending = false; nwgs_known = true; }
        return nwgs_known && !nwgs_pending ? *host_word : 0;
    }
};

// The HIP-free half of an accel's two counter blocks (counters.hpp; rtk_accel::d_counters).  A megakernel frame without per-ray
// statistics counts into the current block and its workgroup 0 clears the other one (RenderArgs::zero_next), so the next such frame
// on the same stream finds a zeroed block waiting: it flips the blocks and issues no fill.  What is held: which block is current,
// and whether the other one is known to be zero behind everything enqueued on `stream`.  Every other user of the counters (the
// streaming engine, views, regions, statistics, the batches) fills and uses the current block itself and calls forget(), as does a
// failed call and whatever resets the launch orders (accel.hpp forget_orders): the next frame then fills again.
// A stream is known by its handle: a caller that destroys a stream and creates another must not count on the accel telling them
// apart (rtk.h, rtk_render_frame_device).
// (tests/cpp/counter_state_check.cpp pins the sequences; tests/test_gpu_steady_frames.py renders them.)
struct CounterState {
    struct Step { int current; bool fill, carry; };    // the block to count into; fill it with zeros first; hand the kernel the other one to clear
    int current = 0;
    bool other_zero = false;
    const void *stream = nullptr;

    void forget() { other_zero = false; }
    // behind the order step of a frame's own tables: a frame of a new shape starts the order over, and the counter blocks with it
    void after_order(const OrderState::Step &st) { if (st.prior || !st.use_order) forget(); }
    // One frame on stream `s`.  `carries`: its launch clears the other block (a megakernel frame, no statistics, no only_if).
    Step frame(const void *s, bool carries) {
        const bool flip = carries && other_zero && stream == s;
        if (flip) current ^= 1;
        other_zero = carries; stream = s;
        return {current, !flip, carries};
    }
};

// Units (8x8 pixel blocks of all views) of one views launch are at most `limit`; a call with more is cut into launches of whole views.
struct ViewsLaunches { size_t per_launch, n_parts; };
inline ViewsLaunches views_launches(size_t n, size_t per_view, size_t limit) {
    const size_t per_launch = per_view >= limit ? 1 : limit / per_view;
    return {per_launch, (n + per_launch - 1) / per_launch};
}

// What the streaming workspace has room for.  It is re-made, never shrunk, when a call asks for more of anything.
struct StreamWsShape {
    size_t pixels = 0, nodes = 0, lights = 0;
    int lanes = 0;
    bool sum = false;                  // per-pixel sums of a multi-sample frame
    StreamWsShape asked() const { StreamWsShape r = *this; if (r.lights == 0) r.lights = 1; if (r.lanes < 1) r.lanes = 1; return r; }
    bool covers(const StreamWsShape &request) const {
        const StreamWsShape r = request.asked();
        return r.pixels <= pixels && r.nodes <= nodes && r.lights <= lights && (!r.sum || sum) && r.lanes <= lanes;
    }
    StreamWsShape grown(const StreamWsShape &request) const {
        const StreamWsShape r = request.asked();
        StreamWsShape n;
        n.pixels = r.pixels > pixels ? r.pixels : pixels; n.nodes = r.nodes > nodes ? r.nodes : nodes;
        n.lights = r.lights > lights ? r.lights : lights; n.lanes = r.lanes > lanes ? r.lanes : lanes;
        n.sum = r.sum || sum;
        return n;
    }
    bool refused() const { return nodes > 0xFFFFFFF0ull; }                  // the pipeline's node ids have 32 bits
    static size_t hit_cap(size_t nodes) { return nodes / 2 + 64; }          // every shading point belongs to a distinct node
};

}  // namespace rtk
