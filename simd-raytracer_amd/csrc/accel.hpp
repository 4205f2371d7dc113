// Internal to the host side of the C-ABI (api*.hip), not part of the ABI: an accel's state and what more than one of those files needs.
// Ownership: every device or pinned allocation and every event of an accel is a member of rtk_accel (or of a struct it holds) of
// one of dev_mem.hpp's owning types, over the three memory sources below; they free themselves when the accel is deleted.  A new
// buffer is one field here and one reserve() where it is used.  The structs the kernels take by value (dev::TreeView,
// dev::RenderArgs, dev::StreamWs, StreamSide ...) stay plain and are filled from the owners.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "kernels.hpp"
#include "stream.hpp"
#include "build.hpp"
#include "dev_mem.hpp"
#include "stage_plan.hpp"
#include "frame_plan.hpp"
#include "order_judge.hpp"
#include "update_plan.hpp"

// Environment knobs (all optional).  Read ONCE, when an accel is built: nothing on the launch path
// calls getenv.
struct rtk_knobs {
    uint32_t slice_min_tris = rtk::kSliceMinTrisDefault;   // RTK_SLICE_MIN_TRIS
    bool shadow_exit = true;                                // RTK_SHADOW_EARLY_EXIT
    bool skip_unlit_shadow = true;                          // RTK_SKIP_UNLIT_SHADOW: occlusion queries that cannot change the pixel are not traced
    bool bundle_cull = true;                                // RTK_BUNDLE_CULL
    bool auto_trials = true;                                // RTK_AUTO_TRIALS
    bool cost_feedback = true;                              // RTK_COST_FEEDBACK
    unsigned resort_every = 16;                             // RTK_COST_RESORT_EVERY
    unsigned resort_max = 128;                              // RTK_COST_RESORT_MAX: the interval doubles from a shape's third sort on, up to this (0: never; frame_plan.hpp)
    bool judge = true;                                      // RTK_COST_JUDGE: a newly sorted launch order is kept only if its first frame was not slower (order_judge.hpp)
    int judge_force = rtk::kJudgeByScore;                   // RTK_COST_JUDGE_FORCE: 1 every new order is taken, 2 the champion is always kept (the tests)
    uint32_t light_cycles = 140000u;                        // RTK_LIGHT_BELOW_CYCLES
    uint32_t order_floor_cycles = 20000u;                   // RTK_ORDER_FLOOR_CYCLES
    bool batch_scalar_surv = false;                         // RTK_BATCH_SCALAR_SURV: the same in the batched intersect
    bool stream_scalar_surv = true;                         // RTK_STREAM_SCALAR_SURV: survivors through the scalar cache in the streaming kernels
    bool repack = true;                                     // RTK_REPACK: RTK_TRACE_AUTO may sort large incoherent ray batches
    bool raster_tiles = true;                               // RTK_RASTER_TILES: coherent batches that are rows of camera rays go to the waves as 8x8 blocks
    int repack_skip_bits = 6;                               // RTK_REPACK_SKIP_BITS: low key bits left unsorted when <= 3 dimensions vary (0..14)
    bool repack_full_bounds = false;                        // RTK_REPACK_FULL_BOUNDS: key cells from the bounds of all rays, not of a sample
    int repack_skip_bits2 = 14;                             // RTK_REPACK_SKIP_BITS2: the same when <= 2 dimensions vary (0..22)
    bool repack_dirs3 = false;                              // RTK_REPACK_DIRS3: directions enter the sort keys as three components even when all rays share an origin
    int repack_trace = -1;                                  // RTK_REPACK_TRACE: strategy for a sorted batch (0 auto, 1 lane, 2 wave; default: by the probe)
    size_t group8_below = 9000;                             // RTK_GROUP8_BELOW_BLOCKS
    int stream_node_factor = 0;                             // RTK_STREAM_NODE_FACTOR (0 = default)
    int stream_deep_level = 99, stream_deep_mode = RTK_TRACE_AUTO;   // RTK_STREAM_DEEP_LEVEL / _MODE
    uint32_t auto_min_lanes = 12;                           // RTK_AUTO_MIN_LANES
    int stream_sort_from = -1;                              // RTK_STREAM_SORT_FROM (-1 = default)
    bool stream_debug = false;                              // RTK_STREAM_DEBUG
    bool stream_side = true;                                // RTK_STREAM_SIDE: k_shadow on side streams
    int stream_lanes = 4;                                   // RTK_STREAM_LANES: batches of a frame in flight at once (1..kStreamLanes); 8 measured no faster
    int stream_slices = 0;                                  // RTK_STREAM_SLICES: waves per work unit of the streaming levels (1, 2, 4; 0 = by the tree's leaf sizes)
    int stream_batch = 0;                                   // RTK_STREAM_BATCH: samples traced together per launch (stream.hpp; 0 = the pass split evenly over the lanes)
    int stream_mem_gb = 96;                                 // RTK_STREAM_MEM_GB: budget for the queues of all batches in flight
    int stream_side_below = 2;                              // RTK_STREAM_SIDE_BELOW: k_shadow on side streams while at most this many samples are in flight
    bool first_frame_prior = true;                          // RTK_FIRST_FRAME_PRIOR: launch order of a shape's first frame from k_block_prior
    bool fast_occluders = true;                             // RTK_FAST_OCCLUDERS: RTK_TRAVERSAL_FAST answers occlusion through transmissive surfaces from the opaque triangles alone
    bool camera_keeps_order = false;                        // RTK_CAMERA_KEEPS_ORDER: rtk_accel_set_camera leaves the cost-feedback launch order of the previous camera in place
    size_t views_launch_units = 131072;                     // RTK_VIEWS_LAUNCH_UNITS: pixel blocks of one rtk_render_views launch (api_views.hip; a test lowers it)
    bool traversal_fast = false;                            // RTK_TRAVERSAL_FAST: front-to-back leaf order (rtk.h; NOT the parity mode)
    size_t adaptive_chunk_pixels = size_t(1) << 20;         // RTK_ADAPTIVE_CHUNK_PIXELS: pixels of one chunk of an adaptive round (adaptive_plan.hpp; a test lowers it)

    static rtk_knobs from_env() {
        rtk_knobs k;
        auto geti = [](const char *name, long &out) { const char *e = std::getenv(name); if (!e || !*e) return false; out = std::atol(e); return true; };
        long v;
        if (geti("RTK_SLICE_MIN_TRIS", v) && v > 0) k.slice_min_tris = uint32_t(v);
        if (geti("RTK_SHADOW_EARLY_EXIT", v)) k.shadow_exit = v != 0;
        if (geti("RTK_SKIP_UNLIT_SHADOW", v)) k.skip_unlit_shadow = v != 0;
        if (geti("RTK_BUNDLE_CULL", v)) k.bundle_cull = v != 0;
        if (geti("RTK_AUTO_TRIALS", v)) k.auto_trials = v != 0;
        if (geti("RTK_COST_FEEDBACK", v)) k.cost_feedback = v != 0;
        // (an interval that is asked for is kept as it is asked for: no stretching, unless a cap is asked for as well)
        if (geti("RTK_COST_RESORT_EVERY", v) && v > 0) { k.resort_every = unsigned(v); k.resort_max = 0; }
        if (geti("RTK_COST_RESORT_MAX", v) && v >= 0 && v <= (1l << 30)) k.resort_max = unsigned(v);
        if (geti("RTK_COST_JUDGE", v)) k.judge = v != 0;
        if (geti("RTK_COST_JUDGE_FORCE", v) && v >= rtk::kJudgeByScore && v <= rtk::kJudgeAlwaysKeep) k.judge_force = int(v);
        if (geti("RTK_LIGHT_BELOW_CYCLES", v) && v >= 0) k.light_cycles = uint32_t(v);
        if (geti("RTK_ORDER_FLOOR_CYCLES", v) && v >= 0) k.order_floor_cycles = uint32_t(v);
        if (geti("RTK_REPACK", v)) k.repack = v != 0;
        if (geti("RTK_RASTER_TILES", v)) k.raster_tiles = v != 0;
        if (geti("RTK_REPACK_FULL_BOUNDS", v)) k.repack_full_bounds = v != 0;
        if (geti("RTK_REPACK_SKIP_BITS2", v) && v >= 0 && v <= 22) k.repack_skip_bits2 = int(v);
        if (geti("RTK_REPACK_DIRS3", v)) k.repack_dirs3 = v != 0;
        if (geti("RTK_REPACK_SKIP_BITS", v) && v >= 0 && v <= 14) k.repack_skip_bits = int(v);
        if (geti("RTK_STREAM_SCALAR_SURV", v)) k.stream_scalar_surv = v != 0;
        if (geti("RTK_BATCH_SCALAR_SURV", v)) k.batch_scalar_surv = v != 0;
        if (geti("RTK_REPACK_TRACE", v) && (v == RTK_TRACE_AUTO || v == RTK_TRACE_WAVE || v == RTK_TRACE_LANE)) k.repack_trace = int(v);
        if (geti("RTK_GROUP8_BELOW_BLOCKS", v) && v >= 0) k.group8_below = size_t(v);
        if (geti("RTK_STREAM_NODE_FACTOR", v) && v >= 1) k.stream_node_factor = int(v);
        if (geti("RTK_STREAM_DEEP_LEVEL", v)) k.stream_deep_level = int(v);
        if (geti("RTK_STREAM_DEEP_MODE", v)) k.stream_deep_mode = int(v);
        if (geti("RTK_AUTO_MIN_LANES", v) && v > 0 && v <= 64) k.auto_min_lanes = uint32_t(v);
        if (geti("RTK_STREAM_SORT_FROM", v)) k.stream_sort_from = int(v);
        if (geti("RTK_STREAM_DEBUG", v)) k.stream_debug = v != 0;
        if (geti("RTK_STREAM_SIDE", v)) k.stream_side = v != 0;
        if (geti("RTK_TRAVERSAL_FAST", v)) k.traversal_fast = v != 0;
        if (geti("RTK_FIRST_FRAME_PRIOR", v)) k.first_frame_prior = v != 0;
        if (geti("RTK_STREAM_SLICES", v) && (v == 0 || v == 1 || v == 2 || v == 4)) k.stream_slices = int(v);
        if (geti("RTK_STREAM_BATCH", v) && v >= 0 && v <= 4096) k.stream_batch = int(v);
        if (geti("RTK_STREAM_MEM_GB", v) && v >= 1 && v <= 256) k.stream_mem_gb = int(v);
        if (geti("RTK_FAST_OCCLUDERS", v)) k.fast_occluders = v != 0;
        if (geti("RTK_STREAM_SIDE_BELOW", v) && v >= 0) k.stream_side_below = int(v);
        if (geti("RTK_VIEWS_LAUNCH_UNITS", v) && v >= 1 && v <= (1l << 30)) k.views_launch_units = size_t(v);
        if (geti("RTK_CAMERA_KEEPS_ORDER", v)) k.camera_keeps_order = v != 0;
        if (geti("RTK_STREAM_LANES", v) && v >= 1 && v <= rtk::dev::kStreamLanes) k.stream_lanes = int(v);
        if (geti("RTK_ADAPTIVE_CHUNK_PIXELS", v) && v >= 1 && v <= (1l << 30)) k.adaptive_chunk_pixels = size_t(v);
        return k;
    }
};

namespace rtk {
// The three real memory sources of dev_mem.hpp.  Nothing else in the C-ABI files allocates, frees, or makes an event.
struct DeviceMem {
    static int alloc(void **p, size_t bytes) { return int(hipMalloc(p, bytes)); }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static int alloc(void **p, size_t bytes) { return int(hipHostMalloc(p, bytes, hipHostMallocDefault)); }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <unsigned Flags> struct EventSrc {
    using handle = hipEvent_t;
    static int create(handle *h) { return int(Flags == hipEventDefault ? hipEventCreate(h) : hipEventCreateWithFlags(h, Flags)); }
    static void destroy(handle h) { (void)hipEventDestroy(h); }
};
template <typename T> using DevBuf = Buf<T, DeviceMem>;
template <typename T> using PinBuf = Buf<T, PinnedMem>;
using DevEvent = Event<EventSrc<hipEventDisableTiming>>;
using TimedEvent = Event<EventSrc<hipEventDefault>>;

// What a host variant of the C-ABI stages on the device: the caller's arrays on their way up and the answers on their way down, laid
// out by stage_plan.hpp in ONE buffer.  It grows by grow_bytes and never shrinks; growing frees the old allocation, which waits for
// the device.  Either the call's own (freed when the call returns) or rtk_accel::stage.  Statuses are RTK_MEM's and RTK_HIP's.
class HostStage {
    DevBuf<uint32_t> buf_;
    StageLayout lay_;
    uint32_t *words(int i) const { return lay_.present(i) ? buf_.get() + lay_.off[i] : nullptr; }
public:
    // room for the planes of L; a layout whose bytes are no size_t fails like an allocation that cannot succeed
    int reserve(const StageLayout &L) {
        if (!L.fits()) return int(hipErrorOutOfMemory);
        lay_ = L;
        return buf_.reserve(size_t(L.total), grow_bytes());
    }
    // plane i on the device, null for an absent one
    template <typename T> T *at(int i) const { return reinterpret_cast<T *>(words(i)); }
    // blocking copies of a whole plane; nothing moves for an absent one
    hipError_t upload(int i, const void *src) const {
        return lay_.present(i) ? hipMemcpy(words(i), src, size_t(lay_.bytes[i]), hipMemcpyHostToDevice) : hipSuccess;
    }
    hipError_t download(int i, void *dst) const {
        return lay_.present(i) ? hipMemcpy(dst, words(i), size_t(lay_.bytes[i]), hipMemcpyDeviceToHost) : hipSuccess;
    }
};

// A workspace of the accel that calls on different streams share: its last user recorded `done` behind its last kernel, the next
// user, on any stream, waits for that on the device before it touches the workspace.
struct LastUse {
    DevEvent done;
    bool in_use = false;               // done has been recorded
    hipError_t wait_previous(hipStream_t s) {
        const hipError_t e = static_cast<hipError_t>(done.ensure());
        return e == hipSuccess && in_use ? hipStreamWaitEvent(s, done.get(), 0) : e;
    }
    hipError_t record(hipStream_t s) {
        hipError_t e = static_cast<hipError_t>(done.ensure());
        if (e == hipSuccess) e = hipEventRecord(done.get(), s);
        if (e == hipSuccess) in_use = true;
        return e;
    }
};

// What a call that changes a resident accel on its caller's stream (an update, a regather, set_lights_device) leaves for every
// later call, on whatever stream: the event behind its last kernel or copy, and whether anybody still has to wait for it.
class GeomFence {
    DevEvent ready_;
    bool pending_ = false;
public:
    // entry of a call that rewrites what earlier work, on whatever stream, may still read: the device is idle afterwards.  The
    // event is made here, the first time, so that its creation fails before the call has written anything, in place or beside.
    hipError_t quiesce() {
        hipError_t e = static_cast<hipError_t>(ready_.ensure());
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) pending_ = false;
        return e;
    }
    // behind the last piece of work on `s` of a call that began with quiesce(), and before the call swaps anything in
    hipError_t publish(hipStream_t s) {
        const hipError_t e = hipEventRecord(ready_.get(), s);
        if (e == hipSuccess) pending_ = true;
        return e;
    }
    // `s` is about to read the accel: nothing to do once the event has been seen complete, else `s` waits for it on the device
    hipError_t wait(hipStream_t s) {
        if (!pending_) return hipSuccess;
        if (hipEventQuery(ready_.get()) == hipSuccess) { pending_ = false; return hipSuccess; }
        (void)hipGetLastError();                                            // (hipErrorNotReady is no error of the caller's)
        return hipStreamWaitEvent(s, ready_.get(), 0);
    }
    // the host is about to read what the last publisher wrote
    hipError_t sync_host() const { return ready_.get() ? hipEventSynchronize(ready_.get()) : hipSuccess; }
};

// The geometry of an accel exists twice, as two values of this struct: an update builds into the spare one and swaps it with
// the active one at the end, so a failed update leaves the accel as it was and a steady animation allocates nothing.
struct GeomBufs {
    DevBuf<DevNode> nodes, leaves;
    DevBuf<DevNode> leaves_fast;              // RTK_TRAVERSAL_FAST: 8 front-to-back orders of the leaves (empty in the parity mode)
    DevBuf<DevTri> tris;
    DevBuf<uint32_t> tri_ids;
    DevBuf<DevShade> shade;
    DevBuf<int32_t> leaf_refs;                // leaf_refs in reference order, written by the device build
    // RTK_TRAVERSAL_FAST on a scene with transmissive materials: the tree again with the opaque triangles only (occlusion queries, k_shadow)
    DevBuf<DevNode> occl_nodes, occl_leaves;
    DevBuf<DevTri> occl_tris;
    DevBuf<uint32_t> occl_ids;
    void swap_occl(GeomBufs &o) { occl_nodes.swap(o.occl_nodes); occl_leaves.swap(o.occl_leaves); occl_tris.swap(o.occl_tris); occl_ids.swap(o.occl_ids); }
    void swap(GeomBufs &o, bool fast, bool occl) {
        nodes.swap(o.nodes); leaves.swap(o.leaves); tris.swap(o.tris); tri_ids.swap(o.tri_ids); shade.swap(o.shade); leaf_refs.swap(o.leaf_refs);
        if (fast) leaves_fast.swap(o.leaves_fast);
        if (occl) swap_occl(o);
    }
};
// Likewise the topology tables of an update (vertex ids per triangle, incidence lists, opaque flags, per-triangle uvs), which
// rtk_accel_update_geometry replaces.
struct TopoBufs {
    DevBuf<uint32_t> index, inc_off, inc;
    DevBuf<uint8_t> opaque;
    DevBuf<DevTriUv> tri_uv;
    void swap(TopoBufs &o, bool uv) { index.swap(o.index); inc_off.swap(o.inc_off); inc.swap(o.inc); opaque.swap(o.opaque); if (uv) tri_uv.swap(o.tri_uv); }
};
// the queues of one lane of the streaming pipeline: what a dev::StreamWs points into
struct StreamBufs {
    DevBuf<dev::RayRec> rays;
    DevBuf<dev::NodeRes> nodes;
    DevBuf<dev::HitRec> hits;
    DevBuf<float2> contrib;
    DevBuf<uint32_t> ctrl, node_bins, hit_bins, node_order, hit_order;
    void reset() { rays.reset(); nodes.reset(); hits.reset(); contrib.reset(); ctrl.reset(); node_bins.reset(); hit_bins.reset(); node_order.reset(); hit_order.reset(); }
};
// The streaming pipeline's workspace of an accel (rtk_accel::stream), grown on demand; its operations are api_stream.hip's
// (render_internal.hpp).  One set of queues per sample lane (stream.hpp kStreamLanes); `ws` = lane 0; all lanes share lane 0's
// sumbuf.  bufs / sumbuf own the memory, ws / lane_ws are the views of it that the kernels take by value.
struct StreamWorkspace {
    StreamBufs bufs[dev::kStreamLanes];
    DevBuf<float> sumbuf;
    dev::StreamWs ws = {};
    dev::StreamWs lane_ws[dev::kStreamLanes] = {};
    StreamWsShape shape;                                   // what they have room for (frame_plan.hpp)
    hipStream_t lane_stream[dev::kStreamLanes] = {};       // the process's (api_stream.hip LaneStreams): not freed with an accel
    DevEvent lane_done[dev::kStreamLanes];
    DevEvent lane_fork;
    struct SideEvents { DevEvent ready[2], done[2]; } lane_side_ev[dev::kStreamLanes];
    StreamSide lane_side[dev::kStreamLanes] = {};          // k_shadow side streams of every lane (the process's) and views of lane_side_ev
    LastUse last;                                          // of a STREAM frame or a radiance batch
};
}  // namespace rtk

// Per-pixel-block cost of the last frame of shape `state.sig`, and the launch order made from it.
struct rtk_cost_feedback {
    rtk::DevBuf<uint32_t> cost, order;
    rtk::DevBuf<uint8_t> bins;
    rtk::OrderState state;           // what the tables hold (frame_plan.hpp)
    // number of workgroups in order's workgroup list, read back behind the sort that made it (pinned host word + event)
    rtk::PinBuf<uint32_t> nwgs_host;
    rtk::DevEvent nwgs_ev;
    // [kJudgeWords] order_judge.hpp: the newest frame's stamp, the champion's and the challenger's score, the counts; zeroed when made
    rtk::DevBuf<uint32_t> judge;
    size_t list_units = 0;           // units of the lists as the newest launch laid them out (the header sits behind `list_units` words of order)
    uint64_t sorts = 0, judges = 0;  // k_order_by_cost / k_judge_order launches enqueued for this table so far (rtk_debug_order_judge)

    void forget() { state.forget(); }
};

struct rtk_accel {
    rtk_knobs knobs;
    bool coords_small = false;        // every leaf-reference coordinate is below kBundleLimit: bundle culling cannot overflow
    rtk_scene scene;                  // private copy: the caller may free its scene (kd_tree_simd.hpp:106-107 copies too)
    rtk::HostTree tree;
    rtk_accel_params params;
    bool has_refractive = false;
    bool fast_traversal = false;
    // Streaming pipeline: waves per 64-ray work unit.  Helper waves pay where a ray meets large leaves (hw11/scene8, a
    // triangle reference sits in a leaf of 258 on average: 23.3 ms with three helpers, 36.6 without) and cost where it does not
    // (hw15/scene2, 109: 64.1 ms with, 47.8 without -- the helpers' wave slots are worth more as owners of further units).
    int stream_slices_auto = 4;
    std::mutex mu;
    // ---- device residency (api.hip ensure_device; lazy: built on first compute call so host-only use needs no GPU)
    bool on_device = false;
    int device = -1;
    // the members below free themselves; the body only selects the device they live on (it runs before they are destroyed).  An
    // accel that never reached a device holds nothing and makes no HIP call here.
    ~rtk_accel() { if (device >= 0) (void)hipSetDevice(device); }
    rtk::GeomBufs geom, geom_spare;   // active / spare (api_update.hip)
    rtk::DevBuf<rtk::DevMaterial> d_materials;
    rtk::DevBuf<rtk::DevLight> d_lights;           // its capacity is the rows it has room for: grows with head room, never shrinks
    rtk::DevBuf<rtk::DevTexture> d_textures;
    rtk::DevBuf<uint8_t> d_tex_pixels;
    // [2][kCounterAllocWords] counters.hpp: the block in use (counters_now) and the one a steady frame's kernel clears for the next frame
    rtk::DevBuf<unsigned long long> d_counters;
    rtk::CounterState cnt;                         // which is which (frame_plan.hpp)
    uint64_t counter_fills = 0;                    // fills of the block in use issued so far (rtk_debug_counter_fills)
    uint32_t occl_n_leaves = 0;
    bool occl_on = false;
    // ---- stream: the streaming pipeline's queues, lanes and events (api_stream.hip ensure_stream_ws)
    rtk::StreamWorkspace stream;
    // ---- fb / fb_views: cost feedback (megakernel frames, api_order.hip render_megakernel).  Frames have one set of tables;
    // rtk_render_views has one per launch of a call (a call is cut into launches of whole views), so that a caller who
    // alternates frames and views calls keeps the order of both.
    rtk_cost_feedback fb;
    std::vector<rtk_cost_feedback> fb_views;
    // ---- stage: what the host variants of the calls that take an accel stage on the device (HostStage above), shared by all of them.
    // Invariant: a host variant holds `mu` from its reserve() to its last blocking copy, and no _device variant ever touches the
    // stage; so the planes of one call are never in use when the next call lays out its own, and the accel keeps the largest
    // stage any call needed, not the sum.
    rtk::HostStage stage;
    // ---- views: rtk_render_views (api_views.hip)
    rtk::DevBuf<unsigned long long> d_views_counters;   // [kCounterWords] the call's totals while its frames / launches run
    // ---- rg_* / fb_regions: rtk_render_regions (api_regions.hip).  One set of cost tables per launch of a call, as for views; they are
    // reused only by a call whose rectangle list, layout and frame width equal the previous call's (rg_rects, rg_layout, rg_width), and
    // then the table on the device is that call's too and is not uploaded again.
    std::vector<rtk_cost_feedback> fb_regions;
    std::vector<rtk_rect> rg_rects;
    rtk::RegionsPlan rg_plan;                  // the plan of rg_rects (regions_plan.hpp): entries and launches
    int rg_layout = -1;
    uint32_t rg_width = 0;
    size_t rg_limit = 0;                       // the launch limit the table on the device was cut with
    rtk::DevBuf<rtk::RegionEntry> rg_table;    // the entries of all launches of the call, one behind the other
    bool rg_table_valid = false;               // rg_table holds the plan of rg_rects
    rtk::LastUse rg_last;                      // of rg_table by a call's kernels: the next table upload waits for it
    rtk::DevBuf<rtk_ray> rg_rays;              // streaming path: rays, frame pixel indices and colours of one chunk of pixels
    rtk::DevBuf<uint32_t> rg_ids;
    rtk::DevBuf<float> rg_rgb;
    // ---- ad_*: rtk_render_adaptive (api_adaptive.hip, adaptive.hip).  24 B per pixel of the largest frame so far: the luminance sums,
    // the two lists of active pixels a round reads and writes; beside them the two block lists, the count word with its pinned host
    // copy, and the rays and colours of one chunk.  All grow with head room and never shrink.
    rtk::DevBuf<double> ad_s1, ad_s2;
    rtk::DevBuf<uint32_t> ad_list;             // [2][pixels]
    rtk::DevBuf<uint32_t> ad_blocks;           // [2][blocks]
    rtk::DevBuf<unsigned long long> ad_count;  // adaptive_plan.hpp ad_count_word
    rtk::PinBuf<unsigned long long> ad_count_host;
    rtk::DevBuf<rtk_ray> ad_rays;
    rtk::DevBuf<float> ad_rgb;
    rtk::LastUse ad_last;                      // of the workspace by a call's kernels: a call on another stream waits for it
    // ---- fn_*: rtk_render_frame_noise (api_frame_noise.hip, frame_noise.hip).  Its running sums are ad_s1 / ad_s2, behind ad_last;
    // its own are the pinned word the overflow flag is read back into and the count of redone calls.
    rtk::PinBuf<uint32_t> fn_overflow_host;
    uint64_t noise_fallbacks = 0;              // calls redone through the adaptive path because a queue overflowed (rtk_debug_noise_fallbacks)
    // ---- trial*: RTK_TRACE_AUTO on forking scenes: which engine is faster for the current shape (api_frame.hip choose_engine)
    rtk::TimedEvent trial_ev[4];
    rtk::EngineTrial trial;
    // ---- rp_*: ray repacking workspace (batched intersect: api_batch.hip, repack.hip)
    rtk::DevBuf<uint32_t> rp_bounds, rp_keys, rp_idx;
    rtk::DevBuf<uint8_t> rp_temp;
    size_t rp_temp_bytes = 0;
    rtk::PinBuf<uint32_t> rp_host;   // pinned: the probe's words as the host sees them
    rtk::DevEvent rp_probe_ev;
    rtk::LastUse rp_last;            // of rp_idx by the k_intersect that walks it: the next repack waits for it
    // ---- rad_*: batched radiance (rtk_accel_radiance, api_radiance.hip)
    // one counter block per lane for a chunk's pipeline, then {rays, chunks redone} of the call (counters.hpp)
    rtk::DevBuf<unsigned long long> d_rad_counters;
    // ---- up_*: rtk_accel_update_vertices (api_update.hip, build.hip): scratch of a build; buffers grow, never shrink
    bool refs_on_device = false;               // tree.leaf_refs (and every per-triangle host array) lives on the device only
    int32_t n_leaf_refs_dev = 0;
    bool up_static = false;                    // the tables of the current topology (topo) are made
    rtk::TopoBufs topo, topo_spare;            // active / spare; topo.tri_uv is the scene's from ensure_device on
    rtk::DevBuf<float> up_verts;               // staging of the host variant
    rtk::DevBuf<rtk::DevTri> up_tris;          // per triangle: scratch of a build, grows with the triangle count
    rtk::DevBuf<float> up_tbox;
    // ---- topo_*: rtk_accel_update_geometry (api_update.hip, topology.hip).  The new tables are made on the device into topo_spare
    // (with tri_uv, and mesh / material in the spare shading records) and swapped in with the geometry.  The counts per mesh are
    // numbers: the host arrays they came from are dropped by the updates.
    std::vector<int32_t> mesh_nverts, mesh_ntris;
    rtk::DevBuf<rtk::dev::TopoMesh> topo_meshes;   // [n_meshes + 1] the small per-mesh table of the call in flight
    rtk::DevBuf<float> topo_vert_uv;           // [n_vertices][2], zero for meshes without uvs: the current ones while vert_uv_dev
    rtk::DevBuf<uint32_t> topo_keys;           // the sorted vertex ids of the incidence sort
    rtk::DevBuf<uint8_t> topo_temp;            // rocPRIM's
    rtk::DevBuf<uint32_t> up_idx_stage;        // staging of the host variant's indices
    rtk::DevBuf<uint32_t> up_ref_id, up_ref_node;  // reference lists of a build: their capacity is the build's cap_refs
    rtk::DevBuf<uint8_t> up_table;             // BuildHdr + BuildNode[cap_nodes], sized exactly
    rtk::PinBuf<uint8_t> up_table_host;        // its pinned host copy
    rtk::DevBuf<rtk::dev::GatherLeaf> up_gather;
    rtk::PinBuf<uint8_t> up_stage;             // pinned: the small tables on their way up
    rtk::GeomFence geom_fence;                 // published behind an update's last kernel: later work on any stream waits for it
    // ---- st_*: rtk_accel_set_lights / _set_materials (api_state.hip; the regather: api_update.hip, occluders.hip)
    bool lights_on_device = false;             // rtk_accel_set_lights_device: scene.lights has the COUNT, the values are in d_lights
    rtk::DevBuf<rtk::DevMaterial> st_materials;    // the spare material table: written, read by the regather, then swapped with d_materials
    rtk::DevBuf<rtk::dev::OcclLeaf> st_leaves;     // one row per leaf of the active tree
    rtk::DevBuf<uint32_t> st_counts;           // opaque references per leaf
    // ---- tx_* / vert_uv: textures and uvs of a live accel (api_state.hip).  On the host scene.textures / scene.tex_pixels stay the
    // dense table rtk_scene_create makes; a resident accel keeps every bitmap in a slot of d_tex_pixels, 16-byte aligned once a
    // setter has laid the buffer out, and d_textures holds the slots' offsets.
    struct TexSlot {
        int32_t off = 0;                       // of the texels in d_tex_pixels
        size_t cap = 0;                        // bytes the slot has room for
        bool on_device = false;                // set through a _device call: the host's bytes of this texture are stale
    };
    std::vector<TexSlot> tx_slots;             // one per texture of a resident accel (used by the bitmaps)
    size_t tx_used = 0;                        // bytes of d_tex_pixels handed out
    rtk::DevBuf<rtk::DevTexture> tx_textures;  // the spare table and the spare texel buffer: written, then swapped in
    rtk::DevBuf<uint8_t> tx_pixels;
    std::vector<float> vert_uv;                // [n_vertices][2] of all meshes, zeros for a mesh without uvs; made on first use
    bool vert_uv_made = false;
    bool uvs_on_device = false;                // rtk_accel_set_uvs_device: the values are in topo_vert_uv only
    bool vert_uv_dev = false;                  // topo_vert_uv holds the current uvs
    // ---- the last frame (rtk_render_last_counters, rtk_render_last_critical_path)
    hipStream_t last_stream = nullptr;
    uint64_t last_primary = 0;
    bool last_stats = false;
};

namespace rtk {

inline int fail(int code, const std::string &msg) { set_error(msg); return code; }

// a call that takes no accel (and so never goes through ensure_device) is about to use the device
inline int need_device() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(RTK_ERR_NO_DEVICE, "no usable HIP device (this engine has no CPU path)");
    return RTK_OK;
}

inline int hip_fail(hipError_t e, const char *what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return RTK_ERR_HIP;
}

#define RTK_HIP_AS(call, what)                               \
    do {                                                     \
        const hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hip_fail(e_, what);     \
    } while (0)
#define RTK_HIP(call) RTK_HIP_AS(call, #call)
#define RTK_TRY(call) do { const int rc_ = (call); if (rc_ != RTK_OK) return rc_; } while (0)   // an int status: RTK_OK or the caller's return

#define RTK_MEM(call) RTK_HIP_AS(static_cast<hipError_t>(call), #call)                          // a status of dev_mem.hpp: a reserve(), an ensure()

// `dst` afterwards holds a copy of src (room for one element if src is empty); what a failed earlier attempt left is reused or replaced
template <typename T>
int upload(const std::vector<T> &src, DevBuf<T> &dst) {
    RTK_MEM(dst.reserve(src.empty() ? 1 : src.size()));
    if (src.empty()) return RTK_OK;
    const hipError_t e = hipMemcpy(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) { dst.reset(); return hip_fail(e, "upload"); }
    return RTK_OK;
}

inline bool valid_mode(int m) { return m == RTK_TRACE_AUTO || m == RTK_TRACE_LANE || m == RTK_TRACE_WAVE; }
inline bool valid_batch_mode(int m) { return valid_mode(m) || m == RTK_TRACE_REPACK; }
inline bool valid_frame_mode(int m) { return valid_mode(m) || m == RTK_TRACE_GROUP4 || m == RTK_TRACE_GROUP8 || m == RTK_TRACE_GROUP16 ||
           m == RTK_TRACE_STREAM || m == RTK_TRACE_TWOPASS; }

inline int stream_slices_for(const HostTree &t) {     // rtk_accel.stream_slices_auto, by the size of the leaf a random triangle reference lives in
    double refs = 0.0, sq = 0.0;
    for (const DevNode &l : t.dev_leaves) { refs += double(l.b); sq += double(l.b) * double(l.b); }
    return (refs > 0.0 && sq / refs < 150.0) ? 1 : 4;
}

// whether the ray trees of a frame or batch fork (refraction, diffuse GI) ...
inline bool scene_forks(const rtk_accel *a, int diffuse_rays) { return a->has_refractive || diffuse_rays > 0; }
// ... and whether it needs the general build of the kernels (+ refraction, diffuse GI, textures) and not the lean one
inline bool scene_general(const rtk_accel *a, int diffuse_rays) { return scene_forks(a, diffuse_rays) || !a->scene.textures.empty(); }

// The accel's counter block in use and the other one (frame_plan.hpp CounterState).  Whoever counts into the current block without
// handing a kernel the other one to clear (everything but a steady megakernel frame) fills what it uses itself and calls a->cnt.forget().
inline unsigned long long *counters_now(const rtk_accel *a) { return a->d_counters.get() + size_t(a->cnt.current) * kCounterAllocWords; }
inline unsigned long long *counters_other(const rtk_accel *a) { return a->d_counters.get() + size_t(a->cnt.current ^ 1) * kCounterAllocWords; }

// api.hip
// `s`: the stream the caller is about to issue work on.  It waits for the geometry of the last rtk_accel_update_vertices
// (which was built on that call's stream) unless that has completed already.
int ensure_device(rtk_accel *a, hipStream_t s = nullptr);
dev::TreeView tree_view(const rtk_accel *a);
// What the frames learnt about the scene as it was says nothing about the scene as it is now: the launch orders of frames, views
// and regions start over, and so does RTK_TRACE_AUTO's engine trial.  `keep`: what the caller's change leaves valid.
enum : unsigned { kKeepViewOrders = 1u, kKeepTrial = 2u };
inline void forget_orders(rtk_accel *a, unsigned keep = 0u) {
    a->fb.forget();
    a->cnt.forget();                  // (with the frames' order: the next frame fills its counters itself)
    if (!(keep & kKeepViewOrders)) for (rtk_cost_feedback &f : a->fb_views) f.forget();
    for (rtk_cost_feedback &f : a->fb_regions) f.forget();
    if (!(keep & kKeepTrial)) a->trial.abandon();
}

// The blocks' costs have changed but the picture's silhouettes have not: the orders stay, their re-sort schedules start over.
inline void restart_order_schedules(rtk_accel *a) {
    const unsigned every = a->knobs.resort_every;
    a->fb.state.restart_schedule(every);
    for (rtk_cost_feedback &f : a->fb_views) f.state.restart_schedule(every);
    for (rtk_cost_feedback &f : a->fb_regions) f.state.restart_schedule(every);
}

// api_update.hip
// What follows from a new material table on a RESIDENT accel whose device is idle: the per-triangle opaque flags the updates read,
// and -- when the set of refractive materials changed -- the opaque-only occlusion tree of a RTK_TRAVERSAL_FAST accel, re-made
// from the active tree into the spare buffers and swapped in.  `d_materials`: the new table on the device; a->scene.materials
// and a->has_refractive are still the old ones and stay so on failure.
int remake_occluders(rtk_accel *a, const std::vector<DevMaterial> &materials, const DevMaterial *d_materials, hipStream_t s);
// The topology tables of the scene the accel was built from, on the device (topo): made once, on the first call that needs them.
int ensure_update_static(rtk_accel *a);
// api_state.hip
// the slots of a dense texel upload (ensure_device), the per-vertex uvs on the host, and the same on the device (topo_vert_uv)
void dense_texture_slots(rtk_accel *a);
const std::vector<float> &host_vert_uv(rtk_accel *a);
int ensure_vert_uv_dev(rtk_accel *a);

}  // namespace rtk
