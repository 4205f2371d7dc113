// Internal to the host side of the C-ABI (api*.hip), not part of the ABI: an accel's state and what more than one of those files needs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "stream.hpp"
#include "build.hpp"

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
    size_t views_launch_units = 131072;                     // RTK_VIEWS_LAUNCH_UNITS: pixel blocks of one rtk_render_views launch (api_frame.hip; a test lowers it)
    bool traversal_fast = false;                            // RTK_TRAVERSAL_FAST: front-to-back leaf order (rtk.h; NOT the parity mode)

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
        if (geti("RTK_COST_RESORT_EVERY", v) && v > 0) k.resort_every = unsigned(v);
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
        return k;
    }
};

// Per-pixel-block cost of the last frame of shape `sig`, and the launch order made from it.
struct rtk_cost_feedback {
    uint32_t *cost = nullptr, *order = nullptr;
    uint8_t *bins = nullptr;
    size_t units = 0;
    uint64_t sig[5] = {0, 0, 0, 0, 0};
    bool valid = false;              // cost holds the costs of a frame of shape sig
    bool order_valid = false;        // order was made from such costs
    unsigned age = 0;                // frames rendered with the current order
    // number of workgroups in order's workgroup list, read back behind the sort that made it (pinned host word + event)
    uint32_t *nwgs_host = nullptr;
    hipEvent_t nwgs_ev = nullptr;
    bool nwgs_pending = false, nwgs_known = false;

    void forget() { valid = false; order_valid = false; age = 0; nwgs_pending = false; nwgs_known = false; }
    void release() {
        (void)hipFree(cost); (void)hipFree(order); (void)hipFree(bins);
        if (nwgs_ev) (void)hipEventDestroy(nwgs_ev);
        if (nwgs_host) (void)hipHostFree(nwgs_host);
        *this = rtk_cost_feedback();
    }
};

namespace rtk {
enum { G_NODES, G_LEAVES, G_FAST, G_TRIS, G_IDS, G_SHADE, G_LREFS, G_ONODES, G_OLEAVES, G_OTRIS, G_OIDS, kGeomBufs };
// the topology tables of an update (up_index, up_inc_off, up_inc, up_opaque, d_tri_uv), which rtk_accel_update_geometry replaces
enum { T_INDEX, T_INC_OFF, T_INC, T_OPAQUE, T_TRI_UV, kTopoBufs };
}

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
    rtk::DevNode *d_nodes = nullptr;
    rtk::DevNode *d_leaves = nullptr;
    rtk::DevNode *d_leaves_fast = nullptr;    // RTK_TRAVERSAL_FAST: 8 front-to-back orders of the leaves (null in the parity mode)
    rtk::DevTri *d_tris = nullptr;
    uint32_t *d_tri_ids = nullptr;
    rtk::DevShade *d_shade = nullptr;
    rtk::DevMaterial *d_materials = nullptr;
    rtk::DevLight *d_lights = nullptr;
    rtk::DevTexture *d_textures = nullptr;
    rtk::DevTriUv *d_tri_uv = nullptr;
    uint8_t *d_tex_pixels = nullptr;
    unsigned long long *d_counters = nullptr;     // 8 x u64 in rtk_counters order + kRayCounterShards ray-count shards
    // RTK_TRAVERSAL_FAST on a scene with transmissive materials: the tree again with the opaque triangles only (occlusion queries, k_shadow)
    rtk::DevNode *d_occl_nodes = nullptr, *d_occl_leaves = nullptr;
    rtk::DevTri *d_occl_tris = nullptr;
    uint32_t *d_occl_ids = nullptr;
    uint32_t occl_n_leaves = 0;
    bool occl_on = false;
    // ---- ws_* / lane_*: streaming-pipeline workspace (api_frame.hip ensure_stream_ws; grown on demand)
    // one per sample lane (stream.hpp kStreamLanes); `ws` = lane 0; all lanes share lane 0's sumbuf
    rtk::dev::StreamWs ws = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0u, nullptr, nullptr, nullptr, nullptr};
    rtk::dev::StreamWs ws_lane[rtk::dev::kStreamLanes] = {};
    int ws_lanes = 0;
    size_t ws_pixels = 0, ws_lights = 0, ws_nodes = 0;
    bool ws_sum = false;
    hipStream_t lane_stream[rtk::dev::kStreamLanes] = {};
    hipEvent_t lane_done[rtk::dev::kStreamLanes] = {};
    hipEvent_t lane_fork = nullptr;
    rtk::StreamSide lane_side[rtk::dev::kStreamLanes] = {};     // k_shadow side streams of every lane
    // the streaming workspace's last user (a STREAM frame or a radiance batch) recorded ws_done: the next one on any stream waits for it
    hipEvent_t ws_done = nullptr;
    bool ws_in_use = false;
    // ---- tp_*: two-pass workspace (api_frame.hip ensure_twopass_ws)
    float4 *tp_prim = nullptr;
    uint32_t *tp_bins = nullptr;       // [kCostBins] counts, [1] n_listed
    uint32_t *tp_bin_list = nullptr, *tp_order = nullptr;
    size_t tp_pixels = 0, tp_tiles = 0;
    // ---- fb / fb_views: cost feedback (megakernel frames, api_frame.hip render_megakernel).  Frames have one set of tables;
    // rtk_render_views has one per launch of a call (a call is cut into launches of whole views), so that a caller who
    // alternates frames and views calls keeps the order of both.
    rtk_cost_feedback fb;
    std::vector<rtk_cost_feedback> fb_views;
    // ---- views_*: rtk_render_views (api_frame.hip).  The host variant's staging (view table, output) grows and never shrinks.
    float *views_tab = nullptr;
    size_t views_tab_cap = 0;                  // views
    float *views_out = nullptr;
    size_t views_out_cap = 0;                  // floats
    unsigned long long *d_views_counters = nullptr;   // [kCounterWords] the call's totals while its frames / launches run
    // ---- rg_* / fb_regions: rtk_render_regions (api_frame.hip).  One set of cost tables per launch of a call, as for views; they are
    // reused only by a call whose rectangle list, layout and frame width equal the previous call's (rg_rects, rg_layout, rg_width), and
    // then the table on the device is that call's too and is not uploaded again.
    std::vector<rtk_cost_feedback> fb_regions;
    std::vector<rtk_rect> rg_rects;
    rtk::RegionsPlan rg_plan;                  // the plan of rg_rects (regions_plan.hpp): entries and launches
    int rg_layout = -1;
    uint32_t rg_width = 0;
    size_t rg_limit = 0;                       // the launch limit the table on the device was cut with
    rtk::RegionEntry *rg_table = nullptr;      // the entries of all launches of the call, one behind the other
    size_t rg_table_cap = 0;                   // entries
    bool rg_table_valid = false;               // rg_table holds the plan of rg_rects
    hipEvent_t rg_done = nullptr;              // recorded behind a call's last kernel: the next table upload, on any stream, waits for it
    bool rg_in_use = false;
    rtk_ray *rg_rays = nullptr;                // streaming path: rays, frame pixel indices and colours of one chunk of pixels
    uint32_t *rg_ids = nullptr;
    float *rg_rgb = nullptr;
    size_t rg_cap = 0;                         // pixels
    float *rg_out = nullptr;                   // staging of the host variant
    size_t rg_out_cap = 0;                     // floats
    // ---- trial_*: RTK_TRACE_AUTO on forking scenes: which engine is faster for the current shape (api_frame.hip choose_engine)
    hipEvent_t trial_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t trial_sig[3] = {0, 0, 0};
    int trial_state = 0;
    // ---- rp_*: ray repacking workspace (batched intersect: api_batch.hip, repack.hip)
    uint32_t *rp_bounds = nullptr, *rp_keys = nullptr, *rp_idx = nullptr;
    void *rp_temp = nullptr;
    size_t rp_temp_bytes = 0, rp_cap = 0;
    uint32_t *rp_host = nullptr;     // pinned: the probe's words as the host sees them
    hipEvent_t rp_probe_ev = nullptr;
    hipEvent_t rp_done = nullptr;    // recorded behind the k_intersect that walks rp_idx: the next repack on any stream waits for it
    bool rp_in_use = false;
    // ---- oc_*: staging of the host variant of the occlusion batch (rtk_accel_occluded, api_batch.hip): grows, never shrinks
    rtk_ray *oc_rays = nullptr;
    float *oc_max_t = nullptr;
    uint8_t *oc_out = nullptr;
    size_t oc_cap = 0;
    // ---- rad_*: batched radiance (rtk_accel_radiance, api_frame.hip)
    // one kCounterWords block per lane for a chunk's pipeline, then {rays, chunks redone} of the call
    unsigned long long *d_rad_counters = nullptr;
    // staging of the host variant: grows, never shrinks
    rtk_ray *rad_rays = nullptr;
    uint32_t *rad_ids = nullptr;
    float *rad_rgb = nullptr;
    size_t rad_cap = 0;
    // ---- up_*: rtk_accel_update_vertices (api_update.hip, build.hip).  The geometry buffers exist twice: an update builds into
    // the spare set and swaps it with the active one (d_nodes ... d_occl_ids, d_leaf_refs) at the end, so a failed update leaves
    // the accel as it was and a steady animation allocates nothing.  Capacities in bytes; buffers grow, never shrink.
    void *spare[rtk::kGeomBufs] = {};
    size_t spare_cap[rtk::kGeomBufs] = {}, active_cap[rtk::kGeomBufs] = {};
    int32_t *d_leaf_refs = nullptr;            // leaf_refs in reference order, written by the device build
    bool refs_on_device = false;               // tree.leaf_refs (and every per-triangle host array) lives on the device only
    int32_t n_leaf_refs_dev = 0;
    bool up_static = false;                    // the tables of the current topology below are made
    uint32_t *up_index = nullptr, *up_inc_off = nullptr, *up_inc = nullptr;
    uint8_t *up_opaque = nullptr;
    float *up_verts = nullptr;                 // staging of the host variant
    rtk::DevTri *up_tris = nullptr;            // per triangle: scratch of a build, grows with the triangle count
    float *up_tbox = nullptr;
    size_t up_tris_cap = 0, up_tbox_cap = 0;   // bytes
    // ---- topo_*: rtk_accel_update_geometry (api_update.hip, topology.hip).  The topology tables exist twice like the geometry:
    // the new ones are made on the device into the spare set (with d_tri_uv, and mesh / material in the spare shading records)
    // and swapped in with it.  The counts per mesh are numbers: the host arrays they came from are dropped by the updates.
    std::vector<int32_t> mesh_nverts, mesh_ntris;
    void *topo_spare[rtk::kTopoBufs] = {};
    size_t topo_spare_cap[rtk::kTopoBufs] = {}, topo_active_cap[rtk::kTopoBufs] = {};
    rtk::dev::TopoMesh *topo_meshes = nullptr; // [n_meshes + 1] the small per-mesh table of the call in flight
    float *topo_vert_uv = nullptr;             // [n_vertices][2], zero for meshes without uvs; made once, with textures only
    uint32_t *topo_keys = nullptr;             // the sorted vertex ids of the incidence sort
    void *topo_temp = nullptr;                 // rocPRIM's
    size_t topo_keys_cap = 0, topo_temp_cap = 0;
    uint32_t *up_idx_stage = nullptr;          // staging of the host variant's indices
    size_t up_idx_stage_cap = 0;
    uint32_t *up_ref_id = nullptr, *up_ref_node = nullptr;
    size_t up_cap_refs = 0, up_cap_nodes = 0;
    uint8_t *up_table = nullptr, *up_table_host = nullptr;     // BuildHdr + BuildNode[up_cap_nodes]; the host copy is pinned
    rtk::dev::GatherLeaf *up_gather = nullptr;
    size_t up_gather_cap = 0;
    uint8_t *up_stage = nullptr;               // pinned: the small tables on their way up
    size_t up_stage_cap = 0;
    hipEvent_t geom_ready = nullptr;           // recorded behind an update's last kernel: later work on any stream waits for it
    bool geom_pending = false;
    // ---- st_*: rtk_accel_set_lights / _set_materials (api_state.hip; the regather: api_update.hip, occluders.hip)
    size_t lights_cap = 0;                     // rows d_lights has room for; grows with head room, never shrinks
    bool lights_on_device = false;             // rtk_accel_set_lights_device: scene.lights has the COUNT, the values are in d_lights
    rtk::DevMaterial *st_materials = nullptr;  // the spare material table: written, read by the regather, then swapped with d_materials
    rtk::dev::OcclLeaf *st_leaves = nullptr;   // one row per leaf of the active tree
    uint32_t *st_counts = nullptr;             // opaque references per leaf
    size_t st_leaves_cap = 0, st_counts_cap = 0;   // bytes
    // ---- the last frame (rtk_render_last_counters, rtk_render_last_critical_path)
    hipStream_t last_stream = nullptr;
    uint64_t last_primary = 0;
    bool last_stats = false;
};

namespace rtk {

inline int fail(int code, const std::string &msg) { set_error(msg); return code; }

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

template <typename T>
int upload(const std::vector<T> &src, T **dst) {
    *dst = nullptr;
    const size_t bytes = (src.empty() ? 1 : src.size()) * sizeof(T);
    RTK_HIP(hipMalloc(reinterpret_cast<void **>(dst), bytes));
    if (!src.empty()) RTK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
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

struct FrameGeom {
    uint32_t width, height, bucket, tiles_x, tiles_y, n_buckets, blocks_side, buckets_per_rank;
    uint32_t skew_q;                   // kernels.hpp rank_bucket(): 0 = round robin, else tiles_x / world (diagonal deal)
    int rank, world;
    int sample_begin, sample_end;      // this call renders samples [sample_begin, sample_end) (rtk_render_params.sample_begin/_count)
};

// api.hip
// `s`: the stream the caller is about to issue work on.  It waits for the geometry of the last rtk_accel_update_vertices
// (which was built on that call's stream) unless that has completed already.
int ensure_device(rtk_accel *a, hipStream_t s = nullptr);
dev::TreeView tree_view(const rtk_accel *a);
// api_update.hip
int grow_dev(void **p, size_t *cap, size_t need);
int ensure_update_common(rtk_accel *a);
// What follows from a new material table on a RESIDENT accel whose device is idle: the per-triangle opaque flags the updates read,
// and -- when the set of refractive materials changed -- the opaque-only occlusion tree of a RTK_TRAVERSAL_FAST accel, re-made
// from the active tree into the spare buffers and swapped in.  `d_materials`: the new table on the device; a->scene.materials
// and a->has_refractive are still the old ones and stay so on failure.
int remake_occluders(rtk_accel *a, const std::vector<DevMaterial> &materials, const DevMaterial *d_materials, hipStream_t s);
// api_frame.hip
int frame_geom(const rtk_accel *a, const rtk_render_params *p, FrameGeom &g);
int ensure_stream_ws(rtk_accel *a, size_t pixels, size_t nodes, size_t lights, bool need_sum, int lanes);
void free_stream_ws(rtk_accel *a);

}  // namespace rtk
