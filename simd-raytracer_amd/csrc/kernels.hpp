// Kernel argument blocks and launchers shared by kernels.hip and the api*.hip files.
#pragma once

#include <hip/hip_runtime.h>

#include "rtk_internal.hpp"
#include "counters.hpp"

namespace rtk {

constexpr int kMaxRayDepth = 16;                 // frame-stack capacity of the render kernel
constexpr unsigned long long kCriticalMinTicks = 1000;   // blocks shorter than 10 us do not report (one atomic per block would serialise the frame)
constexpr uint32_t kSliceMinTrisDefault = 33;    // GROUP modes: leaves of at least two 64-triangle chunks are cut across the waves
constexpr size_t kMaxNodeLdsBytes = 48 * 1024;   // node arrays up to this size are staged in LDS (1536 nodes)

}  // namespace rtk

#include "trace.hip.hpp"
#include "regions_plan.hpp"

namespace rtk {
namespace dev {

// Which rank renders which bucket (tile/bucket.hpp:7-21's row-major bucket list dealt to GPUs instead of threads).
// Round robin: bucket i -> rank i % world, the i / world-th bucket of that rank.  When a row of buckets is a whole number of
// rounds (tiles_x % world == 0: 3840 / 24 = 160 buckets per row on 8 ranks) round robin hands every rank the same COLUMNS of
// every row, and a rank's share is as uneven as the picture is from left to right (config 5's shape: 32.8 M ... 38.9 M rays per
// rank).  Those frames are dealt diagonally instead: bucket (bx, by) -> rank (bx + by) % world; with q = tiles_x / world buckets
// per rank and row it is that rank's (by * q + bx / world)-th.  skew_q = q selects it (0 = round robin).  Host mirrors:
// api_frame.hip frame_geom / rank_bucket, parallel.py BucketLayout.
__host__ __device__ inline uint32_t rank_bucket(uint32_t rank, uint32_t local, uint32_t world, uint32_t skew_q) {
    if (skew_q == 0u) return rank + local * world;
    const uint32_t by = local / skew_q, m = local % skew_q;
    const uint32_t c0 = (rank + world - by % world) % world;
    return by * (skew_q * world) + c0 + m * world;
}
__host__ __device__ inline void bucket_owner(uint32_t bucket, uint32_t tiles_x, uint32_t world, uint32_t skew_q, uint32_t &rank, uint32_t &local) {
    if (skew_q == 0u) { rank = bucket % world; local = bucket / world; return; }
    const uint32_t bx = bucket % tiles_x, by = bucket / tiles_x;
    rank = (bx + by) % world; local = by * skew_q + bx / world;
}

struct IntersectArgs {
    TreeView tree;
    const rtk_ray *rays;
    rtk_hit *out;
    size_t n;
    const uint32_t *perm;             // lane i takes ray perm[i] and writes hit perm[i] (repack.hip); null = identity
    uint32_t raster_w;                // != 0 (perm == null): the batch is rows of raster_w rays; waves take 8x8 blocks of it (k_raster_probe)
    const uint32_t *verdict;          // non-null: a launch made BEFORE the host knows the probe's verdict (repack.hpp words 15-17, on the
                                      // device): it does nothing if the batch is to be sorted, and takes the raster width from there
    int cull;
    unsigned long long *counters;
};

struct RenderArgs {
    TreeView tree;
    const DevMaterial *materials;
    const DevTexture *textures;       // procedural textures (null / unused when the scene has none)
    const DevTriUv *tri_uv;           // per-triangle uvs, only when the scene has textures
    const uint8_t *tex_pixels;        // RGB bytes of the bitmap textures (DevTexture::bmp), null without them
    const DevLight *lights;
    int n_lights;
    int has_refractive;
    float cam_pos[3];
    float cam_mat[9];
    float background[3];
    uint32_t width, height;
    float aspect;
    float tan_half_fov;               // tanf(float(radians) / 2.0f), render.hpp:55-57
    int spp, max_depth, diffuse_rays;
    int sample_begin, sample_end;     // this pass renders samples [sample_begin, sample_end) of every pixel (progressive accumulation)
    uint32_t seed;
    float shadow_bias, reflection_bias, refraction_bias;
    // bucket sharding
    uint32_t bucket, tiles_x, tiles_y, n_buckets, blocks_per_bucket_side;
    uint32_t buckets_per_rank;
    uint32_t skew_q;                  // rank_bucket(): 0 = buckets dealt round robin, else diagonally with tiles_x / world per rank and row
    int rank, world;
    uint32_t slice_min_tris;          // GROUP modes: smallest leaf that is split across the workgroup's waves
    int compact;                      // 1: out is [buckets_per_rank][bucket][bucket][3]; 0: out is [h][w][3]
    float *out;
    unsigned long long *counters;
    // Non-null (a megakernel frame without statistics, api_frame.hip): the accel's other counter block, kCounterAllocWords words that
    // workgroup 0 of k_render stores zeros to, so that the next frame counts into it without a fill in front (frame_plan.hpp CounterState).
    unsigned long long *zero_next;
    // Never read or written.  It keeps the fields below at the kernel-argument offsets the kernels were tuned at: with them 48 bytes
    // lower the compiler schedules the scalar loads of the arguments differently, and 17 k_render builds (the benchmark's among them)
    // move by 1 to 3 instructions.  With the pad (zero_next took its first word) every field below stays where it was.
    unsigned long long keep_offsets_[5];
    const uint32_t *only_if;          // non-null: the kernel does nothing unless this word is non-zero (overflow fallback)
    // frame-to-frame scheduling feedback (api_order.hip render_megakernel): every pixel block reports what it cost; the next
    // frame of the same shape starts its blocks most-expensive-first (results do not depend on the order)
    uint32_t n_units;                 // pixel blocks (8x8) of this rank = buckets_per_rank * blocks_per_bucket_side^2
    uint32_t *cost_out;               // [n_units] or null
    float width_f, height_f, spp_f, gi_div_f;   // (float)width, height, spp, diffuse_rays + 1: wave-uniform, converted once on the host
                                      // (converted in the kernel they sit in vector registers and are spilled per lane)
    const uint32_t *order_in;         // permutation of the pixel blocks, or null = natural order
    const uint32_t *order_hdr;        // {n_workgroups, n}: see launch_order_by_cost
    const uint32_t *wg_list;          // [n_workgroups] a block id, or 0x80000000 | index into order_in of the first block of a packed workgroup
    int shadow_exit;                  // occlusion queries may stop at the first answering hit (no transmissive material; trace())
    int skip_unlit;                   // occlusion queries whose light contribution is +-0 in every channel are counted but not traced (unlit_query())
    // RTK_TRAVERSAL_FAST on a scene with transmissive materials: `occl` is the tree without the transmissive triangles, and an occlusion
    // query of the streaming pipeline (k_shadow) is ONE any-hit query against it instead of is_occluded's stepping loop (rtk.h)
    int occl_on;
    TreeView occl;
    // rtk_render_views as ONE launch (k_render<..., VIEWS>; api_views.hip render_views_impl / api_order.hip render_megakernel): the launch's units are (view, pixel
    // block) pairs, unit = view * units_per_view + block, and n_units counts them all.  Null / 0 for a frame.
    const float *views;               // [n_views][12] position, matrix (rtk_view), on the device
    uint32_t n_views, units_per_view;
    size_t view_stride;               // floats from one view's output to the next (width * height * 3)
    // rtk_render_regions as ONE launch (k_render<..., REGIONS>; api_regions.hip): the launch's units are (rectangle, 8x8 block) pairs, the
    // blocks anchored at the rectangle's own corner; unit = regions[r].first_unit + block.  Null / 0 for a frame.
    const RegionEntry *regions;       // [n_regions] regions_plan.hpp, on the device; every entry has pixels
    uint32_t n_regions;

    __device__ __forceinline__ size_t out_index(uint32_t local_bucket, uint32_t lx, uint32_t ly, uint32_t px,
                                                uint32_t py) const {
        return compact ? (((size_t)local_bucket * bucket + ly) * bucket + lx) : ((size_t)py * width + px);
    }
};

struct AssembleArgs {
    const float *gathered;
    float *rgb;
    uint32_t width, height, bucket, tiles_x, world, buckets_per_rank, skew_q;
};

}  // namespace dev

hipError_t launch_intersect(const dev::IntersectArgs &A, int mode, bool stats, hipStream_t s);
// n_workgroups (GROUP modes with a workgroup list): how many workgroups the list holds, when the host knows; 0 = one per pixel block
hipError_t launch_render(const dev::RenderArgs &A, int mode, bool stats, bool forks, hipStream_t s, unsigned n_workgroups = 0);
// order[0..n) = the pixel blocks sorted by cost[], most expensive first (one workgroup, counting sort over 256 log-scale bins;
// blocks cheaper than floor_below are not ordered among themselves).  Blocks costlier than light_below (units of 16 cycles;
// 0 = all) get a workgroup each, the rest are packed `pack` to a workgroup; wg_list[0..hdr[0]) = the workgroups by expected
// duration, longest first (see RenderArgs::wg_list); hdr[1] = n
// judge (null, or the table's judge block, order_judge.hpp): `champion` says what becomes of the
// champion's score: cleared (there is no champion), the device time of the frame in front of this launch (from its stamp to now), or left
enum : int { kChampionNone = 0, kChampionScore = 1, kChampionLeave = 2 };
hipError_t launch_order_by_cost(const uint32_t *cost, uint8_t *bins /* [n] scratch */, uint32_t *order, uint32_t *wg_list /* [n] */,
                                uint32_t *hdr /* [2] */, uint32_t n, uint32_t light_below, uint32_t floor_below, uint32_t pack,
                                hipStream_t s, uint32_t *judge = nullptr, int champion = kChampionNone);
// In front of a frame whose list is scored (the last frame of a segment, the first of a challenger): one thread stores the 100 MHz
// device clock into the judge block's stamp.  The kernel behind the frame -- the re-sort or the judge -- reads its own clock and has
// the device time of a frame under the list in use.  (The same store by workgroup 0 of k_render itself costs the lean GROUP4 build
// a spilled VGPR and 8 B of scratch per lane: DESIGN.md 4.3.)
hipError_t launch_stamp(uint32_t *judge, hipStream_t s);
// Behind the first frame of a newly sorted list (the challenger, in `read_set`): one workgroup scores that frame, asks
// order_judge.hpp's rule and, if the champion stays, copies the champion's `words` words (order, header, workgroup list: one run)
// from `other_set` over the challenger's.  `force`: kJudgeByScore, or the verdict to give whatever the scores say.
hipError_t launch_judge_order(uint32_t *judge, uint32_t *read_set, const uint32_t *other_set, uint32_t words, int force, hipStream_t s);
// first frame of a shape: the launch list (order, wg_list, hdr as launch_order_by_cost leaves them) from the camera rays alone:
// blocks whose centre ray hits a reflective / refractive surface, then blocks that enter the tree, then background blocks `pack`
// to a workgroup.  cls [n_units] and scratch [6] are work space.
hipError_t launch_block_prior(const dev::RenderArgs &A, uint8_t *cls, uint32_t *order, uint32_t *wg_list, uint32_t *hdr,
                              uint32_t *scratch, uint32_t pack, hipStream_t s);
// a call made of several frames (the views of a fallback rtk_render_views, the launches of a chunked one): acc[] += cur[] for the
// counts, max for the critical-path words; both [kCounterWords]
hipError_t launch_counters_fold(const unsigned long long *cur, unsigned long long *acc, hipStream_t s);
hipError_t launch_assemble(const dev::AssembleArgs &A, hipStream_t s);
hipError_t launch_camera_rays(const dev::RenderArgs &A, int sample, rtk_ray *d_rays, hipStream_t s);
hipError_t launch_to_rgb8(const float *d_rgb, size_t n, uint8_t *d_out, hipStream_t s);
// the same bytes for the n = width * height * 3 floats of a frame, to any byte address (a texture's slot)
hipError_t launch_frame_to_texels(const float *d_rgb, size_t n, uint8_t *d_out, hipStream_t s);
// The streaming path of rtk_render_regions, per sample and chunk of `n` pixels starting at pixel `first` of the launch's entries
// (RegionEntry::first_pixel order): the camera rays of those pixels at `sample` with their frame pixel indices ...
hipError_t launch_region_rays(const dev::RenderArgs &A, int sample, uint64_t first, uint32_t n, rtk_ray *d_rays, uint32_t *d_ids, hipStream_t s);
// ... and their colours added into A.out: `start` = the pixel's sum starts at +0 (sample 0), `divide` = this is sample spp - 1 of spp > 1
hipError_t launch_region_accumulate(const dev::RenderArgs &A, uint64_t first, uint32_t n, const float *d_rgb, bool start, bool divide, hipStream_t s);
// dst[0] += src[0] (a radiance batch's ray count into the call's counters)
hipError_t launch_add_word(unsigned long long *dst, const unsigned long long *src, hipStream_t s);

}  // namespace rtk
