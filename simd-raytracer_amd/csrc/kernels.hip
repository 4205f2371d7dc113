// HIP kernels for gfx950: batched closest-hit intersect, the device-side render loop
// (render_frame / color_hit / is_occluded of render/render.hpp), and the multi-GPU bucket assembly.
// One ray per lane, 256-thread workgroups (4 wave64), kd-tree nodes staged in LDS.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "order_judge.hpp"
#include "trace.hip.hpp"
#include "shade.hip.hpp"

namespace rtk {
namespace dev {

// ------------------------------------------------------------------------------------------------
// accel.intersect<cull>(ray) for a batch (kd_tree_simd.hpp:187-264): lane i takes ray i.
template <int MODE, bool STATS, bool LDS_NODES>
__global__ __launch_bounds__(256) void k_intersect(IntersectArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevNode *lds_nodes = reinterpret_cast<DevNode *>(smem);
    if (LDS_NODES) stage_nodes(A.tree.nodes, A.tree.n_nodes, lds_nodes);

    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = slot < A.n;
    size_t i = (active && A.perm != nullptr) ? (size_t)A.perm[slot] : slot;            // repacked batches: the ray this slot was dealt
    uint32_t raster_w = A.raster_w;
    if (A.verdict != nullptr) {                                                        // (wave-uniform scalar loads)
        if (A.verdict[16] != 0u) return;                                               // to be sorted: the host launches again
        raster_w = A.verdict[15];
        if (raster_w < 64u || (raster_w & 7u) != 0u || (size_t)raster_w * 16u > A.n) raster_w = 0u;
    }
    if (raster_w != 0u) {
        // a raster of rows: bands of 8 rows are dealt as 8x8 blocks, one per wave; what is left over after the last whole band stays as it is
        const size_t band = (size_t)raster_w * 8u;
        const size_t tiled = (A.n / band) * band;
        if (slot < tiled) {
            const size_t b = slot / band;
            const uint32_t within = (uint32_t)(slot % band), tile = within >> 6, l = within & 63u;
            i = (b * 8u + (l >> 3)) * (size_t)raster_w + (size_t)tile * 8u + (l & 7u);
        }
    }
    Ray r;
    if (active) {
        const float *p = reinterpret_cast<const float *>(A.rays + i);
        r = make_ray(mk(p[0], p[1], p[2]), mk(p[3], p[4], p[5]));
    } else {
        r = make_ray(mk(0.f, 0.f, 0.f), mk(1.f, 1.f, 1.f));
    }
    Stats st = {0, 0, 0, 0, 0, 0};
    __shared__ __attribute__((aligned(16))) float wave_bundles[4][kMaxBundles * kBundleFloats];
    SliceCtx sx = {nullptr, 0u, 0u, true, 0u, wave_bundles[(threadIdx.x >> 6) & 3u]};
    const Cand c = trace<MODE, STATS, LDS_NODES>(A.tree, lds_nodes, r, A.cull != 0, active, st, sx);
    if (active) {
        float4 o0, o1;
        if (c.k != kMiss) {
            const Surface s = reconstruct(A.tree, c);
            o0 = make_float4(c.t, c.u, c.v, __uint_as_float(s.tri));
            o1 = make_float4(__uint_as_float(s.mesh), s.hit_normal.x, s.hit_normal.y, s.hit_normal.z);
        } else {
            o0 = make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kMiss));
            o1 = make_float4(__uint_as_float(kMiss), 0.0f, 0.0f, 0.0f);
        }
        float4 *out = reinterpret_cast<float4 *>(A.out + i);
        out[0] = o0;
        out[1] = o1;
    }
    if (STATS) flush_stats(st, active ? 1u : 0u, A.counters);
}

// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// Device-side render loop.  One lane = one pixel; a wave = an 8x8 pixel block of a bucket, buckets are
// dealt to ranks round-robin (bucket i -> rank i % world).  color_hit's recursion (render.hpp:133-308) is
// run as a per-lane state machine around ONE wave-wide trace call per iteration; refractive forks and
// diffuse-GI parents keep their partial results in a small per-lane frame stack, evaluated in the same
// order as the recursion so the floating-point results are identical.

// "Light burst": the occlusion queries of a diffuse hit towards its lights (render.hpp:184-206) are independent of each other.
// When every lane that is about to query a light is at the SAME light k, the owner posts GROUP_EXTRA and each helper wave
// traces the whole query of one further light (k + 1, k + 2, ...) on its own -- a single-class pencil bundle per wave, no
// slicing -- while the owner traces light k (and whatever other rays its lanes have pending).  The owner then adds the
// contributions in light order, so the float sums are those of the sequential loop.  Four dependent traces become one step.
// Scenes with transmissive materials keep the sequential loop (a query there may need several segments).
// The lanes of a burst are dealt to 1, 2 or 4 jobs per light by WHERE their rays go (the widest axis of their directions cut
// at its middle, the halves once more): a job's time is set by the triangles inside the cone of its rays, so two jobs that
// each take every other row of the pixel block would each cost as much as the whole (measured), two halves of the cone half.
// (Halves of equal extent, not of equal counts: a half with a few far-out rays has the whole cone again -- measured too.)
// Every wave computes the same partition from the same rays.
__device__ __forceinline__ bool upper_half(const V3 d, const bool sel) {
    Ray q;
    q.o = d; q.d = d; q.inv = d;                                            // (only q.d is read)
    const DirSpread S = dir_spread(q, sel);
    const float dv = S.axis == 0u ? d.x : (S.axis == 1u ? d.y : d.z);
    return sel & !(dv <= S.mid);
}
__device__ __forceinline__ uint32_t burst_part(const V3 d, const bool in, const uint32_t plog) {
    uint32_t part = 0u;
    if (plog == 0u) return part;
    if (upper_half(d, in)) part = 1u;
    if (plog >= 2u) {
#pragma unroll
        for (uint32_t h = 0u; h < 2u; ++h)
            if (upper_half(d, in & (part == h))) part |= 2u;
    }
    return part;
}

template <int SLICES>
struct ShadowBurstService {
    const RenderArgs &A;
    float4 *res;             // [jobs][64] answers: contribution, clear, flags (bit 0: a ray was asked for (counted); bit 1: this job answers for the lane)
    // Jobs (light, part) are handed out through a counter in LDS: a wave that is done takes the next one, so unequal jobs
    // (one half of a cone over the mesh, the other past it) even out.  Job 0 is the owner's own.
    __device__ __forceinline__ void operator()(GroupShared *sh, const uint32_t slice) const {
        const uint32_t lane = __lane_id();
        const uint32_t hdr = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh->count);
        const uint32_t plog = hdr & 0xFFu, n_jobs = hdr >> 8;                                   // log2(parts); lights x parts
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh->first);
        const unsigned long long mask = sh->pass_mask;
        const float4 a = sh->ray_o[lane], b = sh->ray_d[lane];
        const V3 P = mk(a.x, a.y, a.z), ncos = mk(a.w, b.x, b.y);
        const bool in_burst = ((mask >> lane) & 1ull) != 0ull;
        for (;;) {
            uint32_t job = 0u;
            if (lane == 0u) job = atomicAdd(&sh->pad[0], 1u);
            job = (uint32_t)__builtin_amdgcn_readfirstlane((int)job);
            if (job >= n_jobs) break;
            const uint32_t k = first + (job >> plog);                        // this job's light (< n_lights: the owner counted the jobs)
            const uint32_t part = job & ((1u << plog) - 1u);
            const DevLight *L = A.lights + k;                                // wave-uniform
            const V3 lp = mk(L->pos[0], L->pos[1], L->pos[2]);
            const LightTerm lt = light_term(L, P, ncos);
            const V3 ld = lt.dir;
            const float radius = lt.radius, contrib = lt.contrib;
            const bool mine = in_burst & (burst_part(ld, in_burst, plog) == part);
            const bool asked = mine & (0.0f < radius);                       // is_occluded's loop guard, render.hpp:114
            // counted, not traced, when it cannot light the lane (unlit_query(); b.z = the lane's albedo_reach).  A job none of
            // whose lanes is lit ends in trace() before any bundle is made.
            const bool q = asked & !(A.skip_unlit != 0 && unlit_query(contrib, b.z));
            const Ray ray = make_ray(P + (A.shadow_bias * ld), ld);
            Stats st = {0, 0, 0, 0, 0, 0};
            SliceCtx sx = {nullptr, 0xFFFFFFFFu, 0u, true, 0u, group_private_bundles<SLICES>(sh, slice)};
            const float exit_t = A.shadow_exit ? radius : -1.0f;
            const Cand c = trace<RTK_TRACE_WAVE, false, false, 1>(A.tree, nullptr, ray, false, q, st, sx, kAutoMinLanes, exit_t,
                                                                  kClsHasApex | (0x100u + k), lp);
            bool clear = true;
            uint32_t fl = mine ? 2u : 0u;
            if (asked) fl |= 1u;
            if (q) clear = (c.k == kMiss) | (radius < c.t);                  // render.hpp:117
            res[job * 64u + lane] = make_float4(contrib, clear ? 1.0f : 0.0f, __uint_as_float(fl), 0.0f);
        }
    }
};

// The lane index, computed where it is asked for.  From threadIdx / __lane_id() the compiler derives a dozen per-lane
// constants in the kernel's prologue (pixel coordinates as floats, the pixel's RNG hash, its output address, one LDS
// address per array and stride, 1 << lane as a 64-bit pair ...), keeps them across the traversal loops and, out of registers
// there, spills every one of them to scratch right away: 22 dwords per lane written by each of a frame's 32,400 owner waves,
// 180 MB of HBM traffic per launch.  An `asm volatile` is opaque and is not hoisted: two instructions at each use instead.
__device__ __forceinline__ uint32_t fresh_lane() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// a ray whose inv_direction is filled in by k_render right before the query (see there)
__device__ __forceinline__ Ray spawn_ray(const V3 o, const V3 d) {
    Ray r;
    r.o = o; r.d = d; r.inv = d;
    return r;
}

// An entry of a regions launch's table, through the scalar cache (trace.hip.hpp "Wave-uniform loads": as plain global loads the
// compiler fetched the entry per lane, and the block's corner then lived in -- and was spilled from -- vector registers).
typedef const RegionEntry __attribute__((address_space(4))) *cptr_region;
__device__ __forceinline__ cptr_region region_entry(const RegionEntry *table, const uint32_t r) {
    return (cptr_region)(const void __attribute__((address_space(4))) *)(table + r);
}

enum : int { ST_NEW_SAMPLE = 0, ST_TRACE, ST_SHADE, ST_LIGHT, ST_RETURN, ST_DONE };
enum : int { PEND_CHILD_BG = 0, PEND_CHILD_BLACK = 1, PEND_SHADOW = 2 };
enum : uint32_t { FR_REFR_A = 0, FR_REFR_B = 1, FR_DIFFUSE = 2 };

struct Frame {            // 15 dwords, lives in scratch; touched only at refractive / GI events
    float a[12];
    uint32_t meta;        // kind | depth << 8 | iteration << 16
    uint32_t tri;
    uint32_t key;         // RNG key of the ray whose hit this frame shades
};

template <int MODE, bool STATS, bool FORKS, bool LDS_NODES, int SLICES, bool VIEWS = false, bool REGIONS = false>
// GROUP4 without per-ray statistics is built for RTK_G4_WAVES (5) waves per SIMD = 96 VGPRs: a fifth resident workgroup per CU.
// The lean build (FORKS = false) fits with its cold state parked in LDS (`park_lds`); 4 waves / 128 VGPRs and 6 / 80 are slower.
__global__ __launch_bounds__(SLICES > 1 ? 64 * SLICES : 256, SLICES == 16 ? 1 : SLICES == 8 ? 2 : (SLICES == 4 && !STATS ? RTK_G4_WAVES : 4)) void k_render(RenderArgs A) {
    FrameProbe phases = FrameProbe::enter();                     // diagnostic build only (phases.hip.hpp); empty in the product
    if (A.only_if != nullptr && *A.only_if == 0u) return;        // fallback launch behind the streaming pipeline: nothing overflowed
    // the counters of the NEXT frame start at zero: nothing else touches that block while this launch runs (frame_plan.hpp CounterState)
    if (A.zero_next != nullptr && blockIdx.x == 0u && threadIdx.x < (uint32_t)kCounterAllocWords) A.zero_next[threadIdx.x] = 0ull;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevNode *lds_nodes = reinterpret_cast<DevNode *>(smem);
    // the per-lane path reads nodes from LDS; the wave-cooperative paths fetch them with scalar loads instead
    constexpr bool kStage = LDS_NODES && (MODE == RTK_TRACE_LANE || MODE == RTK_TRACE_AUTO);
    if (kStage) stage_nodes(A.tree.nodes, A.tree.n_nodes, lds_nodes);
    __shared__ GroupStorage<(SLICES > 1 ? SLICES : 1)> group_st;
    GroupShared *const group_sh = group_st.get();
    // the wave index is wave-uniform: say so (readfirstlane) or everything derived from it is compiled per-lane
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // The owner role rotates with the workgroup index: the dispatcher places wave i of every workgroup on SIMD i, so a
    // fixed owner wave would put every owner of a CU on the same SIMD and leave the other three to the (mostly idle) helpers.
    uint32_t slice = SLICES > 1 ? (wave_in_wg + blockIdx.x) % (uint32_t)SLICES : 0u;
    // ---- which 8x8 pixel block (tile/bucket.hpp:7-21 buckets, 8x8 blocks inside, round-robin over ranks).
    // SLICES > 1: the whole workgroup serves ONE block (one wave owns the rays, the others help with big leaves) -- except
    // for the blocks the cost feedback found cheap (background, a few nodes): those are packed SLICES to a workgroup,
    // every wave renders its own and nobody helps ("light" workgroups; they never touch the barrier protocol).
    // (Cutting the most expensive blocks into 4x4-pixel quadrants was tried and dropped: a quadrant's rays visit the same
    // leaves as the whole block's, so it cost as much as the block.)
    uint32_t gwave;
    bool light = false;
    if (SLICES > 1 && A.order_in != nullptr) {
        const uint32_t n_wgs = A.order_hdr[0], n_total = A.order_hdr[1];
        if (blockIdx.x >= n_wgs) return;
        const uint32_t desc = A.wg_list[blockIdx.x];                        // k_order_by_cost: workgroups by expected duration
        if ((desc >> 31) == 0u) {
            gwave = desc;
        } else {
            const uint32_t idx = (desc & 0x7FFFFFFFu) + wave_in_wg;
            if (idx >= n_total) return;
            gwave = A.order_in[idx];
            light = true;
            slice = 0u;
        }
    } else {
        const uint32_t unit = SLICES > 1 ? blockIdx.x : blockIdx.x * (blockDim.x >> 6) + wave_in_wg;
        gwave = (A.order_in != nullptr && unit < A.n_units) ? A.order_in[unit] : unit;
    }
    // VIEWS (rtk_render_views as one launch): the units in the lists above are (view, pixel block) pairs.  The view belongs to the
    // WAVE's unit, never to the workgroup: the four blocks of a light workgroup may come from four views.  It is wave-uniform
    // (gwave is), so the camera is fetched through the scalar cache like a node, and the output pointer is a scalar add.  Only the
    // view's number is kept: the two pointers are made where they are used (a camera ray, the pixel's store), four scalar registers
    // less across the traversal.
    uint32_t block = gwave, view = 0u;
    if constexpr (VIEWS) {
        view = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gwave / A.units_per_view));
        if (view >= A.n_views) return;                   // purely defensive: launch_render refuses a launch whose units are not n_views x units_per_view
        block = gwave - view * A.units_per_view;
    }
    // REGIONS (rtk_render_regions as one launch): the units are (rectangle, 8x8 block) pairs, the blocks anchored at the rectangle's own
    // corner.  The rectangle belongs to the WAVE's unit, as a view does, and is found wave-uniformly: a binary search over the
    // entries' first_unit with scalar loads (gwave is wave-uniform; 17 steps for 65,536 rectangles, once per block).  Only its
    // number is kept; the entry is read again through the scalar cache where a pixel is stored.
    uint32_t rect = 0u;
    if constexpr (REGIONS) {
        const uint32_t unit = (uint32_t)__builtin_amdgcn_readfirstlane((int)gwave);
        if (unit >= A.n_units || A.n_regions == 0u) return;      // purely defensive: launch_render refuses a launch without units or entries
        uint32_t lo = 0u, hi = A.n_regions;                      // regions[lo].first_unit <= unit < regions[hi].first_unit (or hi == n)
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (region_entry(A.regions, mid)->first_unit <= unit) lo = mid; else hi = mid;
        }
        rect = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
        block = unit - region_entry(A.regions, rect)->first_unit;
    }
    const auto view_out = [&]() { return VIEWS ? A.out + (size_t)view * A.view_stride : A.out; };
    // one parking area per wave that can own rays: every wave of a light or SLICES == 1 workgroup, one otherwise -- the
    // others then hold the answers of a light burst's jobs (ShadowBurstService)
    constexpr int kParkSlots = 4;                        // light workgroups exist for SLICES == 4 only (api_order.hip)
    __shared__ __attribute__((aligned(16))) float park_lds[kParkSlots][18][64];
    float4 *const burst_res = reinterpret_cast<float4 *>(&park_lds[1][0][0]);
    // one job per wave: twice as many, handed out as waves fall idle, came out slower (each job pays its own ray setup,
    // bundles and leaf-list pass, and the owner only ever traces job 0): config 2 0.21 -> 0.255 ms, one rank of eight 0.155 -> 0.18
    constexpr uint32_t kBurstMaxJobs = SLICES > 8 ? 8u : SLICES > 1 ? (uint32_t)SLICES : 1u;
    static_assert(SLICES <= 1 || (size_t)kBurstMaxJobs * 64 * sizeof(float4) <= sizeof(float) * (kParkSlots - 1) * 18 * 64, "burst answers fit the spare parking slots");
    if (SLICES > 1 && slice != 0u) {                 // helper waves (trace.hip.hpp, "Workgroup-cooperative leaves")
        group_helper_loop<SLICES>(A.tree, group_sh, slice, ShadowBurstService<SLICES>{A, burst_res});
        return;
    }
    // bundles of the current trace (trace.hip.hpp "Bundle culling"): in the group's shared block when helpers must see them,
    // wave-private otherwise (light workgroups and SLICES == 1 have one owner per wave)
    __shared__ __attribute__((aligned(16))) float wave_bundles[4][kMaxBundles * kBundleFloats];
    SliceCtx sx = {SLICES > 1 ? group_sh : nullptr, light ? 0xFFFFFFFFu : A.slice_min_tris, 0u, true, 0u,
                   (SLICES > 1 && !light) ? group_sh->bundles : wave_bundles[wave_in_wg & 3u]};
    const uint32_t park_slot = (SLICES > 1 && !light) ? 0u : (wave_in_wg & 3u);
    const unsigned long long cost_t0 = __builtin_readcyclecounter();
    const unsigned long long real_t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz, for the frame's critical path (bench.py)
    constexpr bool writer = true;
    // (block_map() / block_pixel() written out: through them the benchmark's kernel loses its register allocation)
    uint32_t local_bucket, bx, by, sub_x0, sub_y0;
    bool valid;
    if constexpr (REGIONS) {
        // the block's corner in the frame: the pixels, their RNG keys and camera rays below are the frame's own (px, py, width, height)
        const cptr_region R = region_entry(A.regions, rect);
        const uint32_t blocks_x = ((uint32_t)R->w + 7u) >> 3;
        const uint32_t row = block / blocks_x;
        local_bucket = 0u; sub_x0 = 0u; sub_y0 = 0u;
        bx = (uint32_t)R->x0 + (block - row * blocks_x) * 8u; by = (uint32_t)R->y0 + row * 8u;
        valid = true;
    } else {
    const uint32_t bpb = A.blocks_per_bucket_side * A.blocks_per_bucket_side;
    local_bucket = block / bpb;
    const uint32_t sub = block % bpb;
    const uint32_t bucket = rank_bucket((uint32_t)A.rank, local_bucket, (uint32_t)A.world, A.skew_q);
    valid = bucket < A.n_buckets;
    bx = (bucket % A.tiles_x) * A.bucket; by = (bucket / A.tiles_x) * A.bucket;
    sub_x0 = (sub % A.blocks_per_bucket_side) * 8u; sub_y0 = (sub / A.blocks_per_bucket_side) * 8u;   // wave-uniform
    }
    // this lane's pixel: recomputed where it is needed (see fresh_lane) instead of living in registers across the traversal
    const auto my_pixel = [&]() {
        const uint32_t l = fresh_lane();
        Pixel p;
        p.lx = sub_x0 + (l & 7u); p.ly = sub_y0 + (l >> 3);
        p.px = bx + p.lx; p.py = by + p.ly;
        return p;
    };
    // where that pixel lives in the output, in pixels (REGIONS: the entry says, so the kernel does not know the two layouts apart)
    const auto pixel_slot = [&](const Pixel &p) -> size_t {
        if constexpr (REGIONS) {
            const cptr_region R = region_entry(A.regions, rect);
            return (size_t)(R->base + (long long)p.py * (long long)R->pitch + (long long)p.px);
        } else {
            return A.out_index(local_bucket, p.lx, p.ly, p.px, p.py);
        }
    };
    {
        const Pixel p = my_pixel();
        if constexpr (REGIONS) {
            const cptr_region R = region_entry(A.regions, rect);
            valid = (p.px < (uint32_t)(R->x0 + R->w)) & (p.py < (uint32_t)(R->y0 + R->h));
        } else {
        valid = valid & (p.lx < A.bucket) & (p.ly < A.bucket) & (p.px < A.width) & (p.py < A.height);
        }
    }

    phases.prologue_done();
    const V3 background = mk(A.background[0], A.background[1], A.background[2]);
    const V3 black = mk(0.f, 0.f, 0.f);
    const uint32_t seed_hash = pcg_hash(A.seed);

    // ---- per-lane path state
    int state = valid ? ST_NEW_SAMPLE : ST_DONE;
    int pend = PEND_CHILD_BG;
    int sample = A.sample_begin, depth = 0, light_k = 0;
    uint32_t rkey = 0;                    // RNG key of the ray in flight (position in the sample's ray tree)
    uint32_t nrays_wave = 0;              // rays of the whole wave so far (wave-uniform: a scalar, not a register per lane)
    bool cull = false;
    Ray ray = spawn_ray(black, mk(1.f, 1.f, 1.f));
    V3 pixel_sum = black, ret = black;
    if (A.sample_begin > 0 && valid) {                                     // a later pass of a progressive frame: the running sum so far
        const Pixel p = my_pixel();
        const float *o = view_out() + pixel_slot(p) * 3;
        pixel_sum = mk(o[0], o[1], o[2]);
    }
    // hit being shaded / lit
    V3 P = black, hn = black, fn = black, din = black, ncos = black, acc = black, albedo = black;
    uint32_t hit_tri = 0, hit_mat = 0;
    float shadow_max_t = 0.f, contrib = 0.f;
    bool lit_textured = false;
    Frame frames[FORKS ? kMaxRayDepth : 1];
    int fsp = 0;
    Stats st = {0, 0, 0, 0, 0, 0};
    Cand cand;
    cand.t = kFltMax; cand.u = cand.v = 0.f; cand.k = kMiss;
    // apex hint of the ray in flight (trace.hip.hpp "Pencil bundles"): camera rays leave the camera; their reflections off a
    // plane leave the camera's mirror image.  A hint only: wrong or noisy, it loosens the culling and changes no result.
    V3 mirror_apex = black;
    bool burst_done = false;                 // the trace of this iteration ran as a light burst (wave-uniform)
    unsigned long long burst_lanes = 0ull;
    uint32_t burst_plog_done = 0u, burst_part0 = 0u;   // log2(parts) of that burst; this lane's part for its first light
    uint32_t burst_nl_done = 0u;                       // lights of that burst

    for (;;) {
        // ---------- resolve: run each lane forward until it needs a ray traced (or is done)
        while (state != ST_TRACE && state != ST_DONE) {
            if (state == ST_NEW_SAMPLE) {                                   // render.hpp:35-69
                if (sample == A.sample_end) {
                    const float inv = A.spp_f;
                    if (writer) {
                        const Pixel p = my_pixel();
                        float *o = view_out() + pixel_slot(p) * 3;
                        // the last pass divides (render.hpp:72; x / 1.0f == x, bit for bit); earlier passes leave the running sum
                        if (A.spp == 1 || A.sample_end != A.spp) { o[0] = pixel_sum.x; o[1] = pixel_sum.y; o[2] = pixel_sum.z; }
                        else { o[0] = pixel_sum.x / inv; o[1] = pixel_sum.y / inv; o[2] = pixel_sum.z / inv; }
                    }
                    state = ST_DONE;
                    continue;
                }
                const Pixel p = my_pixel();
                rkey = root_key(seed_hash, p.py * A.width + p.px, (uint32_t)sample);
                // (the RNG key is the pixel's index inside ITS view: equal cameras give equal views)
                if constexpr (VIEWS) {
                    const float *cam = A.views + (size_t)view * 12u;
                    ray = camera_ray_of(A, cam, cam + 3, p.px, p.py, rkey);
                }
                else ray = camera_ray(A, p.px, p.py, rkey);
                mirror_apex = ray.o;
                cull = true; depth = 0; pend = PEND_CHILD_BG; fsp = 0;
                state = ST_TRACE;
            } else if (state == ST_SHADE) {                                 // color_hit, render.hpp:133-308
                if (depth == A.max_depth) { ret = background; state = ST_RETURN; continue; }   // :138-139
                const DevMaterial *mat = A.materials + hit_mat;
                const int kind = mat->kind;
                if (kind == RTK_MAT_CONSTANT) {
                    ret = mk(mat->albedo[0], mat->albedo[1], mat->albedo[2]);                  // :302-303
                    state = ST_RETURN;
                } else if (kind == RTK_MAT_REFLECTIVE) {
                    const RayOD refl = reflect_at(P, hn, din, A.reflection_bias);
                    // the reflected line leaves the mirror image of the incoming line's apex: as far behind P as that apex was
                    mirror_apex = P - ((length(P - mirror_apex) / length(refl.d)) * refl.d);
                    ray = spawn_ray(refl.o, refl.d);
                    rkey = child_key(rkey, 0u);
                    cull = false; depth += 1; pend = PEND_CHILD_BG;
                    state = ST_TRACE;
                } else if (FORKS && kind == RTK_MAT_REFRACTIVE) {                               // (FORKS = the general kernel)
                    const Refraction rf = refract_at(A, mat, P, mat->smooth ? hn : fn, din);
                    if (rf.tir) {
                        ray = spawn_ray(rf.refl.o, rf.refl.d);
                    } else {
                        Frame &f = frames[fsp++];                                               // the reflection ray waits for the refraction's subtree
                        f.a[0] = rf.refl.o.x; f.a[1] = rf.refl.o.y; f.a[2] = rf.refl.o.z;
                        f.a[3] = rf.refl.d.x; f.a[4] = rf.refl.d.y; f.a[5] = rf.refl.d.z;
                        f.a[6] = rf.fresnel;
                        f.meta = FR_REFR_A | ((uint32_t)depth << 8);
                        f.key = rkey;
                        ray = spawn_ray(rf.refr.o, rf.refr.d);
                    }
                    rkey = child_key(rkey, 0u);
                    cull = false; depth += 1; pend = PEND_CHILD_BLACK;
                    state = ST_TRACE;
                } else {                                                                        // diffuse :148-209, texture :211-238
                    lit_textured = FORKS && (kind == RTK_MAT_TEXTURE); // light loop only: no GI rays, no final division
                    if (!lit_textured) albedo = mk(mat->albedo[0], mat->albedo[1], mat->albedo[2]);
                    ncos = mat->smooth ? hn : fn;
                    acc = black;
                    if (FORKS && A.diffuse_rays > 0 && !lit_textured) {
                        Frame &f = frames[fsp++];
                        f.a[0] = P.x; f.a[1] = P.y; f.a[2] = P.z;
                        f.a[3] = din.x; f.a[4] = din.y; f.a[5] = din.z;
                        f.a[6] = hn.x; f.a[7] = hn.y; f.a[8] = hn.z;
                        f.a[9] = 0.f; f.a[10] = 0.f; f.a[11] = 0.f;
                        f.meta = FR_DIFFUSE | ((uint32_t)depth << 8);
                        f.tri = hit_tri;
                        f.key = rkey;
                        state = ST_RETURN;      // the frame handler below issues GI ray 0 (ret = 0 adds nothing)
                        ret = black;
                        f.meta |= 0xFFFF0000u;  // iteration = -1: "no child returned yet"
                    } else {
                        light_k = 0;
                        state = ST_LIGHT;
                    }
                }
            } else if (state == ST_LIGHT) {                                 // light loop, render.hpp:184-208
                if (light_k == A.n_lights) {
                    const float div = A.gi_div_f;
                    ret = lit_textured ? acc : mk(acc.x / div, acc.y / div, acc.z / div);
                    state = ST_RETURN;
                    continue;
                }
                const LightTerm lt = light_term(A.lights + light_k, P, ncos);
                contrib = lt.contrib;
                if (0.0f < lt.radius) {                                      // is_occluded's loop guard, :114
                    ray = spawn_ray(P + (A.shadow_bias * lt.dir), lt.dir);
                    shadow_max_t = lt.radius;
                    cull = false; pend = PEND_SHADOW;
                    state = ST_TRACE;
                } else {
                    acc = acc + (contrib * albedo);
                    light_k += 1;
                }
            } else {                                                         // ST_RETURN: hand `ret` to the caller
                if (!FORKS || fsp == 0) {
                    pixel_sum = pixel_sum + ret;                             // render.hpp:66
                    sample += 1;
                    state = ST_NEW_SAMPLE;
                    continue;
                }
                Frame &f = frames[fsp - 1];
                const uint32_t kind = f.meta & 0xFFu;
                const int fdepth = (int)((f.meta >> 8) & 0xFFu);
                if (kind == FR_REFR_A) {                                     // refraction subtree done -> reflection ray
                    f.a[7] = ret.x; f.a[8] = ret.y; f.a[9] = ret.z;
                    f.meta = FR_REFR_B | ((uint32_t)fdepth << 8);
                    ray = spawn_ray(mk(f.a[0], f.a[1], f.a[2]), mk(f.a[3], f.a[4], f.a[5]));
                    rkey = child_key(f.key, 1u);
                    cull = false; depth = fdepth + 1; pend = PEND_CHILD_BLACK;
                    state = ST_TRACE;
                } else if (kind == FR_REFR_B) {                              // :301
                    const float fresnel = f.a[6];
                    const V3 refr = mk(f.a[7], f.a[8], f.a[9]);
                    ret = (fresnel * ret) + ((1.0f - fresnel) * refr);
                    fsp -= 1;
                } else {                                                     // FR_DIFFUSE: GI loop, :151-182
                    int it = (int)(short)(f.meta >> 16);
                    if (it >= 0) { f.a[9] += ret.x; f.a[10] += ret.y; f.a[11] += ret.z; }
                    it += 1;
                    const V3 fP = mk(f.a[0], f.a[1], f.a[2]);
                    const V3 fhn = mk(f.a[6], f.a[7], f.a[8]);
                    if (it < A.diffuse_rays) {
                        f.meta = FR_DIFFUSE | ((uint32_t)fdepth << 8) | ((uint32_t)it << 16);
                        const RayOD gi = gi_ray(fP, fhn, mk(f.a[3], f.a[4], f.a[5]), f.key, (uint32_t)it, A.reflection_bias);
                        ray = spawn_ray(gi.o, gi.d);
                        rkey = child_key(f.key, (uint32_t)it);
                        cull = false; depth = fdepth + 1; pend = PEND_CHILD_BLACK;
                        state = ST_TRACE;
                    } else {                                                 // GI done: light this hit
                        P = fP; hn = fhn;
                        acc = mk(f.a[9], f.a[10], f.a[11]);
                        hit_tri = f.tri;
                        const DevShade *sh = A.tree.shade + hit_tri;
                        fn = mk(sh->fn[0], sh->fn[1], sh->fn[2]);
                        hit_mat = sh->material;
                        const DevMaterial *mat = A.materials + hit_mat;
                        albedo = mk(mat->albedo[0], mat->albedo[1], mat->albedo[2]);
                        ncos = mat->smooth ? hn : fn;
                        lit_textured = false;
                        depth = fdepth;
                        fsp -= 1;
                        light_k = 0;
                        state = ST_LIGHT;
                    }
                }
            }
        }

        // ---------- one wave-wide closest-hit query for every lane that has a ray pending
        const bool need = (state == ST_TRACE);
        if (__ballot(need) == 0ull) break;
        // hn/fn/din/ret are written when a hit (or a miss) is consumed below and read by ST_SHADE / ST_RETURN in the very next
        // resolve pass, never across a trace.  Saying so keeps twelve registers out of the traversal loops (the difference
        // between 5 resident waves per SIMD with scratch spills and 5 without).
        hn = black; fn = black; din = black; ret = black;
        hit_tri = 0u; hit_mat = 0u;              // likewise: set when a hit is consumed, read by the ST_SHADE that follows at once
        // Most queries of a frame never enter the tree (background): the root box is tested first, and when no lane passes
        // nothing else is set up -- no parking, no bundles.
        constexpr bool kRootFirst = !STATS && MODE == RTK_TRACE_WAVE;
        // ray3's inv_direction (ray3.hpp:11-14): the same three divisions, made here instead of where the ray is spawned -- the
        // quotients are only read by the box tests of the query, and would otherwise sit in (or be spilled from) three
        // registers from the shading code to this point
        ray.inv = mk((1.0f / ray.d.x), (1.0f / ray.d.y), (1.0f / ray.d.z));
        // An occlusion query whose contribution is +-0 whatever the answer is counted and consumed as ever (a miss: "clear", and
        // the +-0 is added), but takes no part in the trace (common.hip.hpp, unlit_query): not in the root test either, so that an
        // iteration of unlit lanes alone is `quiet`.  Each lane still spends one iteration per light: lanes that ran ahead on
        // their own would stand at different lights, and a burst forms only when they all stand at the same one.
        const float reach = albedo_reach(albedo);
        const bool unlit = (A.skip_unlit != 0) & need & (pend == PEND_SHADOW) && unlit_query(contrib, reach);
        const bool traced = need & !unlit;
        const bool in_root = kRootFirst ? enters_root(A.tree, ray, traced) : traced;
        // light burst (ShadowBurstService): every lane about to query a light is at the same light, and more lights follow
        bool burst = false;
        uint32_t burst_k = 0u, burst_plog = 0u, burst_nl = 0u;
        unsigned long long burst_mask = 0ull;
        bool elsewhere = false;                  // this lane's occlusion query is answered by a helper wave (another part)
        uint32_t burst_my_part = 0u;
        if (SLICES > 1 && !STATS && !light && A.has_refractive == 0) {
            const bool sh_lane = need & (pend == PEND_SHADOW);
            burst_mask = __builtin_amdgcn_ballot_w64(sh_lane);
            if (burst_mask != 0ull) {
                burst_k = (uint32_t)__builtin_amdgcn_readlane(light_k, __builtin_ctzll(burst_mask));
                const uint32_t left = (uint32_t)A.n_lights - burst_k;
                burst_nl = left < kBurstMaxJobs ? left : kBurstMaxJobs;                      // lights of this burst
                burst_plog = (burst_nl * 4u <= kBurstMaxJobs) ? 2u : (burst_nl * 2u <= kBurstMaxJobs) ? 1u : 0u;
                burst = (__builtin_amdgcn_ballot_w64(sh_lane & ((uint32_t)light_k != burst_k)) == 0ull) & (1u < (burst_nl << burst_plog));
                if (burst && A.skip_unlit != 0) {
                    // no burst when no shadow lane is lit by any of its lights: nobody would trace anything
                    bool lit = sh_lane & !unlit;
                    for (uint32_t s = 1u; s < burst_nl; ++s)                                // (the light is wave-uniform)
                        lit |= sh_lane & !unlit_query(light_term(A.lights + burst_k + s, P, ncos).contrib, reach);
                    burst = wave_any(lit);
                }
                if (burst) burst_my_part = burst_part(ray.d, sh_lane, burst_plog);   // (every shadow lane of a burst is at light burst_k)
                elsewhere = burst & sh_lane & (burst_my_part != 0u);
            }
        }
        const bool quiet = kRootFirst && !burst && !wave_any(in_root);
        if (quiet) {
            cand.t = kFltMax; cand.u = cand.v = 0.f; cand.k = kMiss;
            burst_done = false;
        } else {
        // State that is live across the query but not used by it waits in LDS instead of in registers: with it the
        // traversal loops overflow the 96 registers of a 5-waves-per-SIMD build into scratch (measured: a background block
        // spent more time on scratch reloads than on its rays).  [var][lane] layout: conflict-free, 36 LDS operations per query.
        float *const park = &park_lds[park_slot][0][fresh_lane()];
        park[0 * 64] = pixel_sum.x; park[1 * 64] = pixel_sum.y; park[2 * 64] = pixel_sum.z;
        park[3 * 64] = acc.x; park[4 * 64] = acc.y; park[5 * 64] = acc.z;
        park[6 * 64] = albedo.x; park[7 * 64] = albedo.y; park[8 * 64] = albedo.z;
        park[9 * 64] = ncos.x; park[10 * 64] = ncos.y; park[11 * 64] = ncos.z;
        park[12 * 64] = P.x; park[13 * 64] = P.y; park[14 * 64] = P.z;
        park[15 * 64] = mirror_apex.x; park[16 * 64] = mirror_apex.y; park[17 * 64] = mirror_apex.z;
        phases.trace_begins();
        // shadow rays of scenes without transmissive materials only ask "is the closest hit nearer than the light":
        // they may stop at the first hit that says yes (trace(), `exit_t`; A.shadow_exit is set by the host).
        const float exit_t = (A.shadow_exit && pend == PEND_SHADOW) ? shadow_max_t : -1.0f;
        // ray class for the bundle culling: shadow rays by light, everything else by depth (camera rays = 0)
        // (shadow rays end in their light: the lines of a class pass through that point, the "apex" of a pencil bundle)
        uint32_t cls = (uint32_t)depth;
        V3 apex = black;
        if (pend == PEND_CHILD_BG) { cls |= kClsHasApex; apex = mirror_apex; }      // camera rays and chains of reflections
        if (pend == PEND_SHADOW) {
            const DevLight *L = A.lights + light_k;
            cls = kClsHasApex | (0x100u + (uint32_t)light_k + 0x40u * (uint32_t)depth);   // (different depths: different surfaces)
            apex = mk(L->pos[0], L->pos[1], L->pos[2]);
        }
        if (burst) {
            const uint32_t lane = fresh_lane();
            group_sh->ray_o[lane] = make_float4(P.x, P.y, P.z, ncos.x);
            group_sh->ray_d[lane] = make_float4(ncos.y, ncos.z, reach, 0.f);
            if (lane == 0u) {
                group_sh->pass_mask = burst_mask; group_sh->first = burst_k; group_sh->count = burst_plog | ((burst_nl << burst_plog) << 8);
                group_sh->pad[0] = 1u;                                  // next job to hand out (job 0 is traced right here)
                // (an opaque constant: folded, it becomes one lane of a three-register tuple {first, count, kind} that is
                // set up in the kernel's prologue and spilled to scratch until it is needed here)
                uint32_t extra = GROUP_EXTRA;
                asm volatile("" : "+v"(extra));
                group_sh->kind = extra;
            }
            __syncthreads();                                            // B1: the helpers start on their lights
            sx.min_tris = 0xFFFFFFFFu;                                  // (they are busy: the owner's own leaves stay whole)
        }
        cand = trace<MODE, STATS, kStage, SLICES, kRootFirst>(A.tree, lds_nodes, ray, cull, in_root & !elsewhere, st, sx, kAutoMinLanes, exit_t, cls, apex);   // (in_root: no unlit lane)
        phases.trace_returned();
        if (burst) {
            __syncthreads();                                            // B2: their answers are in LDS
            sx.min_tris = A.slice_min_tris;
        }
        phases.trace_done(sx.probe(), burst, SLICES > 1, burst_plog, in_root);
        burst_done = burst; burst_lanes = burst_mask; burst_plog_done = burst_plog; burst_part0 = burst_my_part;
        burst_nl_done = burst_nl;

        float *const unpark = &park_lds[park_slot][0][fresh_lane()];
        pixel_sum = mk(unpark[0 * 64], unpark[1 * 64], unpark[2 * 64]);
        acc = mk(unpark[3 * 64], unpark[4 * 64], unpark[5 * 64]);
        albedo = mk(unpark[6 * 64], unpark[7 * 64], unpark[8 * 64]);
        ncos = mk(unpark[9 * 64], unpark[10 * 64], unpark[11 * 64]);
        P = mk(unpark[12 * 64], unpark[13 * 64], unpark[14 * 64]);
        mirror_apex = mk(unpark[15 * 64], unpark[16 * 64], unpark[17 * 64]);
        }

        // ---------- consume
        uint32_t more_rays = 0u;                 // this lane's rays of this iteration (<= 1 + the lights of a burst)
        if (need) {
            const uint32_t lane = fresh_lane();
            more_rays = 1u;
            const bool hit = cand.k != kMiss;
            if (pend == PEND_SHADOW) {                                       // is_occluded, render.hpp:110-131
                // (occlusion_step() written out: calling it here costs the benchmark's kernel its register allocation)
                bool clear = !hit | (shadow_max_t < cand.t);
                const bool in_burst = SLICES > 1 && burst_done && ((burst_lanes >> lane) & 1ull) != 0ull;
                const uint32_t my_part = in_burst ? burst_part0 : 0u;
                if (my_part != 0u) clear = burst_res[my_part * 64u + lane].y != 0.0f;     // light k of the other parts: a helper's answer
                bool again = false;
                if (!clear && A.has_refractive) {
                    const uint32_t tri = A.tree.tri_ids[cand.k];
                    const uint32_t m = A.tree.shade[tri].material;
                    if (A.materials[m].kind == RTK_MAT_REFRACTIVE) {         // transmissive: step through, :126-127
                        const V3 hp = ray.o + (cand.t * ray.d);
                        ray.o = hp + (A.shadow_bias * ray.d);
                        shadow_max_t -= cand.t;
                        if (0.0f < shadow_max_t) again = true; else clear = true;
                    }
                }
                if (!again) {
                    if (clear) acc = acc + (contrib * albedo);               // :205
                    light_k += 1;
                    state = ST_LIGHT;
                    if (in_burst) {
                        // the helpers' lights, in light order: the same float sum as the sequential loop
                        const uint32_t plog = burst_plog_done;
                        for (uint32_t s = 1u; s < burst_nl_done; ++s) {
                            for (uint32_t pp = 0u; pp < (1u << plog); ++pp) {          // exactly one part answers for this lane
                                const float4 res = burst_res[((s << plog) + pp) * 64u + lane];
                                const uint32_t fl = __float_as_uint(res.z);
                                if ((fl & 2u) != 0u) {
                                    if (res.y != 0.0f) acc = acc + (res.x * albedo);
                                    more_rays += fl & 1u;
                                }
                            }
                            light_k += 1;
                        }
                    }
                }
            } else if (!hit) {
                ret = (pend == PEND_CHILD_BG) ? background : black;
                state = ST_RETURN;
            } else {
                const Surface s = reconstruct(A.tree, cand);
                P = ray.o + (cand.t * ray.d);                                // kd_tree_simd.hpp:254
                hn = s.hit_normal; fn = s.face_normal; din = ray.d;
                hit_tri = s.tri; hit_mat = s.material;
                if (FORKS && A.tri_uv != nullptr && A.materials[hit_mat].kind == RTK_MAT_TEXTURE)   // texture_material: colour of this hit
                    albedo = sample_texture(A.textures + A.materials[hit_mat].texture, A.tri_uv + hit_tri, cand.u, cand.v, A.tex_pixels);
                state = ST_SHADE;
            }
        }
        // (added up here, in uniform control flow, bit by bit through ballots: four scalar popcounts)
        nrays_wave += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((more_rays & 1u) != 0u)) +
                      2u * (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((more_rays & 2u) != 0u)) +
                      4u * (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((more_rays & 4u) != 0u)) +
                      8u * (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((more_rays & 8u) != 0u));
        static_assert(kBurstMaxJobs + 1u <= 15u, "a lane's rays of one iteration fit four bits");
    }

    const uint32_t lane = fresh_lane();
    if (kPhases && valid && writer) {
        const Pixel p = my_pixel();
        phases.write(sx.probe(), lane, view_out() + pixel_slot(p) * 3);
    }
    if (A.cost_out != nullptr && lane == 0u && gwave < A.n_units) {        // what this block cost, for the next frame's order
        // (a block that ran alone on one wave of a packed workgroup took about twice as long as it would with helpers)
        const unsigned long long dt = (__builtin_readcyclecounter() - cost_t0) >> (light ? 5 : 4);
        A.cost_out[gwave] = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dt;
    }
    {   // the longest pixel block of the frame: what the frame cannot be shorter than.  Only long blocks report, into one of 64
        // words (a single word takes ~88 atomics per microsecond: every block reporting would serialise the frame).
        const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - real_t0;
        if (lane == 0u && dt >= kCriticalMinTicks) atomicMax(A.counters + kCriticalWord + (gwave % (uint32_t)kRayCounterShards), dt);
    }
    if (SLICES > 1 && !light) group_post_exit(group_sh);
    const uint32_t total = nrays_wave;
    if (STATS && writer) flush_stats(st, 0u, A.counters);
    // one no-return atomic per pixel block, spread over 64 words (a single word saturates near 88 atomics/us)
    if (lane == 0u && writer) atomicAdd(A.counters + kRayShardWord + (gwave % (uint32_t)kRayCounterShards), (unsigned long long)total);
}

// ------------------------------------------------------------------------------------------------
// After the all-gather: [world][buckets_per_rank][bucket*bucket][3] -> frame [h][w][3].
__global__ __launch_bounds__(256) void k_assemble(AssembleArgs A) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)A.width * A.height) return;
    const uint32_t px = (uint32_t)(i % A.width), py = (uint32_t)(i / A.width);
    const uint32_t bucket = (py / A.bucket) * A.tiles_x + (px / A.bucket);
    uint32_t rank, local;
    bucket_owner(bucket, A.tiles_x, A.world, A.skew_q, rank, local);
    const size_t src = (((size_t)rank * A.buckets_per_rank + local) * A.bucket + (py % A.bucket)) * A.bucket + (px % A.bucket);
    A.rgb[i * 3 + 0] = A.gathered[src * 3 + 0];
    A.rgb[i * 3 + 1] = A.gathered[src * 3 + 1];
    A.rgb[i * 3 + 2] = A.gathered[src * 3 + 2];
}

// ------------------------------------------------------------------------------------------------
// The camera rays of one sample of every pixel (render.hpp:35-62), [h][w] row-major: one thread per pixel.
__global__ __launch_bounds__(256) void k_camera_rays(RenderArgs A, int sample, rtk_ray *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)A.width * A.height) return;
    const uint32_t px = (uint32_t)(i % A.width), py = (uint32_t)(i / A.width);
    const Ray r = camera_ray(A, px, py, root_key(pcg_hash(A.seed), py * A.width + px, (uint32_t)sample));
    float *o = reinterpret_cast<float *>(out + i);
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
}

// The streaming path of rtk_render_regions.  Pixel i of a launch's entries (RegionEntry::first_pixel order: rectangle after
// rectangle, each row-major) -> its rectangle (a binary search per thread: one thread per pixel, nothing here is hot) and its
// frame coordinates.
struct RegionPixel { const RegionEntry *R; uint32_t px, py; };
__device__ __forceinline__ RegionPixel region_pixel(const RenderArgs &A, const uint64_t i) {
    uint32_t lo = 0u, hi = A.n_regions;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.regions[mid].first_pixel <= i) lo = mid; else hi = mid;
    }
    RegionPixel q;
    q.R = A.regions + lo;
    const uint64_t local = i - q.R->first_pixel;
    const uint32_t w = (uint32_t)q.R->w, row = (uint32_t)(local / w);
    q.py = (uint32_t)q.R->y0 + row;
    q.px = (uint32_t)q.R->x0 + (uint32_t)(local - (uint64_t)row * w);
    return q;
}

// camera rays (k_camera_rays' arithmetic: the frame's px, py, width, height and RNG key) and frame pixel indices of pixels
// [first, first + n) at `sample`: what rtk_accel_radiance needs to give exactly that sample of the frame
__global__ __launch_bounds__(256) void k_region_rays(RenderArgs A, int sample, uint64_t first, uint32_t n, rtk_ray *out, uint32_t *ids) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n || A.n_regions == 0u) return;
    const RegionPixel q = region_pixel(A, first + t);
    const uint32_t pixel = q.py * A.width + q.px;
    const Ray r = camera_ray(A, q.px, q.py, root_key(pcg_hash(A.seed), pixel, (uint32_t)sample));
    float *o = reinterpret_cast<float *>(out + t);
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
    ids[t] = pixel;
}

// pixel_sum += colour (render.hpp:66), in sample order because the launches of a pixel are on one stream; the sample that ends
// the frame divides (render.hpp:72), as k_render's ST_NEW_SAMPLE does.  A colour arrives as +0 + c (rtk.h, rtk_accel_radiance).
__global__ __launch_bounds__(256) void k_region_accumulate(RenderArgs A, uint64_t first, uint32_t n, const float *rgb, int start, int divide) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n || A.n_regions == 0u) return;
    const RegionPixel q = region_pixel(A, first + t);
    float *o = A.out + (size_t)(q.R->base + (long long)q.py * (long long)q.R->pitch + (long long)q.px) * 3;
    const float *c = rgb + (size_t)t * 3;
    V3 sum = start ? mk(0.f, 0.f, 0.f) : mk(o[0], o[1], o[2]);
    sum = sum + mk(c[0], c[1], c[2]);
    if (divide) { const float inv = A.spp_f; sum = mk(sum.x / inv, sum.y / inv, sum.z / inv); }
    o[0] = sum.x; o[1] = sum.y; o[2] = sum.z;
}

__global__ void k_add_word(unsigned long long *dst, const unsigned long long *src) {
    if (threadIdx.x == 0u && blockIdx.x == 0u) dst[0] += src[0];
}

// write_ppm's quantisation (io/image/ppm.hpp:17-19): uint8(255.999 * clamp(c, 0, 1)), the product in double.
__device__ __forceinline__ uint8_t to_rgb8(const float c) {
    const float k = (c < 0.0f) ? 0.0f : ((1.0f < c) ? 1.0f : c);           // std::clamp(c, 0.f, 1.f)
    return (uint8_t)(255.999 * (double)k);
}

__global__ __launch_bounds__(256) void k_to_rgb8(const float *rgb, size_t n, uint8_t *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = to_rgb8(rgb[i]);
}

// rtk_accel_set_texture_frame_device: the same bytes, packed, to a texture's slot -- any byte address.  Behind the up to three
// bytes in front of the first dword boundary a thread owns four pixels: twelve floats in, three dwords out, so a wave's stores
// are 768 consecutive bytes.  The thread behind the last group writes the ragged head and tail (fewer than 15 bytes) one by one.
__global__ __launch_bounds__(256) void k_frame_to_texels(const float *rgb, size_t n, uint8_t *out) {
    const size_t to_boundary = (size_t)((4u - (unsigned)((uintptr_t)out & 3u)) & 3u);
    const size_t head = to_boundary < n ? to_boundary : n;
    const size_t groups = (n - head) / 12u;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < groups) {
        const float *src = rgb + head + t * 12u;
        uint32_t *dst = reinterpret_cast<uint32_t *>(out + head) + t * 3u;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float *c = src + j * 4;
            dst[j] = (uint32_t)to_rgb8(c[0]) | ((uint32_t)to_rgb8(c[1]) << 8) | ((uint32_t)to_rgb8(c[2]) << 16) | ((uint32_t)to_rgb8(c[3]) << 24);
        }
    } else if (t == groups) {
        for (size_t i = 0; i < head; ++i) out[i] = to_rgb8(rgb[i]);
        for (size_t i = head + groups * 12u; i < n; ++i) out[i] = to_rgb8(rgb[i]);
    }
}

}  // namespace dev

// ------------------------------------------------------------------------------------------------ launchers

namespace {

template <int MODE, bool STATS>
hipError_t launch_intersect_m(const dev::IntersectArgs &A, bool lds, size_t lds_bytes, hipStream_t s) {
    const unsigned blocks = (unsigned)((A.n + 255) / 256);
    if (blocks == 0) return hipSuccess;
    // only the per-lane walk reads the node array from LDS: the wave-cooperative one fetches nodes and leaves through the scalar
    // cache (staging the array for it copied 6 KB per 256 rays for nothing)
    constexpr bool kNeedsNodes = (MODE == RTK_TRACE_LANE || MODE == RTK_TRACE_AUTO);
    if constexpr (kNeedsNodes) {
        if (lds) { hipLaunchKernelGGL((dev::k_intersect<MODE, STATS, true>), dim3(blocks), dim3(256), lds_bytes, s, A); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((dev::k_intersect<MODE, STATS, false>), dim3(blocks), dim3(256), 0, s, A);
    return hipGetLastError();
}

// (units, mode) -> kernel: VIEWS / REGIONS say what a unit of the launch is (a frame's pixel block; a (view, block) or a
// (rectangle, block) pair of the one-launch calls).  The LDS_NODES build exists only for the modes that walk per lane.
template <int MODE, bool STATS, bool FORKS, int SLICES, bool VIEWS = false, bool REGIONS = false>
hipError_t launch_render_m(const dev::RenderArgs &A, unsigned blocks, bool lds, size_t lds_bytes, hipStream_t s) {
    const unsigned threads = SLICES > 1 ? 64u * SLICES : 256u;
    constexpr bool kNeedsNodes = (MODE == RTK_TRACE_LANE || MODE == RTK_TRACE_AUTO);
    if constexpr (kNeedsNodes) {
        if (lds) { hipLaunchKernelGGL((dev::k_render<MODE, STATS, FORKS, true, SLICES, VIEWS, REGIONS>), dim3(blocks), dim3(threads), lds_bytes, s, A); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((dev::k_render<MODE, STATS, FORKS, false, SLICES, VIEWS, REGIONS>), dim3(blocks), dim3(threads), 0, s, A);
    return hipGetLastError();
}

// the builds of one (mode, waves per unit): per-ray statistics exist for a frame's own pixel blocks only
template <int MODE, int SLICES, bool VIEWS, bool REGIONS>
hipError_t launch_render_mode(const dev::RenderArgs &A, unsigned blocks, bool stats, bool forks, bool lds, size_t lds_bytes,
                              hipStream_t s) {
    if constexpr (!VIEWS && !REGIONS) {
        if (stats) return forks ? launch_render_m<MODE, true, true, SLICES>(A, blocks, lds, lds_bytes, s)
                                : launch_render_m<MODE, true, false, SLICES>(A, blocks, lds, lds_bytes, s);
    }
    return forks ? launch_render_m<MODE, false, true, SLICES, VIEWS, REGIONS>(A, blocks, lds, lds_bytes, s)
                 : launch_render_m<MODE, false, false, SLICES, VIEWS, REGIONS>(A, blocks, lds, lds_bytes, s);
}

// The one table (units, mode) -> kernel and grid, for a frame and for rtk_render_views / rtk_render_regions as one launch (the GROUP
// modes, no statistics: launch_render has refused the rest).  `listed`: the workgroups of GROUP4's list, when the host knows.
template <bool VIEWS, bool REGIONS>
hipError_t launch_render_units(const dev::RenderArgs &A, int mode, unsigned units, unsigned listed, bool stats, bool forks, hipStream_t s) {
    const size_t lds_bytes = (size_t)A.tree.n_nodes * sizeof(DevNode);
    const bool lds = lds_bytes <= kMaxNodeLdsBytes;
    switch (mode) {
        // (with a workgroup list the kernel's workgroups beyond the list return at once; launched all the same they are ~100,000
        // waves of a config-2 frame that only start and stop)
        case RTK_TRACE_GROUP4: return launch_render_mode<RTK_TRACE_WAVE, 4, VIEWS, REGIONS>(A, listed, stats, forks, lds, lds_bytes, s);
        case RTK_TRACE_GROUP8: return launch_render_mode<RTK_TRACE_WAVE, 8, VIEWS, REGIONS>(A, units, stats, forks, lds, lds_bytes, s);
        case RTK_TRACE_GROUP16: return launch_render_mode<RTK_TRACE_WAVE, 16, VIEWS, REGIONS>(A, units, stats, forks, lds, lds_bytes, s);
        default: break;
    }
    if constexpr (VIEWS || REGIONS) return hipErrorInvalidValue;
    else {
        const unsigned packed = (units + 3u) / 4u;                          // 4 pixel blocks per workgroup
        switch (mode) {
            case RTK_TRACE_LANE: return launch_render_mode<RTK_TRACE_LANE, 1, false, false>(A, packed, stats, forks, lds, lds_bytes, s);
            case RTK_TRACE_WAVE: return launch_render_mode<RTK_TRACE_WAVE, 1, false, false>(A, packed, stats, forks, lds, lds_bytes, s);
            default: return launch_render_mode<RTK_TRACE_AUTO, 1, false, false>(A, packed, stats, forks, lds, lds_bytes, s);
        }
    }
}

}  // namespace

hipError_t launch_intersect(const dev::IntersectArgs &A, int mode, bool stats, hipStream_t s) {
    const size_t lds_bytes = (size_t)A.tree.n_nodes * sizeof(DevNode);
    const bool lds = lds_bytes <= kMaxNodeLdsBytes;
    switch (mode) {
        case RTK_TRACE_LANE:
            return stats ? launch_intersect_m<RTK_TRACE_LANE, true>(A, lds, lds_bytes, s)
                         : launch_intersect_m<RTK_TRACE_LANE, false>(A, lds, lds_bytes, s);
        case RTK_TRACE_WAVE:
            return stats ? launch_intersect_m<RTK_TRACE_WAVE, true>(A, lds, lds_bytes, s)
                         : launch_intersect_m<RTK_TRACE_WAVE, false>(A, lds, lds_bytes, s);
        default:
            return stats ? launch_intersect_m<RTK_TRACE_AUTO, true>(A, lds, lds_bytes, s)
                         : launch_intersect_m<RTK_TRACE_AUTO, false>(A, lds, lds_bytes, s);
    }
}

hipError_t launch_render(const dev::RenderArgs &A, int mode, bool stats, bool forks, hipStream_t s, unsigned n_workgroups) {
#ifdef RTK_ONLY_LEAN_G4     // `make asm-lean`: the benchmark's kernel alone, for quick looks at its ISA (not a product build)
    hipLaunchKernelGGL((dev::k_render<RTK_TRACE_WAVE, false, false, false, 4>), dim3(A.n_units), dim3(256), 0, s, A);
    return hipGetLastError();
#else
    // how many units the launch has, and whether they are what the arguments say they are: whoever did not make them consistent
    // gets an error, not a kernel that indexes by them
    if (A.regions != nullptr) {
        // (rectangle, block) units: the entries say how many there are
        if (stats || A.views != nullptr || A.n_regions == 0u || A.n_units == 0u || A.n_units > 0x7FFFFFFFu || A.world > 1) return hipErrorInvalidValue;
        const unsigned listed = (n_workgroups != 0u && n_workgroups < A.n_units) ? n_workgroups : A.n_units;
        return launch_render_units<false, true>(A, mode, A.n_units, listed, false, forks, s);
    }
    const uint32_t bpb = A.blocks_per_bucket_side * A.blocks_per_bucket_side;
    const uint64_t waves = (uint64_t)A.buckets_per_rank * bpb * (A.views != nullptr ? A.n_views : 1u);   // one per 8x8 pixel block (of every view)
    if (waves == 0) return hipSuccess;
    if (waves > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned listed = (n_workgroups != 0u && n_workgroups < waves) ? n_workgroups : (unsigned)waves;
    if (A.views != nullptr) {
        // (view, block) units
        if (stats || (uint64_t)A.units_per_view * A.n_views != waves || A.n_units != waves) return hipErrorInvalidValue;
        return launch_render_units<true, false>(A, mode, (unsigned)waves, listed, false, forks, s);
    }
    return launch_render_units<false, false>(A, mode, (unsigned)waves, listed, stats, forks, s);
#endif
}

// A prior for the FIRST frame of a shape, when no frame has reported its blocks' costs yet.  One thread per 8x8 pixel block
// sorts it into one of three classes, and a second small kernel lays the launch list out class by class (no sort: ~10 us
// in front of the frame where k_order_by_cost needs 66):
//   1  some probe ray (the four corner pixels, the centre) enters the tree's root box -- first, a workgroup each
//   0  none does: background -- packed four to a workgroup, last
//   (2 is kept for a class to be started before both)
// Only the launch order depends on the classes, no result.  From the second frame on the measured costs take over.
namespace dev {
template <bool VIEWS>
__global__ __launch_bounds__(256) void k_block_prior(RenderArgs A, uint8_t *cls, uint32_t *count /* [3], zeroed */) {
    const uint32_t unit = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = unit < A.n_units;
    // VIEWS: unit = view * units_per_view + block, and the probe rays leave that view's camera (a thread each: per-lane loads)
    const uint32_t view = (VIEWS && have) ? unit / A.units_per_view : 0u;
    const BlockMap blk = block_map(A, have ? unit - view * (VIEWS ? A.units_per_view : 0u) : 0u);
    const uint32_t x0 = blk.bx + blk.sub_x0, y0 = blk.by + blk.sub_y0;
    const bool in_frame = have && blk.bucket < A.n_buckets && x0 < A.width && y0 < A.height;
    const uint32_t x1 = x0 + 7u < A.width ? x0 + 7u : A.width - 1u, y1 = y0 + 7u < A.height ? y0 + 7u : A.height - 1u;
    RenderArgs P = A;
    P.spp = 1;                                                                  // pixel centres: this is an estimate
    if constexpr (VIEWS) {
        const float *cam = A.views + (size_t)(view < A.n_views ? view : 0u) * 12u;
        for (int i = 0; i < 3; ++i) P.cam_pos[i] = cam[i];
        for (int i = 0; i < 9; ++i) P.cam_mat[i] = cam[3 + i];
    }
    const float4 *root = reinterpret_cast<const float4 *>(A.tree.nodes);
    const float4 r0 = root[0], r1 = root[1];
    float t_min;
    const Ray centre = camera_ray(P, in_frame ? (x0 + x1) >> 1 : 0u, in_frame ? (y0 + y1) >> 1 : 0u, 0u);
    const bool centre_in = in_frame && slab(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, centre, t_min);
    bool enters = centre_in;
    if (in_frame) {
        const uint32_t px[4] = {x0, x1, x0, x1}, py[4] = {y0, y0, y1, y1};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const Ray r = camera_ray(P, px[i], py[i], 0u);
            enters = enters | slab(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r, t_min);
        }
    }
    // (Knowing what the centre ray HITS -- a mirror whose reflections fan out over the mesh is where config 2's longest blocks
    // are -- would give a better order still: the frame went from 0.37 to 0.29 ms with such blocks first.  But tracing the 32,400
    // centre rays, 64 to a wave, takes 0.24 ms: their bundles are 64 pixels wide and cull nothing.  Measured, not kept.)
    const uint32_t c = enters ? 1u : 0u;
    if (have) cls[unit] = (uint8_t)c;
#pragma unroll
    for (uint32_t q = 0; q < 3u; ++q) {                                        // one atomic per wave and class
        const unsigned long long m = __builtin_amdgcn_ballot_w64(have && c == q);
        if (m != 0ull && (int)__lane_id() == __builtin_ctzll(m)) atomicAdd(count + q, (uint32_t)__popcll(m));
    }
}

// order[] = the blocks class by class (2, 1, 0), wg_list / hdr as k_order_by_cost leaves them (RenderArgs::wg_list)
__global__ __launch_bounds__(256) void k_prior_layout(const uint8_t *cls, const uint32_t *count, uint32_t *cursor /* [3], zeroed */,
                                                      uint32_t *order, uint32_t *wg_list, uint32_t *hdr, uint32_t n, uint32_t pack) {
    const uint32_t unit = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = unit < n;
    const uint32_t c = have ? (uint32_t)cls[unit] : 3u;
    const uint32_t n2 = count[2], n1 = count[1], n0 = count[0];
    uint32_t pos = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 3u; ++q) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(have && c == q);
        if (m == 0ull) continue;
        const int leader = __builtin_ctzll(m);
        uint32_t first = 0u;
        if ((int)__lane_id() == leader) first = atomicAdd(cursor + q, (uint32_t)__popcll(m));
        first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);
        if (c == q) pos = first + (uint32_t)__popcll(m & ((1ull << __lane_id()) - 1ull));
    }
    if (have) {
        const uint32_t at = c == 2u ? pos : (c == 1u ? n2 + pos : n2 + n1 + pos);
        order[at] = unit;
        if (c != 0u) wg_list[at] = unit;
        else if (pos % pack == 0u) wg_list[n2 + n1 + pos / pack] = 0x80000000u | at;
    }
    if (unit == 0u) { hdr[0] = n2 + n1 + (n0 + pack - 1u) / pack; hdr[1] = n; }
}
}  // namespace dev

hipError_t launch_block_prior(const dev::RenderArgs &A, uint8_t *cls, uint32_t *order, uint32_t *wg_list, uint32_t *hdr,
                              uint32_t *scratch /* [6], zeroed by the caller */, uint32_t pack, hipStream_t s) {
    if (A.n_units == 0u) return hipSuccess;
    // (`scratch` comes zeroed: it lies behind the frame's counters and is cleared with them -- a fill of its own, two in fact for 24
    // bytes, was 15 us in front of the first frame)
    const unsigned blocks = (A.n_units + 255u) / 256u;
    if (A.views != nullptr) hipLaunchKernelGGL(dev::k_block_prior<true>, dim3(blocks), dim3(256), 0, s, A, cls, scratch);
    else hipLaunchKernelGGL(dev::k_block_prior<false>, dim3(blocks), dim3(256), 0, s, A, cls, scratch);
    hipLaunchKernelGGL(dev::k_prior_layout, dim3(blocks), dim3(256), 0, s, cls, scratch, scratch + 3, order, wg_list, hdr, A.n_units, pack);
    return hipGetLastError();
}

namespace dev {
__global__ __launch_bounds__(256) void k_counters_fold(const unsigned long long *cur, unsigned long long *acc) {
    const uint32_t i = threadIdx.x;
    if (i >= (uint32_t)kCounterWords) return;
    const bool longest = i >= (uint32_t)kCriticalWord;                      // the critical path of a call is its longest block
    const unsigned long long a = acc[i], c = cur[i];
    acc[i] = longest ? (a < c ? c : a) : a + c;
}
}  // namespace dev

hipError_t launch_counters_fold(const unsigned long long *cur, unsigned long long *acc, hipStream_t s) {
    hipLaunchKernelGGL(dev::k_counters_fold, dim3(1), dim3(256), 0, s, cur, acc);
    return hipGetLastError();
}

// Counting sort of the pixel blocks by last frame's cost, most expensive first.  One workgroup: a frame has tens of
// thousands of blocks, the whole job is two passes over a few hundred KB.
namespace dev {
__device__ __forceinline__ uint32_t cost_bin(uint32_t c) {                 // 8 bins per octave
    c |= 1u;
    const uint32_t e = 31u - (uint32_t)__clz((int)c);
    const uint32_t m = e >= 3u ? (c >> (e - 3u)) & 7u : (c << (3u - e)) & 7u;
    return e * 8u + m;                                                     // 0..255
}
__global__ __launch_bounds__(1024) void k_order_by_cost(const uint32_t *cost, uint8_t *bins, uint32_t *order, uint32_t *wg_list,
                                                        uint32_t *hdr, uint32_t n, uint32_t light_below, uint32_t floor_below,
                                                        uint32_t pack, uint32_t *judge, int champion) {
    // The frame in front of this launch ran the list in use, the champion: from its stamp to now is that list's score (order_judge.hpp),
    // refreshed by every sort.  A shape's first sort has no list behind it: no champion.
    if (judge != nullptr && threadIdx.x == 0u) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        const unsigned long long t0 = *reinterpret_cast<const unsigned long long *>(judge + kJudgeStampLo);
        if (champion != kChampionLeave) judge[kJudgeChampion] = champion == kChampionScore ? judge_score(t0, now) : 0u;
    }
    __shared__ uint32_t hist[256];
    __shared__ uint32_t start[256];
    __shared__ uint32_t wg_hist[2][256], wg_base[2][256];
    __shared__ uint32_t n_single_sh;
    const uint32_t light_bin = light_below > 0u ? cost_bin(light_below) : 0u;  // blocks in bins below it are packed `pack` to a workgroup
    // ... and of those, the ones below `floor_bin` need no order among themselves (background, a handful of nodes)
    const uint32_t floor_raw = floor_below > 0u ? cost_bin(floor_below) : 0u;
    const uint32_t floor_bin = floor_raw < light_bin ? floor_raw : light_bin;
    constexpr uint32_t kBatch = 8;                                          // loads in flight per thread: the kernel is one workgroup,
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) { hist[i] = 0u; wg_hist[0][i] = 0u; wg_hist[1][i] = 0u; }   // so memory latency, not bandwidth, is what it waits for
    __syncthreads();
    // the bin of every block is computed once and kept: `order` is a permutation even if cost[] changes under us
    for (uint32_t base = 0; base < n; base += blockDim.x * kBatch) {
        uint32_t c[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t i = base + k * blockDim.x + threadIdx.x;
            c[k] = i < n ? cost[i] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t i = base + k * blockDim.x + threadIdx.x;
            // most blocks of a frame are cheap and need no order among themselves: they all go to bin 0, counted once per wave
            uint32_t b = i < n ? cost_bin(c[k]) : 0u;
            if (b < floor_bin) b = 0u;
            if (i < n) bins[i] = (uint8_t)b;
            const unsigned long long cheap = __builtin_amdgcn_ballot_w64(i < n && b == 0u);
            if (i < n && b != 0u) atomicAdd(&hist[b], 1u);
            if (cheap != 0ull && (int)__lane_id() == __builtin_ctzll(cheap)) atomicAdd(&hist[0], (uint32_t)__popcll(cheap));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t acc = 0u;
        uint32_t singles = 0u;
        for (int b = 255; b >= 0; --b) {
            start[b] = acc; acc += hist[b];
            if (light_bin == 0u || (uint32_t)b >= light_bin) singles = acc;
        }
        n_single_sh = light_bin > 0u ? singles : n;                          // order[0, n_single): one workgroup each; the rest packed
        hdr[1] = n;
    }
    __syncthreads();
    for (uint32_t base = 0; base < n; base += blockDim.x * kBatch) {
        uint32_t b[kBatch], pos[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t i = base + k * blockDim.x + threadIdx.x;
            b[k] = i < n ? (uint32_t)bins[i] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t i = base + k * blockDim.x + threadIdx.x;
            const unsigned long long cheap = __builtin_amdgcn_ballot_w64(i < n && b[k] == 0u);
            pos[k] = 0u;
            if (i < n && b[k] != 0u) pos[k] = atomicAdd(&start[b[k]], 1u);
            if (cheap != 0ull) {
                const int leader = __builtin_ctzll(cheap);
                uint32_t first = 0u;
                if ((int)__lane_id() == leader) first = atomicAdd(&start[0], (uint32_t)__popcll(cheap));
                first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);
                if (i < n && b[k] == 0u) pos[k] = first + (uint32_t)__popcll(cheap & ((1ull << __lane_id()) - 1ull));
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t i = base + k * blockDim.x + threadIdx.x;
            if (i < n) order[pos[k]] = i;
        }
    }
    // The launch order of the WORKGROUPS: by how long each will run.  A packed workgroup runs its blocks one wave each, with
    // no helpers: it takes about twice as long as its most expensive block would take alone (8 bins = one octave), and
    // has to start as early as the single-block workgroups of that duration -- started behind all of them it is the
    // frame's tail.  wg_list[w] = block id, or 0x80000000 | index into order[] of the first of `pack` blocks.
    __threadfence_block();
    __syncthreads();
    const uint32_t n_single = n_single_sh;
    const uint32_t n_packed = (n - n_single + pack - 1u) / pack;
    const uint32_t n_wgs = n_single + n_packed;
    for (uint32_t w = threadIdx.x; w < n_wgs; w += blockDim.x) {
        const bool packed = w >= n_single;
        const uint32_t at = packed ? n_single + (w - n_single) * pack : w;
        uint32_t key = (uint32_t)bins[order[at]];
        if (packed && key != 0u) key = key + 8u < 255u ? key + 8u : 255u;
        atomicAdd(&wg_hist[packed ? 1 : 0][key], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t acc = 0u;
        for (int b = 255; b >= 0; --b) {
            wg_base[0][b] = acc; acc += wg_hist[0][b];
            wg_base[1][b] = acc; acc += wg_hist[1][b];
        }
        hdr[0] = n_wgs;
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < n_wgs; w += blockDim.x) {
        const bool packed = w >= n_single;
        const uint32_t at = packed ? n_single + (w - n_single) * pack : w;
        const uint32_t blk = order[at];
        uint32_t key = (uint32_t)bins[blk];
        if (packed && key != 0u) key = key + 8u < 255u ? key + 8u : 255u;
        const uint32_t pos = atomicAdd(&wg_base[packed ? 1 : 0][key], 1u);
        wg_list[pos] = packed ? (0x80000000u | at) : blk;
    }
}
}  // namespace dev

hipError_t launch_order_by_cost(const uint32_t *cost, uint8_t *bins, uint32_t *order, uint32_t *wg_list, uint32_t *hdr, uint32_t n,
                                uint32_t light_below, uint32_t floor_below, uint32_t pack, hipStream_t s, uint32_t *judge, int champion) {
    if (n == 0u) return hipSuccess;
    if (pack == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_order_by_cost, dim3(1), dim3(1024), 0, s, cost, bins, order, wg_list, hdr, n, light_below, floor_below, pack,
                       judge, champion);
    return hipGetLastError();
}

namespace dev {
__global__ __launch_bounds__(64) void k_stamp(unsigned long long *stamp) {
    if (threadIdx.x == 0u) *stamp = __builtin_amdgcn_s_memrealtime();
}
}  // namespace dev

hipError_t launch_stamp(uint32_t *judge, hipStream_t s) {
    if (judge == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_stamp, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned long long *>(judge + kJudgeStampLo));
    return hipGetLastError();
}

// Keep or take (order_judge.hpp), behind the first frame of a newly sorted list.  One workgroup: the two sets of lists of a 1080p
// frame are 260 KB each, and a rejected challenger is the rarer case.  Thread 0 reads the clock before anything else, so the score
// ends where the champion's does: at the start of the kernel behind the frame.
namespace dev {
__global__ __launch_bounds__(1024) void k_judge_order(uint32_t *judge, uint32_t *read_set, const uint32_t *other_set, uint32_t words, int force) {
    __shared__ uint32_t take_sh;
    if (threadIdx.x == 0u) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        const unsigned long long t0 = *reinterpret_cast<const unsigned long long *>(judge + kJudgeStampLo);
        const Verdict v = judge_order({judge[kJudgeChampion], judge_score(t0, now)}, force);
        judge[kJudgeChampion] = v.after.champion;
        judge[kJudgeChallenger] = v.after.challenger;
        judge[v.take ? kJudgeTaken : kJudgeRejected] += 1u;
        take_sh = v.take ? 1u : 0u;
    }
    __syncthreads();
    if (take_sh != 0u) return;
    // the champion's lists back into the set the frames read: 16 bytes per thread and step where both runs allow it
    uint32_t done = 0u;
    if (((reinterpret_cast<uintptr_t>(read_set) | reinterpret_cast<uintptr_t>(other_set)) & 15u) == 0u) {
        const uint32_t quads = words >> 2;
        const uint4 *src = reinterpret_cast<const uint4 *>(other_set);
        uint4 *dst = reinterpret_cast<uint4 *>(read_set);
        constexpr uint32_t kBatch = 4;                                      // loads in flight per thread: one workgroup waits for latency
        for (uint32_t base = 0; base < quads; base += blockDim.x * kBatch) {
            uint4 v[kBatch];
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k) {
                const uint32_t i = base + k * blockDim.x + threadIdx.x;
                if (i < quads) v[k] = src[i];
            }
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k) {
                const uint32_t i = base + k * blockDim.x + threadIdx.x;
                if (i < quads) dst[i] = v[k];
            }
        }
        done = quads << 2;
    }
    for (uint32_t i = done + threadIdx.x; i < words; i += blockDim.x) read_set[i] = other_set[i];
}
}  // namespace dev

hipError_t launch_judge_order(uint32_t *judge, uint32_t *read_set, const uint32_t *other_set, uint32_t words, int force, hipStream_t s) {
    if (judge == nullptr || read_set == nullptr || other_set == nullptr || read_set == other_set) return hipErrorInvalidValue;
    if (words == 0u) return hipSuccess;
    hipLaunchKernelGGL(dev::k_judge_order, dim3(1), dim3(1024), 0, s, judge, read_set, other_set, words, force);
    return hipGetLastError();
}

hipError_t launch_camera_rays(const dev::RenderArgs &A, int sample, rtk_ray *d_rays, hipStream_t s) {
    const size_t n = (size_t)A.width * A.height;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_camera_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, sample, d_rays);
    return hipGetLastError();
}

hipError_t launch_region_rays(const dev::RenderArgs &A, int sample, uint64_t first, uint32_t n, rtk_ray *d_rays, uint32_t *d_ids, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    if (A.regions == nullptr || A.n_regions == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_region_rays, dim3((n + 255u) / 256u), dim3(256), 0, s, A, sample, first, n, d_rays, d_ids);
    return hipGetLastError();
}

hipError_t launch_region_accumulate(const dev::RenderArgs &A, uint64_t first, uint32_t n, const float *d_rgb, bool start, bool divide, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    if (A.regions == nullptr || A.n_regions == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_region_accumulate, dim3((n + 255u) / 256u), dim3(256), 0, s, A, first, n, d_rgb, start ? 1 : 0, divide ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_add_word(unsigned long long *dst, const unsigned long long *src, hipStream_t s) {
    hipLaunchKernelGGL(dev::k_add_word, dim3(1), dim3(64), 0, s, dst, src);
    return hipGetLastError();
}

hipError_t launch_frame_to_texels(const float *d_rgb, size_t n, uint8_t *d_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t threads = n / 12u + 1u;                                    // (at most the groups, and the one behind them)
    hipLaunchKernelGGL(dev::k_frame_to_texels, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, d_rgb, n, d_out);
    return hipGetLastError();
}

hipError_t launch_to_rgb8(const float *d_rgb, size_t n, uint8_t *d_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_to_rgb8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_rgb, n, d_out);
    return hipGetLastError();
}

hipError_t launch_assemble(const dev::AssembleArgs &A, hipStream_t s) {
    const size_t n = (size_t)A.width * A.height;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_assemble, dim3(blocks), dim3(256), 0, s, A);
    return hipGetLastError();
}

}  // namespace rtk
