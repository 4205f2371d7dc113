// C-ABI, rtk_render_regions: rectangles of a frame, as launches of the megakernel over their blocks or, on the streaming path,
// as radiance batches of their camera rays.  The plan of a call (what a rectangle may be, the table, the launches) is regions_plan.hpp.
#include <cstring>
#include <mutex>
#include <string>

#include "render_internal.hpp"

using namespace rtk;

namespace {

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
        rtk_radiance_params rp = frame_radiance_params(p);
        RTK_HIP(zero_counters(a, s));
        for (const RegionLaunch &L : P.launches) {
            A.regions = a->rg_table.get() + L.first_entry; A.n_regions = L.n_entries; A.n_units = L.n_units;
            for (uint64_t first = 0; first < L.n_pixels; first += chunk) {
                const uint32_t cn = uint32_t(L.n_pixels - first < chunk ? L.n_pixels - first : chunk);
                for (int smp = g.sample_begin; smp < g.sample_end; ++smp) {
                    RTK_HIP_AS(launch_region_rays(A, smp, first, cn, a->rg_rays.get(), a->rg_ids.get(), s), "launch k_region_rays");
                    rp.sample = smp;
                    RTK_TRY(radiance_frame_chunk(a, a->rg_rays.get(), a->rg_ids.get(), cn, &rp, a->rg_rgb.get(), s));
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

extern "C" {

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
            HostStage &st = a->stage;
            StageLayout L;
            const int o_rgb = L.add(packed ? pixels * 3 : uint64_t(g.width) * g.height * 3);
            RTK_MEM(st.reserve(L));
            if (!packed || p->sample_begin > 0) RTK_HIP(st.upload(o_rgb, rgb));
            RTK_TRY(render_regions_impl(a, p, g, rects, n_rects, layout, st.at<float>(o_rgb), nullptr));
            RTK_HIP(st.download(o_rgb, rgb));
        }
        if (counters) return rtk_render_last_counters(a, counters);
        return RTK_OK;
    });
}

}  // extern "C"
