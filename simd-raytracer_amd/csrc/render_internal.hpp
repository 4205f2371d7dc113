// Internal to the host files that shade (api_frame, api_stream, api_order, api_views, api_regions, api_radiance, api_gbuffer,
// api_gbuffer_specular, api_adaptive, api_frame_noise .hip): what one of them defines and another calls, grouped by the file that defines it.
#pragma once

#include "accel.hpp"

namespace rtk {

// ---- api_frame.hip
int frame_geom(const rtk_accel *a, const rtk_render_params *p, FrameGeom &g);
size_t out_pixels(const FrameGeom &g);                                                           // output pixels of this rank
uint64_t primary_rays_of_rank(const FrameGeom &g);                                               // pixels of its buckets x samples of this call
dev::RenderArgs scene_args(const rtk_accel *a, int stats_mode);                                  // what a frame and a radiance batch share
rtk_view accel_camera(const rtk_accel *a);                                                       // the camera later frames are rendered from
void camera_args(const rtk_view &cam, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A);   // the camera half of the launch arguments
dev::RenderArgs frame_args(const rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view &cam, float *d_out);
hipError_t zero_counters(rtk_accel *a, hipStream_t s);                                           // the block in use starts at zero; no steady frame behind it
void record_last(rtk_accel *a, hipStream_t s, bool stats, uint64_t primary);                     // what rtk_render_last_counters goes by
int render_frame_impl(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const rtk_view &cam, float *d_out, hipStream_t s,
                      bool steady);                                                              // one frame seen from `cam`

// ---- api_stream.hip
// the workspace (accel.hpp StreamWorkspace: an accel's is a->stream) ...
void free_stream_ws(StreamWorkspace &w);
int ensure_stream_ws(StreamWorkspace &w, int device, size_t pixels, size_t nodes, size_t lights, bool need_sum, int lanes);
int claim_stream_ws(StreamWorkspace &w, hipStream_t s);                                          // the queues' previous user finishes first, on the device
int release_stream_ws(StreamWorkspace &w, hipStream_t s);
int fork_lanes(StreamWorkspace &w, int lanes, hipStream_t s);                                    // lanes 1.. start behind everything enqueued on `s`
int join_lanes(StreamWorkspace &w, int lanes, hipStream_t s);                                    // `s` continues behind every lane's last launch
// ... and the pipeline's setup, for all of its clients
struct StreamSetup {
    dev::StreamArgs S;
    int deep_level, deep_mode, sort_from, slices;      // launch_stream_sample's
    size_t factor, node_bytes, budget;                 // stream_plan.hpp's
};
StreamSetup stream_args(const rtk_accel *a, const dev::RenderArgs &A, int diffuse_rays, bool forks);
// The launches of a streamed frame with arguments `A`, from the plan to the overflow reset, on `s` and the lanes; a->stream is
// claimed and the caller owns the tail: what becomes of an overflow (lane 0's word), then release_stream_ws.  `need_sum`: the
// workspace has a sum buffer; `trial`: RTK_TRACE_AUTO's {start, end} or null; `M`: the statistic beside the sums, or none.
int launch_stream_frame(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const dev::RenderArgs &A, bool forks, bool need_sum,
                        hipEvent_t trial[2], const StreamMoments &M, hipStream_t s);
int render_stream(rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, const dev::RenderArgs &A, bool forks, bool general,
                  hipEvent_t trial[2], hipStream_t s);

// ---- api_order.hip
int render_megakernel(rtk_accel *a, rtk_cost_feedback &fb, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A, bool general,
                      hipStream_t s);

// ---- the launches of a views or a regions call (api_views.hip, api_regions.hip); here because render_parts is a template
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

// ---- api_radiance.hip
int radiance_device_impl(rtk_accel *a, const rtk_ray *d_rays, const uint32_t *d_ids, size_t n, const rtk_radiance_params *p,
                         float *d_rgb, hipStream_t s, uint32_t *n_chunks_out);                   // rtk_accel_radiance_device behind its checks
// the settings of the batches a frame's own camera rays go through (regions' streaming path, the adaptive render); `sample` is the caller's to set
rtk_radiance_params frame_radiance_params(const rtk_render_params *p);
// one sample of one chunk of such a call: the batch, then its rays added to the call's counters
int radiance_frame_chunk(rtk_accel *a, const rtk_ray *d_rays, const uint32_t *d_ids, size_t n, const rtk_radiance_params *rp, float *d_rgb,
                         hipStream_t s);

// ---- api_gbuffer.hip
// what a g-buffer kernel reads of zeroed launch arguments besides its units (gbuffer.hpp GbufferArgs::r): the tree as the batched
// intersect walks it, materials, textures, background and the camera half; for rtk_render_gbuffer and rtk_render_gbuffer_specular
void gbuffer_scene_args(const rtk_accel *a, const rtk_render_params *p, const FrameGeom &g, dev::RenderArgs &A);

// ---- api_adaptive.hip
int adaptive_device_impl(rtk_accel *a, const rtk_render_params *p, const rtk_adaptive_params *ap, const FrameGeom &g, float *d_rgb,
                         uint32_t *d_samples, float *d_noise, hipStream_t s);                    // rtk_render_adaptive_device behind its checks

}  // namespace rtk
