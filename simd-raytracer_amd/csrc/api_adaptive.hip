// C-ABI, rtk_render_adaptive: a frame whose 8x8 pixel blocks stop taking samples once their noise estimate is under the caller's
// threshold.  The arithmetic of the call -- refusals, checkpoints, the chunk walk, the count word -- is adaptive_plan.hpp; the
// kernels are adaptive.hip; the colours come from the streaming pipeline of rtk_accel_radiance (radiance_frame_chunk), as on the
// streaming path of rtk_render_regions.  Nothing here touches the accel's camera, its cost tables, the regions table or
// RTK_TRACE_AUTO's verdict; the counters are the call's, as after a regions call.
#include <cstring>
#include <mutex>

#include "adaptive.hpp"
#include "render_internal.hpp"

using namespace rtk;

namespace {

// everything the call refuses, in the order rtk.h gives; on RTK_OK `g` is the frame's geometry
int adaptive_check(const rtk_accel *a, const rtk_render_params *p, const rtk_adaptive_params *ap, const void *rgb, FrameGeom &g) {
    if (!a || !p || !ap || !rgb) return fail(RTK_ERR_INVALID, "null accel, params, adaptive params or rgb");
    RTK_TRY(frame_geom(a, p, g));
    if (const char *why = adaptive_refusal(*p, *ap, g.width, g.height)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

// Room for a frame of `pixels` pixels and `blocks` blocks walked in chunks of at most `chunk` pixels.  Growing frees what a call
// on another stream may still use, so the device is idle first.
int ensure_adaptive_ws(rtk_accel *a, size_t pixels, size_t blocks, size_t chunk) {
    RTK_MEM(a->ad_count.reserve(1));
    RTK_MEM(a->ad_count_host.reserve(1));
    if (a->ad_s1.capacity() >= pixels && a->ad_s2.capacity() >= pixels && a->ad_list.capacity() >= 2 * pixels &&
        a->ad_blocks.capacity() >= 2 * blocks && a->ad_rays.capacity() >= chunk && a->ad_rgb.capacity() >= 3 * chunk) return RTK_OK;
    RTK_HIP(hipDeviceSynchronize());
    RTK_MEM(a->ad_s1.reserve(pixels, grow_half<0>()));
    RTK_MEM(a->ad_s2.reserve(pixels, grow_half<0>()));
    RTK_MEM(a->ad_list.reserve(2 * pixels, grow_half<0>()));
    RTK_MEM(a->ad_blocks.reserve(2 * blocks, grow_half<0>()));
    RTK_MEM(a->ad_rays.reserve(chunk, grow_half<0>()));
    RTK_MEM(a->ad_rgb.reserve(3 * chunk, grow_half<0>()));
    return RTK_OK;
}

}  // namespace

// The rounds of a call.  Everything is enqueued on `s`; the host waits once per round that is not the last, for the count word.
// (api_frame_noise.hip redoes a call whose queues overflowed through this)
int rtk::adaptive_device_impl(rtk_accel *a, const rtk_render_params *p, const rtk_adaptive_params *ap, const FrameGeom &g, float *d_rgb,
                         uint32_t *d_samples, float *d_noise, hipStream_t s) {
    const uint64_t pixels = uint64_t(g.width) * g.height, blocks = adaptive_blocks(g.width, g.height);
    const uint64_t chunk = a->knobs.adaptive_chunk_pixels;
    RTK_TRY(ensure_adaptive_ws(a, size_t(pixels), size_t(blocks), size_t(adaptive_chunk_capacity(pixels, chunk))));
    RTK_HIP(a->ad_last.wait_previous(s));

    // the camera half of a frame's arguments with spp = the ceiling, as rtk_camera_rays makes them: all k_adaptive_rays reads
    dev::RenderArgs A;
    std::memset(&A, 0, sizeof(A));
    camera_args(accel_camera(a), p, g, A);
    rtk_radiance_params rp = frame_radiance_params(p);

    uint32_t *const list[2] = {a->ad_list.get(), a->ad_list.get() + pixels};
    uint32_t *const blist[2] = {a->ad_blocks.get(), a->ad_blocks.get() + blocks};
    dev::AdaptiveDecide D;
    std::memset(&D, 0, sizeof(D));
    D.width = g.width; D.height = g.height;
    D.threshold = double(ap->threshold); D.floor = double(ap->floor);
    D.rgb = d_rgb; D.s1 = a->ad_s1.get(); D.s2 = a->ad_s2.get(); D.samples = d_samples; D.noise = d_noise;
    D.count = a->ad_count.get();

    RTK_HIP(zero_counters(a, s));
    // the first list: every block of the frame, in frame order
    int cur = 0;
    D.blocks = nullptr; D.n_blocks = uint32_t(blocks); D.next_blocks = blist[cur]; D.next_list = list[cur];
    RTK_HIP_AS(launch_adaptive_decide(D, s), "launch k_adaptive_decide");
    uint64_t active = pixels, active_blocks = blocks, primary = 0;
    int32_t done = 0, next = adaptive_next_checkpoint(0, p->spp, ap->min_samples, ap->step);
    while (active > 0) {
        // within a chunk all of the round's samples run in order before the next chunk, as in render_regions_impl
        for (AdaptiveChunks c(active, chunk); !c.done(); c.next()) {
            const uint32_t *const ids = list[cur] + c.first;         // frame pixel indices: the ids of the radiance batch as they are
            const uint32_t cn = c.n();
            for (int32_t smp = done; smp < next; ++smp) {
                RTK_HIP_AS(launch_adaptive_rays(A, smp, ids, cn, a->ad_rays.get(), s), "launch k_adaptive_rays");
                rp.sample = smp;
                RTK_TRY(radiance_frame_chunk(a, a->ad_rays.get(), ids, cn, &rp, a->ad_rgb.get(), s));
                RTK_HIP_AS(launch_adaptive_accumulate(ids, cn, a->ad_rgb.get(), d_rgb, a->ad_s1.get(), a->ad_s2.get(), pixels, smp == 0, s),
                           "launch k_adaptive_accumulate");
            }
        }
        primary += active * uint64_t(next - done);
        const bool last = next == p->spp;
        if (!last) RTK_HIP(hipMemsetAsync(a->ad_count.get(), 0, sizeof(unsigned long long), s));
        D.blocks = blist[cur]; D.n_blocks = uint32_t(active_blocks); D.n = next; D.last = last ? 1 : 0;
        D.next_blocks = blist[cur ^ 1]; D.next_list = list[cur ^ 1];
        RTK_HIP_AS(launch_adaptive_decide(D, s), "launch k_adaptive_decide");
        if (last) break;                                             // (every block is finished: nothing to read back)
        RTK_HIP(hipMemcpyAsync(a->ad_count_host.get(), a->ad_count.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        RTK_HIP(hipStreamSynchronize(s));
        const uint64_t word = *a->ad_count_host.get();
        active = ad_count_pixels(word); active_blocks = ad_count_blocks(word);
        if (active > pixels || active_blocks > blocks) return fail(RTK_ERR_HIP, "adaptive render: the count word is out of range");
        cur ^= 1;
        done = next; next = adaptive_next_checkpoint(done, p->spp, ap->min_samples, ap->step);
    }
    RTK_HIP(a->ad_last.record(s));
    record_last(a, s, false, primary);
    return RTK_OK;
}

int rtk_render_adaptive_device(rtk_accel *a, const rtk_render_params *p, const rtk_adaptive_params *ap, float *d_rgb, uint32_t *d_samples,
                               float *d_noise, void *stream) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        RTK_TRY(adaptive_check(a, p, ap, d_rgb, g));
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return adaptive_device_impl(a, p, ap, g, d_rgb, d_samples, d_noise, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_adaptive(rtk_accel *a, const rtk_render_params *p, const rtk_adaptive_params *ap, float *rgb, uint32_t *samples, float *noise,
                        rtk_counters *counters) {
    return abi_guard([&]() -> int {
        FrameGeom g;
        RTK_TRY(adaptive_check(a, p, ap, rgb, g));
        {
            std::lock_guard<std::mutex> lock(a->mu);
            RTK_TRY(ensure_device(a));
            // rgb, samples and noise: all three are written on the device, whichever of them the caller wants back
            const uint64_t n = uint64_t(g.width) * g.height;
            HostStage &st = a->stage;
            StageLayout L;
            const int o_rgb = L.add(n * 3), o_samples = L.add(n), o_noise = L.add(n);
            RTK_MEM(st.reserve(L));
            RTK_TRY(adaptive_device_impl(a, p, ap, g, st.at<float>(o_rgb), st.at<uint32_t>(o_samples), st.at<float>(o_noise), nullptr));
            // (a copy on the null stream is behind the kernels and blocks the host)
            RTK_HIP(st.download(o_rgb, rgb));
            if (samples) RTK_HIP(st.download(o_samples, samples));
            if (noise) RTK_HIP(st.download(o_noise, noise));
        }
        if (counters) return rtk_render_last_counters(a, counters);
        return RTK_OK;
    });
}
