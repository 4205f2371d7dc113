// C-ABI, ray batches that need no shading: batched intersect (with the ray repacking of repack.hip) and batched occlusion.
#include <cmath>
#include <mutex>

#include "accel.hpp"
#include "batch_plan.hpp"
#include "repack.hpp"
#include "occluded.hpp"

using namespace rtk;

// ---------------------------------------------------------------- batched intersect

// workspace of the ray repacking: keys and indices (double-buffered for the sort), rocPRIM's temporary storage; grows, never shrinks
static int ensure_repack_ws(rtk_accel *a, size_t n) {
    RTK_MEM(a->rp_bounds.reserve(kRepackBoundsAlloc));
    if (a->rp_temp.get() && a->rp_keys.capacity() >= 2 * n && a->rp_idx.capacity() >= 2 * n) return RTK_OK;
    // re-made as a group, rp_temp last: it is there only while all three were made by one call, for one n (a call that failed
    // part-way leaves it empty, and the next call starts over)
    a->rp_keys.reset(); a->rp_idx.reset(); a->rp_temp.reset();
    size_t tb = 0;
    RTK_HIP(repack_temp_bytes(n, &tb));
    RTK_MEM(a->rp_keys.reserve(2 * n));
    RTK_MEM(a->rp_idx.reserve(2 * n));
    RTK_MEM(a->rp_temp.reserve(tb > 0 ? tb : 16));
    a->rp_temp_bytes = tb;
    return RTK_OK;
}

static int intersect_device_impl(rtk_accel *a, const rtk_ray *d_rays, size_t n, int cull, int mode, rtk_hit *d_out,
                                 hipStream_t s, bool stats) {
    if (!valid_batch_mode(mode)) return fail(RTK_ERR_INVALID, "unknown trace_mode");
    if (n > (size_t(1) << 38)) return fail(RTK_ERR_INVALID, "too many rays for one launch");
    if (n > 0 && (!d_rays || !d_out)) return fail(RTK_ERR_INVALID, "null ray or hit buffer");
    if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0) return fail(RTK_ERR_INVALID, "hit buffer must be 16-byte aligned");
    dev::IntersectArgs A;
    A.tree = tree_view(a);
    A.rays = d_rays; A.out = d_out; A.n = n; A.cull = cull ? 1 : 0; A.counters = counters_now(a); A.perm = nullptr; A.raster_w = 0u; A.verdict = nullptr;
    A.tree.scalar_surv = a->knobs.batch_scalar_surv ? 1 : 0;
    // Ray repacking (repack.hip).  Large batches are probed first (every 16th wave; one stream synchronisation): waves that are
    // coherent as they come are walked wave-cooperatively; a batch in no useful order is sorted by origin / direction cell and
    // then walked wave-cooperatively when the sort makes tight waves (three varying dimensions: 10 bits each), with the per-lane
    // fallback when it cannot (six: 5 bits each).  4 M rays on scene5: shuffled camera rays 4.5 -> 0.47 ms, uniform secondary
    // rays 11.3 -> 4.1 ms, camera rays in pixel order 0.8 (RTK_TRACE_AUTO before) -> 0.3 ms.
    // (the arithmetic of these decisions: batch_plan.hpp)
    const BatchKnobs bk = {a->knobs.repack, a->knobs.repack_full_bounds, a->knobs.repack_skip_bits, a->knobs.repack_skip_bits2, a->knobs.repack_trace};
    const BatchPlan plan = plan_batch(n, mode, stats, bk);
    mode = plan.mode;
    if (plan.workspace) {
        RTK_TRY(ensure_repack_ws(a, n));
        // The workspace (bounds, keys, permutation) belongs to the accel: a batch on another stream may still be walking the
        // permutation of the previous call.  Its k_intersect recorded rp_last; this stream waits for it before it rewrites anything.
        RTK_HIP(a->rp_last.wait_previous(s));
        hipError_t eb = hipSuccess;
        uint32_t sort_word = 0u, dims_word = 0u;
        if (plan.probe) {
            // AUTO: the probe's verdict is needed on the host (one stream synchronisation; RTK_TRACE_REPACK and RTK_REPACK=0 never block)
            // The verdict is made on the device (k_raster_probe) and needed on the host; while it travels, the launch a coherent
            // batch needs is already under way -- it reads the same verdict and does nothing if the batch is to be sorted.
            unsigned fold = 0;
            eb = launch_ray_bounds(d_rays, n, a->rp_bounds.get(), plan.probe_stride, true, s, &fold);
            if (eb == hipSuccess) eb = launch_raster_probe(d_rays, n, a->rp_bounds.get(), a->knobs.raster_tiles, s, fold, a->knobs.repack_dirs3);
            if (eb != hipSuccess) return hip_fail(eb, "launch k_ray_bounds (probe)");
            RTK_MEM(a->rp_host.reserve(kRepackBoundsWords));
            RTK_MEM(a->rp_probe_ev.ensure());
            const uint32_t *const rp_host = a->rp_host.get();
            RTK_HIP(hipMemcpyAsync(a->rp_host.get(), a->rp_bounds.get(), kRepackBoundsWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            RTK_HIP(hipEventRecord(a->rp_probe_ev.get(), s));
            dev::IntersectArgs Spec = A;
            Spec.verdict = a->rp_bounds.get();
            RTK_HIP_AS(launch_intersect(Spec, RTK_TRACE_WAVE, false, s), "launch k_intersect");
            // ... and so are the keys a batch to be sorted needs (k_ray_keys returns at once if it is not): the verdict's trip to the
            // host and the launches that follow it no longer leave the stream idle
            if (plan.keys_ahead) {
                eb = launch_ray_keys(d_rays, n, a->rp_bounds.get(), a->rp_keys.get(), a->rp_idx.get(), s, a->knobs.repack_dirs3, true);
                if (eb != hipSuccess) return hip_fail(eb, "launch k_ray_keys");
            }
            RTK_HIP(a->rp_last.record(s));                                        // (both read the workspace's verdict words)
            RTK_HIP(hipEventSynchronize(a->rp_probe_ev.get()));                   // the verdict, not the trace
            sort_word = rp_host[16]; dims_word = rp_host[17];
        }
        const SortPlan sp = plan_sort(plan, sort_word, dims_word, bk);
        if (!sp.sort) return RTK_OK;                                         // coherent as it comes: the probe's launch was the batch
        // The cells of the sort keys lie in the bounds of a SAMPLE of the batch (the probe's, where there was one; ~4,096 waves
        // otherwise): a ray outside them lands in a border cell -- an order a little worse for it, never another result -- and a
        // pass over all rays (0.13 ms of a 2^24-ray batch's 1.8) is saved.
        if (sp.rebound) eb = launch_ray_bounds(d_rays, n, a->rp_bounds.get(), sp.bounds_stride, false, s);
        if (eb == hipSuccess && !plan.keys_ahead) eb = launch_ray_keys(d_rays, n, a->rp_bounds.get(), a->rp_keys.get(), a->rp_idx.get(), s, a->knobs.repack_dirs3, false);
        if (eb == hipSuccess) eb = launch_key_sort(n, a->rp_keys.get(), a->rp_idx.get(), a->rp_temp.get(), a->rp_temp_bytes, s, sp.sort_from_bit);
        if (eb != hipSuccess) return hip_fail(eb, "ray repacking");
        A.perm = a->rp_idx.get() + n;
        mode = sp.mode;
    }
    RTK_HIP_AS(launch_intersect(A, mode, stats, s), "launch k_intersect");
    if (A.perm != nullptr) RTK_HIP(a->rp_last.record(s));
    return RTK_OK;
}

int rtk_accel_intersect_device(rtk_accel *a, const rtk_ray *d_rays, size_t n, int cull, int mode, rtk_hit *d_out, void *stream) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return intersect_device_impl(a, d_rays, n, cull, mode, d_out, static_cast<hipStream_t>(stream), false);
    });
}

int rtk_accel_intersect_stats(rtk_accel *a, const rtk_ray *d_rays, size_t n, int cull, int mode, rtk_hit *d_out,
                              rtk_counters *counters) {
    return abi_guard([&]() -> int {
        if (!a || !counters) return fail(RTK_ERR_INVALID, "null accel or counters");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        a->cnt.forget();                                                    // (a user of the counters that is no steady frame: frame_plan.hpp CounterState)
        RTK_HIP(hipMemsetAsync(counters_now(a), 0, kCounterWords * sizeof(unsigned long long), nullptr));
        RTK_TRY(intersect_device_impl(a, d_rays, n, cull, mode, d_out, nullptr, true));
        unsigned long long h[kRayShardWord];
        RTK_HIP(hipMemcpy(h, counters_now(a), sizeof(h), hipMemcpyDeviceToHost));
        counters_from_block(h, true, counters);
        return RTK_OK;
    });
}

int rtk_accel_intersect(rtk_accel *a, const rtk_ray *rays, size_t n, int cull, int mode, rtk_hit *out) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        if (n > 0 && (!rays || !out)) return fail(RTK_ERR_INVALID, "null ray or hit buffer");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        if (n == 0) return RTK_OK;
        HostStage stage;                             // (the call's own: freed when it returns)
        StageLayout L;
        const int i_rays = L.add(uint64_t(n) * (sizeof(rtk_ray) / 4)), o_hits = L.add(uint64_t(n) * (sizeof(rtk_hit) / 4));
        RTK_MEM(stage.reserve(L));
        RTK_HIP_AS(stage.upload(i_rays, rays), "intersect copy");
        RTK_TRY(intersect_device_impl(a, stage.at<rtk_ray>(i_rays), n, cull, mode, stage.at<rtk_hit>(o_hits), nullptr, false));
        RTK_HIP_AS(stage.download(o_hits, out), "intersect copy");
        return RTK_OK;
    });
}

// ---------------------------------------------------------------- batched occlusion

// (the host variant counts its closest-hit queries in kOccludedCountWord, behind the frame counters: those of the most recent
// frame, rtk_render_last_counters, stay as that frame left them)

static int occluded_check(const rtk_accel *a, const void *rays, const void *max_t, size_t n, float shadow_bias, int mode, const void *out) {
    if (!a) return fail(RTK_ERR_INVALID, "null accel");
    if (!valid_mode(mode)) return fail(RTK_ERR_INVALID, "trace_mode of an occlusion batch must be RTK_TRACE_AUTO, RTK_TRACE_LANE or RTK_TRACE_WAVE");
    if (!std::isfinite(shadow_bias)) return fail(RTK_ERR_INVALID, "shadow_bias must be finite");
    if (n > (size_t(1) << 38)) return fail(RTK_ERR_INVALID, "too many queries for one launch");
    if (n > 0 && (!rays || !max_t || !out)) return fail(RTK_ERR_INVALID, "null ray, max_t or answer buffer");
    return RTK_OK;
}

static int occluded_launch(rtk_accel *a, const rtk_ray *d_rays, const float *d_max_t, size_t n, float shadow_bias, int mode,
                           uint8_t *d_out, hipStream_t s, bool count) {
    dev::OccludedArgs A;
    A.tree = tree_view(a);
    A.tree.scalar_surv = a->knobs.batch_scalar_surv ? 1 : 0;
    A.materials = a->d_materials.get();
    A.rays = d_rays; A.max_t = d_max_t; A.out = d_out; A.n = n;
    A.shadow_bias = shadow_bias;
    A.has_refractive = a->has_refractive ? 1 : 0;
    A.n_intersect = count ? counters_now(a) + kOccludedCountWord : nullptr;
    RTK_HIP_AS(launch_occluded(A, mode, s), "launch k_occluded");
    return RTK_OK;
}

int rtk_accel_occluded_device(rtk_accel *a, const rtk_ray *d_rays, const float *d_max_t, size_t n, float shadow_bias, int mode,
                              uint8_t *d_out, void *stream) {
    return abi_guard([&]() -> int {
        RTK_TRY(occluded_check(a, d_rays, d_max_t, n, shadow_bias, mode, d_out));
        if (n == 0) return RTK_OK;
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return occluded_launch(a, d_rays, d_max_t, n, shadow_bias, mode, d_out, static_cast<hipStream_t>(stream), false);
    });
}

int rtk_accel_occluded(rtk_accel *a, const rtk_ray *rays, const float *max_t, size_t n, float shadow_bias, int mode, uint8_t *out,
                       uint64_t *n_intersections) {
    return abi_guard([&]() -> int {
        RTK_TRY(occluded_check(a, rays, max_t, n, shadow_bias, mode, out));
        if (n == 0) {
            if (n_intersections) *n_intersections = 0;
            return RTK_OK;
        }
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        HostStage &st = a->stage;
        StageLayout L;
        const int i_rays = L.add(uint64_t(n) * (sizeof(rtk_ray) / 4)), i_max_t = L.add(n), o_out = L.add_bytes(n);
        RTK_MEM(st.reserve(L));
        RTK_HIP(st.upload(i_rays, rays));
        RTK_HIP(st.upload(i_max_t, max_t));
        if (n_intersections) {
            a->cnt.forget();
            RTK_HIP(hipMemsetAsync(counters_now(a) + kOccludedCountWord, 0, sizeof(unsigned long long), nullptr));
        }
        RTK_TRY(occluded_launch(a, st.at<rtk_ray>(i_rays), st.at<float>(i_max_t), n, shadow_bias, mode, st.at<uint8_t>(o_out), nullptr, n_intersections != nullptr));
        RTK_HIP(st.download(o_out, out));
        if (n_intersections) {
            unsigned long long h = 0;
            RTK_HIP(hipMemcpy(&h, counters_now(a) + kOccludedCountWord, sizeof(h), hipMemcpyDeviceToHost));
            *n_intersections = h;
        }
        return RTK_OK;
    });
}
