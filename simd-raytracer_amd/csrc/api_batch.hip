// C-ABI, ray batches that need no shading: batched intersect (with the ray repacking of repack.hip) and batched occlusion.
#include <cmath>
#include <mutex>

#include "accel.hpp"
#include "repack.hpp"
#include "occluded.hpp"

using namespace rtk;

// ---------------------------------------------------------------- batched intersect

// workspace of the ray repacking: keys and indices (double-buffered for the sort), rocPRIM's temporary storage; grows, never shrinks
static int ensure_repack_ws(rtk_accel *a, size_t n) {
    if (!a->rp_bounds) RTK_HIP(hipMalloc(reinterpret_cast<void **>(&a->rp_bounds), kRepackBoundsAlloc * sizeof(uint32_t)));
    if (a->rp_cap >= n) return RTK_OK;
    (void)hipFree(a->rp_keys); (void)hipFree(a->rp_idx); (void)hipFree(a->rp_temp);
    a->rp_keys = a->rp_idx = nullptr; a->rp_temp = nullptr; a->rp_cap = 0;
    size_t tb = 0;
    RTK_HIP(repack_temp_bytes(n, &tb));
    RTK_HIP(hipMalloc(reinterpret_cast<void **>(&a->rp_keys), 2 * n * sizeof(uint32_t)));
    RTK_HIP(hipMalloc(reinterpret_cast<void **>(&a->rp_idx), 2 * n * sizeof(uint32_t)));
    RTK_HIP(hipMalloc(&a->rp_temp, tb > 0 ? tb : 16));
    a->rp_temp_bytes = tb; a->rp_cap = n;
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
    A.rays = d_rays; A.out = d_out; A.n = n; A.cull = cull ? 1 : 0; A.counters = a->d_counters; A.perm = nullptr; A.raster_w = 0u; A.verdict = nullptr;
    A.tree.scalar_surv = a->knobs.batch_scalar_surv ? 1 : 0;
    // Ray repacking (repack.hip).  Large batches are probed first (every 16th wave; one stream synchronisation): waves that are
    // coherent as they come are walked wave-cooperatively; a batch in no useful order is sorted by origin / direction cell and
    // then walked wave-cooperatively when the sort makes tight waves (three varying dimensions: 10 bits each), with the per-lane
    // fallback when it cannot (six: 5 bits each).  4 M rays on scene5: shuffled camera rays 4.5 -> 0.47 ms, uniform secondary
    // rays 11.3 -> 4.1 ms, camera rays in pixel order 0.8 (RTK_TRACE_AUTO before) -> 0.3 ms.
    const bool big = n >= (size_t(1) << 18) && n < (size_t(1) << 32);
    const bool forced = mode == RTK_TRACE_REPACK;
    if (forced) mode = RTK_TRACE_AUTO;
    const bool sortable = !stats && n >= 2 && n < (size_t(1) << 32);
    const bool probe = !stats && !forced && mode == RTK_TRACE_AUTO && a->knobs.repack && big;
    if ((forced && sortable) || probe) {
        RTK_TRY(ensure_repack_ws(a, n));
        // The workspace (bounds, keys, permutation) belongs to the accel: a batch on another stream may still be walking the
        // permutation of the previous call.  Its k_intersect recorded rp_done; this stream waits for it before it rewrites anything.
        if (a->rp_done == nullptr) RTK_HIP(hipEventCreateWithFlags(&a->rp_done, hipEventDisableTiming));
        if (a->rp_in_use) RTK_HIP(hipStreamWaitEvent(s, a->rp_done, 0));
        hipError_t eb = hipSuccess;
        bool sort = forced;
        unsigned sort_from_bit = 0u;
        bool keys_made = false;
        int sorted_mode = RTK_TRACE_AUTO;                                    // any order: wave-cooperative with the per-lane fallback
        if (probe) {
            // AUTO: the probe's verdict is needed on the host (one stream synchronisation; RTK_TRACE_REPACK and RTK_REPACK=0 never block)
            // The verdict is made on the device (k_raster_probe) and needed on the host; while it travels, the launch a coherent
            // batch needs is already under way -- it reads the same verdict and does nothing if the batch is to be sorted.
            const uint32_t probe_stride = uint32_t(((n + 63) / 64 + 4095) / 4096 > 16 ? ((n + 63) / 64 + 4095) / 4096 : 16);   // ~4,096 waves looked at
            unsigned fold = 0;
            eb = launch_ray_bounds(d_rays, n, a->rp_bounds, probe_stride, true, s, &fold);
            if (eb == hipSuccess) eb = launch_raster_probe(d_rays, n, a->rp_bounds, a->knobs.raster_tiles, s, fold);
            if (eb != hipSuccess) return hip_fail(eb, "launch k_ray_bounds (probe)");
            if (!a->rp_host) {
                RTK_HIP(hipHostMalloc(reinterpret_cast<void **>(&a->rp_host), kRepackBoundsWords * sizeof(uint32_t), hipHostMallocDefault));
                RTK_HIP(hipEventCreateWithFlags(&a->rp_probe_ev, hipEventDisableTiming));
            }
            RTK_HIP(hipMemcpyAsync(a->rp_host, a->rp_bounds, kRepackBoundsWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            RTK_HIP(hipEventRecord(a->rp_probe_ev, s));
            dev::IntersectArgs Spec = A;
            Spec.verdict = a->rp_bounds;
            RTK_HIP_AS(launch_intersect(Spec, RTK_TRACE_WAVE, false, s), "launch k_intersect");
            a->rp_in_use = true;
            // ... and so are the keys a batch to be sorted needs (k_ray_keys returns at once if it is not): the verdict's trip to the
            // host and the launches that follow it no longer leave the stream idle
            if (!a->knobs.repack_full_bounds) {
                eb = launch_ray_keys(d_rays, n, a->rp_bounds, a->rp_keys, a->rp_idx, s, a->knobs.repack_dirs3, true);
                if (eb != hipSuccess) return hip_fail(eb, "launch k_ray_keys");
                keys_made = true;
            }
            RTK_HIP(hipEventRecord(a->rp_done, s));                         // (both read the workspace's verdict words)
            RTK_HIP(hipEventSynchronize(a->rp_probe_ev));                   // the verdict, not the trace
            sort = a->rp_host[16] != 0u;
            if (!sort) return RTK_OK;                                        // coherent as it comes: that launch was the batch
            if (a->rp_host[17] <= 3u) {
                sorted_mode = RTK_TRACE_WAVE;                                // ten or fifteen bits per dimension: the sort makes tight waves
                // ... also when the lowest ones stay unsorted: one or two radix passes less (two dimensions: 8 of the 15 bits each)
                sort_from_bit = a->rp_host[17] <= 2u ? uint32_t(a->knobs.repack_skip_bits2) : uint32_t(a->knobs.repack_skip_bits);
            }
        }
        if (sort) {
            // The cells of the sort keys lie in the bounds of a SAMPLE of the batch (the probe's, where there was one; ~4,096 waves
            // otherwise): a ray outside them lands in a border cell -- an order a little worse for it, never another result -- and a
            // pass over all rays (0.13 ms of a 2^24-ray batch's 1.8) is saved.
            if (!probe) {
                const size_t waves = (n + 63) / 64;
                eb = launch_ray_bounds(d_rays, n, a->rp_bounds, a->knobs.repack_full_bounds ? 1u : uint32_t((waves + 4095) / 4096), false, s);
            } else if (a->knobs.repack_full_bounds) eb = launch_ray_bounds(d_rays, n, a->rp_bounds, 1u, false, s);
            if (eb == hipSuccess && !keys_made) eb = launch_ray_keys(d_rays, n, a->rp_bounds, a->rp_keys, a->rp_idx, s, a->knobs.repack_dirs3, false);
            if (eb == hipSuccess) eb = launch_key_sort(n, a->rp_keys, a->rp_idx, a->rp_temp, a->rp_temp_bytes, s, sort_from_bit);
            if (eb != hipSuccess) return hip_fail(eb, "ray repacking");
            A.perm = a->rp_idx + n;
            mode = a->knobs.repack_trace >= 0 ? a->knobs.repack_trace : sorted_mode;
        }
    }
    RTK_HIP_AS(launch_intersect(A, mode, stats, s), "launch k_intersect");
    if (A.perm != nullptr) {
        RTK_HIP(hipEventRecord(a->rp_done, s));
        a->rp_in_use = true;
    }
    return RTK_OK;
}

int rtk_accel_intersect_device(rtk_accel *a, const rtk_ray *d_rays, size_t n, int cull, int mode, rtk_hit *d_out, void *stream) {
    if (!a) return fail(RTK_ERR_INVALID, "null accel");
    std::lock_guard<std::mutex> lock(a->mu);
    RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
    return intersect_device_impl(a, d_rays, n, cull, mode, d_out, static_cast<hipStream_t>(stream), false);
}

int rtk_accel_intersect_stats(rtk_accel *a, const rtk_ray *d_rays, size_t n, int cull, int mode, rtk_hit *d_out,
                              rtk_counters *counters) {
    if (!a || !counters) return fail(RTK_ERR_INVALID, "null accel or counters");
    std::lock_guard<std::mutex> lock(a->mu);
    RTK_TRY(ensure_device(a));
    RTK_HIP(hipMemsetAsync(a->d_counters, 0, kCounterWords * sizeof(unsigned long long), nullptr));
    RTK_TRY(intersect_device_impl(a, d_rays, n, cull, mode, d_out, nullptr, true));
    unsigned long long h[8];
    RTK_HIP(hipMemcpy(h, a->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    counters->rays = h[0]; counters->primary = 0; counters->hits = h[2]; counters->nodes = h[3]; counters->boxpass = h[4];
    counters->leaves = h[5]; counters->tris = h[6]; counters->packets16 = h[7];
    return RTK_OK;
}

int rtk_accel_intersect(rtk_accel *a, const rtk_ray *rays, size_t n, int cull, int mode, rtk_hit *out) {
    if (!a) return fail(RTK_ERR_INVALID, "null accel");
    if (n > 0 && (!rays || !out)) return fail(RTK_ERR_INVALID, "null ray or hit buffer");
    std::lock_guard<std::mutex> lock(a->mu);
    RTK_TRY(ensure_device(a));
    if (n == 0) return RTK_OK;
    rtk_ray *d_rays = nullptr;
    rtk_hit *d_out = nullptr;
    RTK_HIP(hipMalloc(reinterpret_cast<void **>(&d_rays), n * sizeof(rtk_ray)));
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_out), n * sizeof(rtk_hit));
    if (e != hipSuccess) { (void)hipFree(d_rays); return hip_fail(e, "hipMalloc hits"); }
    e = hipMemcpy(d_rays, rays, n * sizeof(rtk_ray), hipMemcpyHostToDevice);
    int rc = RTK_OK;
    if (e == hipSuccess) {
        rc = intersect_device_impl(a, d_rays, n, cull, mode, d_out, nullptr, false);
        if (rc == RTK_OK) e = hipMemcpy(out, d_out, n * sizeof(rtk_hit), hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_rays); (void)hipFree(d_out);
    if (rc != RTK_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "intersect copy");
    return RTK_OK;
}

// ---------------------------------------------------------------- batched occlusion

// Word of the counter buffer the host variant counts its closest-hit queries in: the last of the four words behind the frame
// counters (the first-frame prior's six 32-bit cursors fill the first three), so the counters of the most recent frame
// (rtk_render_last_counters) stay as that frame left them.
static constexpr int kOccludedCountWord = kCounterWords + 3;

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
    A.materials = a->d_materials;
    A.rays = d_rays; A.max_t = d_max_t; A.out = d_out; A.n = n;
    A.shadow_bias = shadow_bias;
    A.has_refractive = a->has_refractive ? 1 : 0;
    A.n_intersect = count ? a->d_counters + kOccludedCountWord : nullptr;
    RTK_HIP_AS(launch_occluded(A, mode, s), "launch k_occluded");
    return RTK_OK;
}

int rtk_accel_occluded_device(rtk_accel *a, const rtk_ray *d_rays, const float *d_max_t, size_t n, float shadow_bias, int mode,
                              uint8_t *d_out, void *stream) {
    RTK_TRY(occluded_check(a, d_rays, d_max_t, n, shadow_bias, mode, d_out));
    if (n == 0) return RTK_OK;
    std::lock_guard<std::mutex> lock(a->mu);
    RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
    return occluded_launch(a, d_rays, d_max_t, n, shadow_bias, mode, d_out, static_cast<hipStream_t>(stream), false);
}

int rtk_accel_occluded(rtk_accel *a, const rtk_ray *rays, const float *max_t, size_t n, float shadow_bias, int mode, uint8_t *out,
                       uint64_t *n_intersections) {
    RTK_TRY(occluded_check(a, rays, max_t, n, shadow_bias, mode, out));
    if (n == 0) {
        if (n_intersections) *n_intersections = 0;
        return RTK_OK;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    RTK_TRY(ensure_device(a));
    if (a->oc_cap < n) {
        (void)hipFree(a->oc_rays); (void)hipFree(a->oc_max_t); (void)hipFree(a->oc_out);
        a->oc_rays = nullptr; a->oc_max_t = nullptr; a->oc_out = nullptr; a->oc_cap = 0;
        RTK_HIP(hipMalloc(reinterpret_cast<void **>(&a->oc_rays), n * sizeof(rtk_ray)));
        RTK_HIP(hipMalloc(reinterpret_cast<void **>(&a->oc_max_t), n * sizeof(float)));
        RTK_HIP(hipMalloc(reinterpret_cast<void **>(&a->oc_out), n));
        a->oc_cap = n;
    }
    RTK_HIP(hipMemcpy(a->oc_rays, rays, n * sizeof(rtk_ray), hipMemcpyHostToDevice));
    RTK_HIP(hipMemcpy(a->oc_max_t, max_t, n * sizeof(float), hipMemcpyHostToDevice));
    if (n_intersections) RTK_HIP(hipMemsetAsync(a->d_counters + kOccludedCountWord, 0, sizeof(unsigned long long), nullptr));
    RTK_TRY(occluded_launch(a, a->oc_rays, a->oc_max_t, n, shadow_bias, mode, a->oc_out, nullptr, n_intersections != nullptr));
    RTK_HIP(hipMemcpy(out, a->oc_out, n, hipMemcpyDeviceToHost));
    if (n_intersections) {
        unsigned long long h = 0;
        RTK_HIP(hipMemcpy(&h, a->d_counters + kOccludedCountWord, sizeof(h), hipMemcpyDeviceToHost));
        *n_intersections = h;
    }
    return RTK_OK;
}
