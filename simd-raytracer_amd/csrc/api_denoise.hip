// C-ABI, rtk_denoise_frame: an edge-avoiding a-trous filter of a frame along the surfaces its g-buffer describes.  The arithmetic of
// the calls -- refusals, tiles, halos, which steps go through LDS, the workspace -- is denoise_plan.hpp; the arithmetic of the filter
// is denoise_math.hpp; the kernels are denoise.hip.  The calls take no accel and touch none: they depend on no scene state.
#include <cstdlib>

#include "accel.hpp"
#include "denoise.hpp"

using namespace rtk;

namespace {

// refusals 1 and 2 of rtk.h; `third`: the call's third pointer that must not be null (in, or bytes)
int denoise_check(const rtk_denoise_params *p, int32_t n_images, const void *third) {
    if (!p || !third) return fail(RTK_ERR_INVALID, "null params, inputs or bytes");
    if (const char *why = denoise_refusal(*p, n_images)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

// RTK_DENOISE_LDS_MAX_STEP, read once per process
int lds_max_step() {
    static const int v = denoise_lds_max_step(std::getenv("RTK_DENOISE_LDS_MAX_STEP"));
    return v;
}

// The launches of a call, all on `s`: the prologue, then one kernel per iteration.  Device planes, a workspace that has passed the
// checks.  No allocation, no host block.
int denoise_device_impl(const rtk_denoise_params &p, int32_t n_images, const rtk_denoise_inputs &in, float *d_out, void *d_ws, hipStream_t s) {
    const uint64_t pixels = uint64_t(p.width) * uint64_t(p.height) * uint64_t(n_images);
    const DnWorkspace ws = denoise_workspace(pixels, p.iterations);
    char *const base = static_cast<char *>(d_ws);
    float4 *const g0 = reinterpret_cast<float4 *>(base + ws.g0), *const g1 = reinterpret_cast<float4 *>(base + ws.g1);
    float4 *const c[2] = {reinterpret_cast<float4 *>(base + ws.c[0]), reinterpret_cast<float4 *>(base + ws.c[1])};

    dev::DenoisePrepare P;
    P.rgb = in.rgb; P.noise = in.noise; P.albedo = in.albedo; P.normal = in.normal; P.position = in.position; P.depth = in.depth;
    P.g0 = g0; P.g1 = g1; P.c = c[0];
    P.pixels = pixels; P.albedo_floor = p.albedo_floor;
    RTK_HIP_AS(launch_denoise_prepare(P, s), "launch k_denoise_prepare");

    dev::DenoiseAtrous A;
    A.g0 = g0; A.g1 = g1; A.albedo = in.albedo;
    A.tiling = denoise_tiling(uint32_t(p.width), uint32_t(p.height), uint32_t(n_images));
    A.normal_power_log2 = p.normal_power_log2;
    A.sl2 = p.sigma_luminance * p.sigma_luminance; A.sp2 = p.sigma_plane * p.sigma_plane; A.albedo_floor = p.albedo_floor;
    for (int k = 0; k < p.iterations; ++k) {
        const bool last = k == p.iterations - 1;
        A.step = denoise_step(k);
        A.src = c[denoise_source(k)];
        A.dst = last ? nullptr : c[denoise_source(k) ^ 1];
        A.rgb_out = last ? d_out : nullptr;
        RTK_HIP_AS(launch_denoise_atrous(A, denoise_staged(A.step, lds_max_step()), s), "launch k_denoise_atrous");
    }
    return RTK_OK;
}

}  // namespace

extern "C" {

int rtk_denoise_workspace_bytes(const rtk_denoise_params *p, int32_t n_images, size_t *bytes) {
    return abi_guard([&]() -> int {
        RTK_TRY(denoise_check(p, n_images, bytes));
        *bytes = size_t(denoise_workspace(uint64_t(p->width) * uint64_t(p->height) * uint64_t(n_images), p->iterations).bytes);
        return RTK_OK;
    });
}

int rtk_denoise_frame_device(const rtk_denoise_params *p, int32_t n_images, const rtk_denoise_inputs *in, float *d_rgb_out, void *d_workspace,
                             size_t workspace_bytes, void *stream) {
    return abi_guard([&]() -> int {
        RTK_TRY(denoise_check(p, n_images, in));
        if (n_images == 0) return RTK_OK;
        if (const char *why = denoise_missing_plane(*in, d_rgb_out)) return fail(RTK_ERR_INVALID, why);
        const uint64_t need = denoise_workspace(uint64_t(p->width) * uint64_t(p->height) * uint64_t(n_images), p->iterations).bytes;
        if (const char *why = denoise_device_refusal(*in, d_rgb_out, d_workspace, workspace_bytes, need)) return fail(RTK_ERR_INVALID, why);
        RTK_TRY(need_device());
        return denoise_device_impl(*p, n_images, *in, d_rgb_out, d_workspace, static_cast<hipStream_t>(stream));
    });
}

int rtk_denoise_frame(const rtk_denoise_params *p, int32_t n_images, const rtk_denoise_inputs *in, float *rgb_out) {
    return abi_guard([&]() -> int {
        RTK_TRY(denoise_check(p, n_images, in));
        if (n_images == 0) return RTK_OK;
        if (const char *why = denoise_missing_plane(*in, rgb_out)) return fail(RTK_ERR_INVALID, why);
        RTK_TRY(need_device());
        // the planes and the output in one staging buffer, the workspace in a second one; both are the call's own and are freed
        // when it returns
        const uint64_t n = uint64_t(p->width) * uint64_t(p->height) * uint64_t(n_images);
        const float *const host[6] = {in->rgb, in->noise, in->albedo, in->normal, in->position, in->depth};
        const uint64_t each[6] = {3, 1, 3, 3, 3, 1};
        StageLayout L;
        for (int i = 0; i < 6; ++i) L.add(each[i] * n, host[i] != nullptr);
        const int o_rgb = L.add(3 * n);
        const DnWorkspace ws = denoise_workspace(n, p->iterations);
        HostStage stage;
        DevBuf<float4> work;
        RTK_MEM(stage.reserve(L));
        RTK_MEM(work.reserve(size_t(ws.bytes / sizeof(float4))));
        for (int i = 0; i < 6; ++i) RTK_HIP(stage.upload(i, host[i]));
        const rtk_denoise_inputs din = {stage.at<float>(0), stage.at<float>(1), stage.at<float>(2), stage.at<float>(3), stage.at<float>(4),
                                        stage.at<float>(5)};
        RTK_TRY(denoise_device_impl(*p, n_images, din, stage.at<float>(o_rgb), work.get(), nullptr));
        // (a copy on the null stream is behind the kernels and blocks the host)
        RTK_HIP(stage.download(o_rgb, rgb_out));
        return RTK_OK;
    });
}

}  // extern "C"
