// Measurement-only door to the launchers of csrc/denoise.hip (tools/bench_denoise.py): one kernel launch per call, so that a tool can
// bracket each with device events and choose the path -- staged in LDS or direct -- per launch instead of per process.  Compiled
// together with denoise.hip itself with the library's own FLAGS (make denoise_probe); not part of the product.
#include <hip/hip_runtime.h>

#include "denoise.hpp"

using namespace rtk;

namespace {
struct Views { float4 *g0, *g1, *c[2]; };
Views views(void *d_ws, uint64_t pixels, int iterations) {
    const DnWorkspace ws = denoise_workspace(pixels, iterations);
    char *const base = static_cast<char *>(d_ws);
    return Views{reinterpret_cast<float4 *>(base + ws.g0), reinterpret_cast<float4 *>(base + ws.g1),
                 {reinterpret_cast<float4 *>(base + ws.c[0]), reinterpret_cast<float4 *>(base + ws.c[1])}};
}
}  // namespace

extern "C" {

// the prologue of a call of `iterations` iterations into the workspace; -> hipError_t
int dn_probe_prepare(const rtk_denoise_params *p, int32_t n_images, const rtk_denoise_inputs *in, void *d_ws, void *stream) {
    if (!p || !in || !d_ws || denoise_refusal(*p, n_images) || denoise_missing_plane(*in, d_ws)) return int(hipErrorInvalidValue);
    const uint64_t pixels = uint64_t(p->width) * uint64_t(p->height) * uint64_t(n_images);
    const Views v = views(d_ws, pixels, p->iterations);
    dev::DenoisePrepare P;
    P.rgb = in->rgb; P.noise = in->noise; P.albedo = in->albedo; P.normal = in->normal; P.position = in->position; P.depth = in->depth;
    P.g0 = v.g0; P.g1 = v.g1; P.c = v.c[0];
    P.pixels = pixels; P.albedo_floor = p->albedo_floor;
    return int(launch_denoise_prepare(P, static_cast<hipStream_t>(stream)));
}

// iteration k of such a call, staged or direct, exactly as rtk_denoise_frame_device launches it; -> hipError_t
int dn_probe_atrous(const rtk_denoise_params *p, int32_t n_images, const float *d_albedo, float *d_rgb_out, void *d_ws, int k, int staged,
                    void *stream) {
    if (!p || !d_ws || !d_rgb_out || denoise_refusal(*p, n_images) || k < 0 || k >= p->iterations) return int(hipErrorInvalidValue);
    const uint64_t pixels = uint64_t(p->width) * uint64_t(p->height) * uint64_t(n_images);
    const Views v = views(d_ws, pixels, p->iterations);
    const bool last = k == p->iterations - 1;
    dev::DenoiseAtrous A;
    A.g0 = v.g0; A.g1 = v.g1; A.albedo = d_albedo;
    A.tiling = denoise_tiling(uint32_t(p->width), uint32_t(p->height), uint32_t(n_images));
    A.normal_power_log2 = p->normal_power_log2;
    A.sl2 = p->sigma_luminance * p->sigma_luminance; A.sp2 = p->sigma_plane * p->sigma_plane; A.albedo_floor = p->albedo_floor;
    A.step = denoise_step(k);
    A.src = v.c[denoise_source(k)];
    A.dst = last ? nullptr : v.c[denoise_source(k) ^ 1];
    A.rgb_out = last ? d_rgb_out : nullptr;
    return int(launch_denoise_atrous(A, staged != 0, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
