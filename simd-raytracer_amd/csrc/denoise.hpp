// rtk_denoise_frame: the argument blocks and launchers of the two kernels of denoise.hip, shared with api_denoise.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "denoise_plan.hpp"

namespace rtk {
namespace dev {

struct DenoisePrepare {
    const float *rgb, *noise, *albedo, *normal, *position, *depth;     // the caller's planes; noise and albedo may be null
    float4 *g0, *g1, *c;                                               // the records of the workspace (denoise_plan.hpp DnWorkspace)
    uint64_t pixels;                                                   // of all images
    float albedo_floor;
};

struct DenoiseAtrous {
    const float4 *g0, *g1, *src;      // (n.xyz, hit), (P.xyz, 0) and the previous iteration's (r, g, b, var)
    float4 *dst;                      // this iteration's (r, g, b, var); null in the last iteration
    float *rgb_out;                   // the last iteration's output [..][3]; null in every other
    const float *albedo;              // the caller's plane for the epilogue or null; read by the last iteration only
    DnTiling tiling;
    uint32_t step;
    int32_t normal_power_log2;
    float sl2, sp2, albedo_floor;
};

}  // namespace dev

hipError_t launch_denoise_prepare(const dev::DenoisePrepare &A, hipStream_t s);
// staged: the halo'd tile goes through LDS (the step must be <= kDnLdsStepLimit); the last iteration is the one with rgb_out set
hipError_t launch_denoise_atrous(const dev::DenoiseAtrous &A, bool staged, hipStream_t s);

}  // namespace rtk
