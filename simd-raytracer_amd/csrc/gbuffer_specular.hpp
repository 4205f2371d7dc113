// rtk_render_gbuffer_specular: the argument block and the launcher of k_gbuffer_specular (gbuffer_specular.hip), shared with
// api_gbuffer_specular.hip.
#pragma once

#include "kernels.hpp"
#include "gbuffer_specular_plan.hpp"

namespace rtk {
namespace dev {

struct GbufferSpecularArgs {
    // Of `r` the kernel reads what k_gbuffer reads (gbuffer.hpp GbufferArgs) and, for the chain, max_depth, reflection_bias and
    // refraction_bias.
    RenderArgs r;
    int sample;
    uint32_t mask;                    // kGs* bits: the planes to write (wave-uniform)
    // the planes of this launch's first view, [n_views][height][width] each; only 4-byte alignment is promised
    float *depth, *position, *normal, *surface_position, *surface_normal, *albedo, *bary;
    uint32_t *tri, *mesh, *material, *bounces;
    float *last_ray;
};

}  // namespace dev

// grid_x * grid_y workgroups of four waves cover the launch's units (gbuffer_plan.hpp GbufferLaunch)
hipError_t launch_gbuffer_specular(const dev::GbufferSpecularArgs &G, uint32_t grid_x, uint32_t grid_y, hipStream_t s);

}  // namespace rtk
