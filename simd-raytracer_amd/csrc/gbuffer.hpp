// rtk_render_gbuffer: the argument block and the launcher of k_gbuffer (gbuffer.hip), shared with api_gbuffer.hip.
#pragma once

#include "kernels.hpp"
#include "gbuffer_plan.hpp"

namespace rtk {
namespace dev {

struct GbufferArgs {
    // Of `r` the kernel reads: tree, materials, textures, tri_uv, tex_pixels, background; the camera half (camera_args: cam_pos,
    // cam_mat, width, height, aspect, tan_half_fov, spp, seed, width_f, height_f); and the units of THIS launch: views (null = the
    // camera in the arguments), n_views, units_per_view, n_units = n_views * units_per_view.
    RenderArgs r;
    int sample;
    uint32_t mask;                    // kGb* bits: the planes to write (wave-uniform)
    // the planes of this launch's first view, [n_views][height][width] each; only 4-byte alignment is promised
    float *depth, *position, *normal, *albedo, *bary;
    uint32_t *tri, *mesh, *material;
};

}  // namespace dev

// grid_x * grid_y workgroups of four waves cover the launch's units (gbuffer_plan.hpp GbufferLaunch)
hipError_t launch_gbuffer(const dev::GbufferArgs &G, uint32_t grid_x, uint32_t grid_y, hipStream_t s);

}  // namespace rtk
