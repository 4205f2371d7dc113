// rtk_render_adaptive: the argument block of k_adaptive_decide and the launchers of the three kernels of adaptive.hip, shared
// with api_adaptive.hip.
#pragma once

#include "kernels.hpp"
#include "adaptive_plan.hpp"

namespace rtk {
namespace dev {

struct AdaptiveDecide {
    // the round's active blocks (numbers in the frame's own 8x8 grid, row-major); null = the call's first launch: unit u IS block
    // u, nothing is judged, and every block goes on at adaptive_first_offset (no atomics, a list in frame order)
    const uint32_t *blocks;
    uint32_t n_blocks;
    uint32_t width, height;
    int32_t n;                        // the checkpoint: samples every pixel of the round's blocks has by now
    int32_t last;                     // n is the ceiling: every block is finished
    double threshold, floor;          // (double)rtk_adaptive_params::threshold / ::floor
    float *rgb;                       // [h][w][3] running sums; a finished block's pixels become sum / float(n)
    const double *s1, *s2;            // [h][w] sums of the luminance and of its square
    uint32_t *samples;                // [h][w] or null
    float *noise;                     // [h][w] or null
    uint32_t *next_blocks, *next_list;    // the next round's blocks and pixels (frame pixel indices)
    unsigned long long *count;        // ad_count_word of the next round; zero when the launch begins (unused by the first launch)
};

}  // namespace dev

// camera rays of pixels list[0, n) at `sample`; A: the camera half of the frame's arguments (camera_args), spp = the ceiling
hipError_t launch_adaptive_rays(const dev::RenderArgs &A, int sample, const uint32_t *list, uint32_t n, rtk_ray *d_rays, hipStream_t s);
// rgb[list[t]] += colours[t], S1 += y, S2 += y * y; `start`: sample 0, the sums begin at +0
hipError_t launch_adaptive_accumulate(const uint32_t *list, uint32_t n, const float *colours, float *rgb, double *s1, double *s2,
                                      uint64_t frame_pixels, bool start, hipStream_t s);
hipError_t launch_adaptive_decide(const dev::AdaptiveDecide &D, hipStream_t s);

}  // namespace rtk
