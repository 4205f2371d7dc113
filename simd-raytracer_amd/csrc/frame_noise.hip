// rtk_render_frame_noise: the luminance statistic of a streamed frame, taken where the frame's samples already lie.
//
// In a RTK_TRACE_STREAM frame every sample of every pixel is a level-0 node of a batch's ray tree (stream.hip).  Once the batch's
// depth-0 k_combine has run, node b * n_root + i holds the colour of sample S.sample + b of pixel slot i, and node i says which
// pixel that is.  k_frame_moments runs behind that k_combine and in front of the event the next batch's k_combine waits for
// (launch_stream_sample), so the batches of a frame reach it in sample order, one at a time: a pixel's running sums need no atomics.
//
//   lane 0   k_path .. k_shadow .. k_combine(d-1 .. 1) | k_combine(0) k_frame_moments  done0 |
//   lane 1   k_path .. k_shadow .. k_combine(d-1 .. 1) ........ wait done0 | k_combine(0) k_frame_moments  done1 |
//   lane 2   ...                                                          ........ wait done1 | ...
//
// One thread per pixel slot, grid-strided like the depth-0 k_combine.  Per slot: 16 B of node i for the pixel, 16 B per sample of
// the batch for the colour, and 16 B of running sums loaded (not by the first batch) and stored (not by the last, which writes
// the 4 B of noise instead).  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "frame_noise_math.hpp"
#include "frame_noise_plan.hpp"
#include "stream.hpp"

namespace rtk {
namespace dev {

struct FrameMomentsArgs {
    const NodeRes *nodes;                          // the lane's: level 0 is nodes [0, n_root * n_batch)
    const uint32_t *overflow;                      // the lane's own overflow word
    const uint32_t *lane_overflow[kStreamLanes];   // and those of all lanes of the frame, as k_combine at depth 0 has them
    uint32_t n_lanes;
    uint32_t n_root, n_batch;
    uint32_t n_pixels;                             // width * height
    int spp;
    uint32_t starts, ends;                         // frame_noise_plan.hpp FrameNoiseBatch
    double *s1, *s2;
    float *noise;
};

__global__ __launch_bounds__(256) void k_frame_moments(FrameMomentsArgs M) {
    // k_combine's early returns at level 0: what it did not emit has no statistic either (the call is redone)
    if (*M.overflow != 0u) return;
    for (uint32_t j = 0; j < M.n_lanes; ++j) if (*M.lane_overflow[j] != 0u) return;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M.n_root; i += stride) {
        const float4 tail = reinterpret_cast<const float4 *>(M.nodes + i)[1];
        const uint32_t pix = __float_as_uint(tail.w);
        if (pix == 0xFFFFFFFFu) continue;                                      // not a pixel of the frame (block overhanging its edge)
        if (pix >= M.n_pixels) continue;                                       // never trust an index read from memory
        double s1 = 0.0, s2 = 0.0;
        if (!M.starts) { s1 = M.s1[pix]; s2 = M.s2[pix]; }
        for (uint32_t b = 0; b < M.n_batch; ++b) {
            const float4 c = reinterpret_cast<const float4 *>(M.nodes + (size_t)b * M.n_root + i)[0];
            // the sample colour as radiance returns it: +0 + c
            fn_add(s1, s2, fn_lum(0.0f + c.x, 0.0f + c.y, 0.0f + c.z));
        }
        if (M.ends) M.noise[pix] = (float)fn_error(s1, s2, M.spp);
        else { M.s1[pix] = s1; M.s2[pix] = s2; }
    }
}

}  // namespace dev

hipError_t launch_frame_moments(const dev::StreamArgs &S, const StreamMoments &M, hipStream_t s) {
    if (S.n_root == 0u || S.n_batch == 0u) return hipSuccess;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    if (!M.s1 || !M.s2 || !M.noise || !S.ws.nodes || !S.ws.ctrl) return hipErrorInvalidValue;
    if (M.n_pixels == 0u || (uint64_t)M.n_pixels > kFrameNoiseMaxPixels || (uint64_t)M.n_pixels != (uint64_t)S.r.width * S.r.height) return hipErrorInvalidValue;
    if ((uint64_t)S.n_root * S.n_batch > (uint64_t)S.ws.node_cap || S.n_lanes > (uint32_t)dev::kStreamLanes) return hipErrorInvalidValue;
    if (S.r.spp < 2 || S.sample < 0 || (int64_t)S.sample + (int64_t)S.n_batch > (int64_t)S.r.spp) return hipErrorInvalidValue;
    for (uint32_t j = 0; j < S.n_lanes; ++j) if (!S.lane_overflow[j]) return hipErrorInvalidValue;
    const FrameNoiseBatch fb =frame_noise_batch(S.sample, S.n_batch, S.r.spp);
    dev::FrameMomentsArgs A;
    A.nodes = S.ws.nodes; A.overflow = S.ws.ctrl + dev::kCtrlOverflow;
    for (int j = 0; j < dev::kStreamLanes; ++j) A.lane_overflow[j] = S.lane_overflow[j];
    A.n_lanes = S.n_lanes; A.n_root = S.n_root; A.n_batch = S.n_batch; A.n_pixels = M.n_pixels; A.spp = S.r.spp;
    A.starts = fb.starts ? 1u : 0u; A.ends = fb.ends ? 1u : 0u;
    A.s1 = M.s1; A.s2 = M.s2; A.noise = M.noise;
    const unsigned blocks = (S.n_root + 255u) / 256u;
    hipLaunchKernelGGL(dev::k_frame_moments, dim3(blocks < 2048u ? blocks : 2048u), dim3(256), 0, s, A);
    return hipGetLastError();
}

}  // namespace rtk
