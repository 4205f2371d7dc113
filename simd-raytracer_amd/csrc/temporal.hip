// rtk_temporal_accumulate: the kernel.  A 256-thread workgroup per 16 x 16 pixel tile (denoise_plan.hpp denoise_tile), thread
// (t & 15, t >> 4) owns one pixel: it projects the pixel's world position into the previous view and walks the four taps of the
// history there in the order of rtk.h (temporal_math.hpp history, the one copy of the arithmetic).  Neighbouring pixels project to
// neighbouring places, so the taps of a tile fall into the same cache lines; where they fall depends on the data, so nothing is
// staged in LDS.  A tap loads depth, length and mesh first, then normal and position, and the 20 B of history only when it is
// accepted.  The new frame's rgb and noise are read only at the pixel that is written, so the outputs may be those planes.  A
// workgroup strides over the tiles, so the grid never exceeds kTpMaxGrid.
#include <hip/hip_runtime.h>

#include "temporal.hpp"
#include "temporal_math.hpp"

namespace rtk {
namespace dev {

__global__ __launch_bounds__(256) void k_temporal_accumulate(TemporalArgs A) {
    const uint32_t lx = threadIdx.x & (kDnTile - 1u), ly = threadIdx.x / kDnTile;
    const int32_t W = int32_t(A.tiling.width), H = int32_t(A.tiling.height);
    for (uint64_t tile = blockIdx.x; tile < A.tiling.n_tiles; tile += gridDim.x) {           // (uniform over the workgroup)
        const DnTile T = denoise_tile(A.tiling, tile);
        if (lx >= T.w || ly >= T.h) continue;
        const size_t at = size_t(T.y0 + ly) * A.tiling.width + (T.x0 + lx);
        tp::Pixel p = {};
        p.c[0] = A.rgb[3u * at]; p.c[1] = A.rgb[3u * at + 1u]; p.c[2] = A.rgb[3u * at + 2u];
        const float noise_p = A.noise ? A.noise[at] : 0.0f;
        p.var = A.noise ? noise_p * noise_p : 1.0f;
        p.depth = A.depth[at];
        bool blended = false;
        tp::Sums s;
        if (A.p_rgb && tp::is_hit(p.depth)) {
            for (uint32_t i = 0; i < 3u; ++i) { p.P[i] = A.position[3u * at + i]; p.n[i] = A.normal[3u * at + i]; }
            const uint32_t mesh_p = A.mesh ? A.mesh[at] : 0u;
            blended = tp::history(A.k, p, s, [&](const int qx, const int qy, tp::Tap &q) -> bool {
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
                const size_t aq = size_t(qy) * A.tiling.width + size_t(qx);
                q.length = A.p_length[aq];
                if (!tp::tap_alive(A.p_depth[aq], q.length)) return false;
                if (A.p_mesh && A.p_mesh[aq] != mesh_p) return false;
                const float nq[3] = {A.p_normal[3u * aq], A.p_normal[3u * aq + 1u], A.p_normal[3u * aq + 2u]};
                const float Pq[3] = {A.p_position[3u * aq], A.p_position[3u * aq + 1u], A.p_position[3u * aq + 2u]};
                if (!tp::tap_on_surface(A.k, p, nq, Pq)) return false;
                q.c[0] = A.p_rgb[3u * aq]; q.c[1] = A.p_rgb[3u * aq + 1u]; q.c[2] = A.p_rgb[3u * aq + 2u];
                float vq = 1.0f;
                if (A.p_noise) { const float nz = A.p_noise[aq]; vq = nz * nz; }
                q.var = vq;
                return true;
            });
        }
        if (blended) {
            const tp::Blend b = tp::blend(A.k, p, s);
            A.o_rgb[3u * at] = b.c[0]; A.o_rgb[3u * at + 1u] = b.c[1]; A.o_rgb[3u * at + 2u] = b.c[2];
            if (A.o_noise) A.o_noise[at] = b.noise;
            A.o_length[at] = b.length;
        } else {                                                       // the bits pass through
            A.o_rgb[3u * at] = p.c[0]; A.o_rgb[3u * at + 1u] = p.c[1]; A.o_rgb[3u * at + 2u] = p.c[2];
            if (A.o_noise) A.o_noise[at] = noise_p;
            A.o_length[at] = 1.0f;
        }
    }
}

}  // namespace dev

hipError_t launch_temporal_accumulate(const dev::TemporalArgs &A, hipStream_t s) {
    const DnTiling &t = A.tiling;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    if (t.width == 0u || t.height == 0u || t.width > uint32_t(kTpMaxSide) || t.height > uint32_t(kTpMaxSide)) return hipErrorInvalidValue;
    const DnTiling want = denoise_tiling(t.width, t.height, 1u);
    if (want.tiles_x != t.tiles_x || want.tiles_y != t.tiles_y || want.tiles_per_image != t.tiles_per_image || want.n_tiles != t.n_tiles)
        return hipErrorInvalidValue;
    if (!A.rgb || !A.position || !A.normal || !A.depth || !A.o_rgb || !A.o_length) return hipErrorInvalidValue;
    if ((A.noise != nullptr) != (A.o_noise != nullptr)) return hipErrorInvalidValue;
    if (A.p_rgb) {
        if (!A.p_length || !A.p_position || !A.p_normal || !A.p_depth) return hipErrorInvalidValue;
        if ((A.p_noise != nullptr) != (A.noise != nullptr) || (A.p_mesh != nullptr) != (A.mesh != nullptr)) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(dev::k_temporal_accumulate, dim3(temporal_grid(t.n_tiles)), dim3(kTpThreads), 0, s, A);
    return hipGetLastError();
}

}  // namespace rtk
