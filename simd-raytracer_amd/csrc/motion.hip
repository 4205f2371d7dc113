// rtk_render_motion: the kernel.  A 256-thread workgroup per 16 x 16 pixel tile (denoise_plan.hpp denoise_tile), thread
// (t & 15, t >> 4) owns one pixel.  Three dependent stages per pixel: the triangle id; then the barycentrics and the triangle's
// three vertex ids; then the nine floats of the previous pose.  The id is tested against the triangle count before anything is
// loaded with it, and a vertex id against the vertex count likewise, so no plane can make the kernel read outside its tables.
// Neighbouring pixels mostly share a triangle, so the gathers of a tile fall into few cache lines; nothing is staged in LDS.
// Only the planes asked for are written: the kernel is instantiated on the two outputs.  A workgroup strides over the tiles, so
// the grid never exceeds kMvMaxGrid.
// RTK_MOTION_UNIFORM=1 builds the variant in which a wave whose active lanes all carry one id reads the three vertex ids once,
// through the scalar cache, and its lanes load the vertices from one address.  Measured, it is no faster,
// so the default is the plain per-lane path.
#include <hip/hip_runtime.h>

#include "motion.hpp"
#include "motion_math.hpp"

#ifndef RTK_MOTION_UNIFORM
#define RTK_MOTION_UNIFORM 0
#endif

namespace rtk {
namespace dev {

template <bool kPosition, bool kMotion>
__global__ __launch_bounds__(256) void k_motion(MotionArgs A) {
    const uint32_t lx = threadIdx.x & (kDnTile - 1u), ly = threadIdx.x / kDnTile;
    const uint32_t *__restrict__ const index = A.index;
    const float *__restrict__ const verts = A.verts;
    for (uint64_t tile = blockIdx.x; tile < A.tiling.n_tiles; tile += gridDim.x) {           // (uniform over the workgroup)
        const DnTile T = denoise_tile(A.tiling, tile);
        if (lx >= T.w || ly >= T.h) continue;
        const uint32_t x = T.x0 + lx, y = T.y0 + ly;
        const size_t at = size_t(y) * A.tiling.width + x;
        const uint32_t id = A.tri[at];
        float P[3] = {0.0f, 0.0f, 0.0f};
        bool hit = mv::is_hit(id, A.n_tris);
        if (hit) {
            const float u = A.bary[2u * at], v = A.bary[2u * at + 1u];
            float a[3], b[3], c[3];
#if RTK_MOTION_UNIFORM
            const uint32_t id0 = __builtin_amdgcn_readfirstlane(id);
            if (__all(id == id0)) {                                                            // (of the lanes that got here)
                const uint32_t i0 = index[3u * size_t(id0)], i1 = index[3u * size_t(id0) + 1u], i2 = index[3u * size_t(id0) + 2u];
                hit = i0 < A.n_verts && i1 < A.n_verts && i2 < A.n_verts;
                if (hit)
                    for (uint32_t i = 0; i < 3u; ++i) { a[i] = verts[3u * size_t(i0) + i]; b[i] = verts[3u * size_t(i1) + i]; c[i] = verts[3u * size_t(i2) + i]; }
            } else
#endif
            {
                const uint32_t i0 = index[3u * size_t(id)], i1 = index[3u * size_t(id) + 1u], i2 = index[3u * size_t(id) + 2u];
                // (the accel's tables hold vertex ids only; a table that did not could still not make the kernel read outside)
                hit = i0 < A.n_verts && i1 < A.n_verts && i2 < A.n_verts;
                if (hit)
                    for (uint32_t i = 0; i < 3u; ++i) { a[i] = verts[3u * size_t(i0) + i]; b[i] = verts[3u * size_t(i1) + i]; c[i] = verts[3u * size_t(i2) + i]; }
            }
            if (hit) mv::surface_point(a, b, c, u, v, P);
        }
        if (kPosition) { A.prev_position[3u * at] = P[0]; A.prev_position[3u * at + 1u] = P[1]; A.prev_position[3u * at + 2u] = P[2]; }
        if (kMotion) {
            float mx = __uint_as_float(mv::kMissBits), my = __uint_as_float(mv::kMissBits);
            if (hit) (void)mv::motion_of(A.k, P, x, y, mx, my);
            A.motion[2u * at] = mx; A.motion[2u * at + 1u] = my;
        }
    }
}

}  // namespace dev

hipError_t launch_motion(const dev::MotionArgs &A, hipStream_t s) {
    const DnTiling &t = A.tiling;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    if (t.width == 0u || t.height == 0u || t.width > uint32_t(kMvMaxSide) || t.height > uint32_t(kMvMaxSide)) return hipErrorInvalidValue;
    const DnTiling want = denoise_tiling(t.width, t.height, 1u);
    if (want.tiles_x != t.tiles_x || want.tiles_y != t.tiles_y || want.tiles_per_image != t.tiles_per_image || want.n_tiles != t.n_tiles)
        return hipErrorInvalidValue;
    if (!A.tri || !A.bary || !A.verts || (!A.prev_position && !A.motion)) return hipErrorInvalidValue;
    if (A.n_tris > 0u && !A.index) return hipErrorInvalidValue;
    const dim3 grid(motion_grid(t.n_tiles)), block(kMvThreads);
    if (A.prev_position && A.motion) hipLaunchKernelGGL((dev::k_motion<true, true>), grid, block, 0, s, A);
    else if (A.prev_position) hipLaunchKernelGGL((dev::k_motion<true, false>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((dev::k_motion<false, true>), grid, block, 0, s, A);
    return hipGetLastError();
}

}  // namespace rtk
