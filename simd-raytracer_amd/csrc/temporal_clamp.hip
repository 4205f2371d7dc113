// rtk_temporal_accumulate_clamped: the kernel.  As k_temporal_accumulate (temporal.hip), a 256-thread workgroup per 16 x 16 pixel
// tile, thread (t & 15, t >> 4) owns one pixel and walks the four taps of the history in global memory through tp::history.  What
// is new is the box of the NEW frame around the pixel (temporal_clamp_math.hpp): its taps are where the tile is, so all 256
// threads first stage the tile with a halo of R pixels in LDS -- (16 + 2R)^2 pixels, five planes of one word each (r, g, b, var,
// mesh), so that neighbouring lanes read neighbouring banks.  A staged pixel that is outside the image or no hit has var = -1
// (var = noise * noise is never negative, and a NaN is not below zero) and nothing else loaded: the box skips it.
//
// Barriers: every thread of a workgroup reaches both barriers of every tile.  The trip count of the tile loop depends on blockIdx
// and gridDim alone, the staging loop has no early exit, and a thread outside a partial tile skips only the per-pixel part
// between the barriers.
#include <hip/hip_runtime.h>

#include "temporal_clamp.hpp"
#include "temporal_clamp_math.hpp"

namespace rtk {
namespace dev {

template <int R>
__global__ __launch_bounds__(256) void k_temporal_accumulate_clamped(TemporalClampArgs B) {
    constexpr uint32_t S = temporal_clamp_side(R), NP = temporal_clamp_lds_pixels(R);
    __shared__ float s_c[3][NP];
    __shared__ float s_var[NP];
    __shared__ uint32_t s_mesh[NP];
    static_assert(sizeof(s_c) + sizeof(s_var) + sizeof(s_mesh) == temporal_clamp_lds_bytes(R), "the plan's footprint");
    const TemporalArgs &A = B.t;
    const uint32_t lx = threadIdx.x & (kDnTile - 1u), ly = threadIdx.x / kDnTile;
    const int32_t W = int32_t(A.tiling.width), H = int32_t(A.tiling.height);
    for (uint64_t tile = blockIdx.x; tile < A.tiling.n_tiles; tile += gridDim.x) {           // (uniform over the workgroup)
        const DnTile T = denoise_tile(A.tiling, tile);
        // ---- stage the tile and its halo: all threads, no early exit
        for (uint32_t i = threadIdx.x; i < NP; i += kTpThreads) {
            const uint32_t sy = i / S, sx = i - sy * S;
            const int32_t gx = int32_t(T.x0 + sx) - R, gy = int32_t(T.y0 + sy) - R;
            float var = -1.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t aq = size_t(gy) * A.tiling.width + size_t(gx);
                if (tp::is_hit(A.depth[aq])) {
                    s_c[0][i] = A.rgb[3u * aq]; s_c[1][i] = A.rgb[3u * aq + 1u]; s_c[2][i] = A.rgb[3u * aq + 2u];
                    var = 1.0f;
                    if (A.noise) { const float nz = A.noise[aq]; var = nz * nz; }
                    s_mesh[i] = A.mesh ? A.mesh[aq] : 0u;
                }
            }
            s_var[i] = var;
        }
        __syncthreads();
        // ---- the per-pixel part: the only part a thread outside a partial tile skips
        if (lx < T.w && ly < T.h) {
            const size_t at = size_t(T.y0 + ly) * A.tiling.width + (T.x0 + lx);
            tp::Pixel p = {};
            p.c[0] = A.rgb[3u * at]; p.c[1] = A.rgb[3u * at + 1u]; p.c[2] = A.rgb[3u * at + 2u];
            const float noise_p = A.noise ? A.noise[at] : 0.0f;
            p.var = A.noise ? noise_p * noise_p : 1.0f;
            p.depth = A.depth[at];
            bool blended = false;
            tp::Sums s;
            uint32_t mesh_p = 0u;
            if (A.p_rgb && tp::is_hit(p.depth)) {
                for (uint32_t i = 0; i < 3u; ++i) { p.P[i] = A.position[3u * at + i]; p.n[i] = A.normal[3u * at + i]; }
                mesh_p = A.mesh ? A.mesh[at] : 0u;
                // (the history walk of k_temporal_accumulate, which stays as it is)
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
                // the box, from LDS: the staged index of p is (ly + R, lx + R), so every tap lies inside the staged square
                tp::Box b = tp::box_empty();
                const uint32_t centre = (ly + uint32_t(R)) * S + (lx + uint32_t(R));
                _Pragma("nounroll")
                for (int dy = -R; dy <= R; ++dy) {
                    RTK_TP_UNROLL
                    for (int dx = -R; dx <= R; ++dx) {
                        const uint32_t q = uint32_t(int32_t(centre) + dy * int32_t(S) + dx);
                        const float var = s_var[q];
                        if (var < 0.0f) continue;
                        if (A.mesh && s_mesh[q] != mesh_p) continue;
                        const float c[3] = {s_c[0][q], s_c[1][q], s_c[2][q]};
                        tp::box_add(b, c, var);
                    }
                }
                const tp::Blend o = tp::blend_clamped(A.k, B.gamma, B.history_keep, p, s, b);
                A.o_rgb[3u * at] = o.c[0]; A.o_rgb[3u * at + 1u] = o.c[1]; A.o_rgb[3u * at + 2u] = o.c[2];
                if (A.o_noise) A.o_noise[at] = o.noise;
                A.o_length[at] = o.length;
            } else {                                                       // the bits pass through
                A.o_rgb[3u * at] = p.c[0]; A.o_rgb[3u * at + 1u] = p.c[1]; A.o_rgb[3u * at + 2u] = p.c[2];
                if (A.o_noise) A.o_noise[at] = noise_p;
                A.o_length[at] = 1.0f;
            }
        }
        __syncthreads();                                                   // the next tile is staged over this one
    }
}

}  // namespace dev

hipError_t launch_temporal_accumulate_clamped(const dev::TemporalClampArgs &B, hipStream_t s) {
    const dev::TemporalArgs &A = B.t;
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
    if (A.o_rgb == A.rgb || (A.o_noise && A.o_noise == A.noise)) return hipErrorInvalidValue;
    const dim3 grid(temporal_grid(t.n_tiles)), block(kTpThreads);
    switch (B.radius) {
        case 1: hipLaunchKernelGGL(dev::k_temporal_accumulate_clamped<1>, grid, block, 0, s, B); break;
        case 2: hipLaunchKernelGGL(dev::k_temporal_accumulate_clamped<2>, grid, block, 0, s, B); break;
        case 3: hipLaunchKernelGGL(dev::k_temporal_accumulate_clamped<3>, grid, block, 0, s, B); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rtk
