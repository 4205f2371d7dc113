// rtk_denoise_frame: the two kernels.  k_denoise_prepare runs the prologue of rtk.h once per pixel and packs what a tap reads into
// three 16-byte records -- (r, g, b, var), (n.xyz, hit) and (P.xyz, 0) -- so that a tap is three dwordx4 loads instead of eleven
// scalar ones out of five planes.  k_denoise_atrous runs one iteration: a 256-thread workgroup per 16 x 16 pixel tile of an image
// (denoise_plan.hpp denoise_tile), thread (t & 15, t >> 4) owns one pixel and walks its 25 taps in the order of rtk.h
// (denoise_math.hpp filter_pixel, the one copy of the arithmetic).
//   staged: the workgroup first copies the tile with its halo of 2 * step pixels into LDS, records of pixels outside the image
//     as misses, and the taps read LDS.  At step 1 the 256 pixels of a tile read 400 distinct pixels 25 times over; at step 8 it is
//     2304 pixels and 108 KiB, one workgroup per CU.
//   direct: the taps read the records from global memory with a bounds test each.
// Which steps take which path is the plan's decision (denoise_staged); both give the same bits.  The last iteration applies the
// epilogue and writes the caller's rgb_out.  A workgroup strides over the tiles, so the grid never exceeds kDnMaxGrid.
#include <hip/hip_runtime.h>

#include "denoise.hpp"
#include "denoise_math.hpp"

namespace rtk {
namespace dev {

__global__ __launch_bounds__(256) void k_denoise_prepare(DenoisePrepare A) {
    const uint64_t stride = (uint64_t)gridDim.x * kDnThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kDnThreads + threadIdx.x; i < A.pixels; i += stride) {
        const bool hit = dn::is_hit(A.depth[i]);
        const dn::Rgbv c = dn::prologue(A.rgb + 3u * i, A.albedo ? A.albedo + 3u * i : nullptr, A.noise ? A.noise + i : nullptr, hit, A.albedo_floor);
        const float *n = A.normal + 3u * i, *P = A.position + 3u * i;
        A.c[i] = make_float4(c.r, c.g, c.b, c.var);
        A.g0[i] = make_float4(n[0], n[1], n[2], hit ? 1.0f : 0.0f);
        A.g1[i] = make_float4(P[0], P[1], P[2], 0.0f);
    }
}

extern __shared__ float4 dn_lds[];       // STAGED: [3][side][pitch] records: g0, g1, signal

__device__ __forceinline__ dn::Tap make_tap(const float4 c, const float4 g0, const float4 g1) {
    dn::Tap t;
    t.c.r = c.x; t.c.g = c.y; t.c.b = c.z; t.c.var = c.w;
    t.g.nx = g0.x; t.g.ny = g0.y; t.g.nz = g0.z;
    t.g.px = g1.x; t.g.py = g1.y; t.g.pz = g1.z;
    return t;
}

template <bool STAGED, bool LAST>
__global__ __launch_bounds__(256) void k_denoise_atrous(DenoiseAtrous A) {
    const int32_t lx = int32_t(threadIdx.x & (kDnTile - 1u)), ly = int32_t(threadIdx.x / kDnTile);
    const int32_t W = int32_t(A.tiling.width), H = int32_t(A.tiling.height), s = int32_t(A.step);
    const uint64_t image_pixels = (uint64_t)A.tiling.width * A.tiling.height;
    const int32_t halo = int32_t(denoise_halo(A.step));
    const uint32_t side = denoise_lds_side(A.step), pitch = denoise_lds_pitch(A.step), plane = pitch * side;
    for (uint64_t tile = blockIdx.x; tile < A.tiling.n_tiles; tile += gridDim.x) {        // (uniform over the workgroup)
        const DnTile T = denoise_tile(A.tiling, tile);
        const uint64_t base = (uint64_t)T.image * image_pixels;
        if (STAGED) {
            __syncthreads();                                           // the previous tile's taps are done with the LDS
            for (uint32_t i = threadIdx.x; i < side * side; i += kDnThreads) {
                const uint32_t ty = i / side, tx = i - ty * side;
                const int32_t gx = int32_t(T.x0 + tx) - halo, gy = int32_t(T.y0 + ty) - halo;
                float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, c = g0;             // outside the image: a miss
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                    const uint64_t q = base + (uint64_t)gy * A.tiling.width + (uint32_t)gx;
                    g0 = A.g0[q]; g1 = A.g1[q]; c = A.src[q];
                }
                const uint32_t at = ty * pitch + tx;
                dn_lds[at] = g0; dn_lds[plane + at] = g1; dn_lds[2u * plane + at] = c;
            }
            __syncthreads();
        }
        if (lx >= int32_t(T.w) || ly >= int32_t(T.h)) continue;        // (no barrier behind this in the iteration)
        const int32_t x = int32_t(T.x0) + lx, y = int32_t(T.y0) + ly;
        const uint64_t at_p = base + (uint64_t)y * A.tiling.width + (uint32_t)x;
        const uint32_t lds_p = uint32_t(ly + halo) * pitch + uint32_t(lx + halo);
        const float4 pg0 = STAGED ? dn_lds[lds_p] : A.g0[at_p];
        const float4 pg1 = STAGED ? dn_lds[plane + lds_p] : A.g1[at_p];
        const float4 pc = STAGED ? dn_lds[2u * plane + lds_p] : A.src[at_p];
        const bool hit = pg0.w != 0.0f;
        const dn::Tap p = make_tap(pc, pg0, pg1);
        dn::Rgbv c = p.c;
        if (hit) {
            c = dn::filter_pixel(p, A.sl2, A.sp2, A.normal_power_log2, [&](const int dx, const int dy, dn::Tap &q) -> bool {
                float4 g0, g1, qc;
                if (STAGED) {
                    const uint32_t at = uint32_t(ly + halo + dy * s) * pitch + uint32_t(lx + halo + dx * s);
                    g0 = dn_lds[at];
                    if (g0.w == 0.0f) return false;
                    g1 = dn_lds[plane + at]; qc = dn_lds[2u * plane + at];
                } else {
                    const int32_t qx = x + dx * s, qy = y + dy * s;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
                    const uint64_t at = base + (uint64_t)qy * A.tiling.width + (uint32_t)qx;
                    g0 = A.g0[at];
                    if (g0.w == 0.0f) return false;
                    g1 = A.g1[at]; qc = A.src[at];
                }
                q = make_tap(qc, g0, g1);
                return true;
            });
        }
        if (LAST) {
            float out[3];
            dn::epilogue(c, A.albedo ? A.albedo + 3u * at_p : nullptr, hit, A.albedo_floor, out);
            float *o = A.rgb_out + 3u * at_p;
            o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
        } else {
            A.dst[at_p] = make_float4(c.r, c.g, c.b, c.var);
        }
    }
}

}  // namespace dev

hipError_t launch_denoise_prepare(const dev::DenoisePrepare &A, hipStream_t s) {
    if (A.pixels == 0u) return hipSuccess;
    if (!A.rgb || !A.normal || !A.position || !A.depth || !A.g0 || !A.g1 || !A.c || A.pixels > kDnMaxPixels) return hipErrorInvalidValue;
    const uint64_t groups = (A.pixels + kDnThreads - 1u) / kDnThreads;
    hipLaunchKernelGGL(dev::k_denoise_prepare, dim3(denoise_grid(groups)), dim3(kDnThreads), 0, s, A);
    return hipGetLastError();
}

namespace {
template <bool STAGED, bool LAST>
hipError_t launch_atrous(const dev::DenoiseAtrous &A, hipStream_t s) {
    const uint32_t lds = STAGED ? denoise_lds_bytes(A.step) : 0u;
    if (lds > 32u * 1024u) {         // beyond what a kernel may ask for by default
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&dev::k_denoise_atrous<STAGED, LAST>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((dev::k_denoise_atrous<STAGED, LAST>), dim3(denoise_grid(A.tiling.n_tiles)), dim3(kDnThreads), lds, s, A);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_denoise_atrous(const dev::DenoiseAtrous &A, bool staged, hipStream_t s) {
    const DnTiling &t = A.tiling;
    if (t.n_tiles == 0u) return hipSuccess;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    const bool last = A.rgb_out != nullptr;
    if (!A.g0 || !A.g1 || !A.src || (last ? A.dst != nullptr : A.dst == nullptr) || A.dst == A.src) return hipErrorInvalidValue;
    if (t.width == 0u || t.height == 0u || (uint64_t)t.width * t.height > kDnMaxImagePixels) return hipErrorInvalidValue;
    const uint64_t images = t.tiles_per_image ? t.n_tiles / t.tiles_per_image : 0u;
    const DnTiling want = denoise_tiling(t.width, t.height, uint32_t(images));
    if (images == 0u || images * ((uint64_t)t.width * t.height) > kDnMaxPixels || want.tiles_x != t.tiles_x || want.tiles_y != t.tiles_y ||
        want.tiles_per_image != t.tiles_per_image || want.n_tiles != t.n_tiles) return hipErrorInvalidValue;
    if (A.step == 0u || (A.step & (A.step - 1u)) != 0u || A.step > denoise_step(kDnMaxIterations - 1)) return hipErrorInvalidValue;
    if (A.normal_power_log2 < 0 || A.normal_power_log2 > kDnMaxNormalPower) return hipErrorInvalidValue;
    if (staged && (A.step > uint32_t(kDnLdsStepLimit) || denoise_lds_bytes(A.step) > kDnLdsPerCu)) return hipErrorInvalidValue;
    if (staged) return last ? launch_atrous<true, true>(A, s) : launch_atrous<true, false>(A, s);
    return last ? launch_atrous<false, true>(A, s) : launch_atrous<false, false>(A, s);
}

}  // namespace rtk
