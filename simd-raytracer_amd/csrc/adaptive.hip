// rtk_render_adaptive: the three kernels around the radiance pipeline.  A round takes the samples up to the next checkpoint of the
// pixels that are still active: k_adaptive_rays makes their camera rays (common.hip.hpp camera_ray / root_key, the frame's own),
// the streaming pipeline of rtk_accel_radiance colours them, k_adaptive_accumulate adds the colours into the running sums and the
// luminance statistics, and at the checkpoint k_adaptive_decide judges every active 8x8 block: finished, or on the next round's list.
// None of them is hot: a thread per pixel per sample, a wave per block per round, next to a pipeline that traces the rays.
#include <hip/hip_runtime.h>

#include "adaptive.hpp"
#include "frame_noise_math.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"    // (det_sincos: the GI rays' helper, static in the shared header)
#include "common.hip.hpp"
#pragma clang diagnostic pop

namespace rtk {
namespace dev {

// k_region_rays' arithmetic with the pixel taken from the list: the ray of sample `sample` of a frame whose spp is the ceiling
// (spp >= 2: the jitter branch, whose draws depend on the seed, the pixel and the sample only)
__global__ __launch_bounds__(256) void k_adaptive_rays(RenderArgs A, int sample, const uint32_t *list, uint32_t n, rtk_ray *out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t pixel = list[t];
    const uint32_t py = pixel / A.width, px = pixel - py * A.width;
    const Ray r = camera_ray(A, px, py, root_key(pcg_hash(A.seed), pixel, (uint32_t)sample));
    float *o = reinterpret_cast<float *>(out + t);
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
}

// pixel_sum += colour as k_region_accumulate does it (in sample order: all launches of a pixel are on one stream; a colour arrives
// as +0 + c), and beside it the statistic of rtk.h (frame_noise_math.hpp): y in float without contraction, S1 and S2 in double.
__global__ __launch_bounds__(256) void k_adaptive_accumulate(const uint32_t *list, uint32_t n, const float *colours, float *rgb, double *s1,
                                                             double *s2, int start) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t pixel = list[t];
    float *o = rgb + (size_t)pixel * 3;
    const float *c = colours + (size_t)t * 3;
    const V3 col = mk(c[0], c[1], c[2]);
    V3 sum = start ? mk(0.f, 0.f, 0.f) : mk(o[0], o[1], o[2]);
    sum = sum + col;
    o[0] = sum.x; o[1] = sum.y; o[2] = sum.z;
    double a = start ? 0.0 : s1[pixel], b = start ? 0.0 : s2[pixel];
    fn_add(a, b, fn_lum(col.x, col.y, col.z));
    s1[pixel] = a; s2[pixel] = b;
}

// lane i's double, i wave-uniform
__device__ __forceinline__ double lane_double(const double v, const int i) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
    return __hiloint2double(hi, lo);
}

// One wave per active block, lane l = pixel (l & 7, l >> 3) of the block.  The reduction runs over the lanes in order, which is the
// block's row-major order; a lane outside the frame adds +0 (the sums start at +0 and never hold -0, so that changes no bit).
// A block that goes on reserves its pixels and its place in the block list with ONE atomic add (adaptive_plan.hpp ad_count_word)
// and writes its valid pixels row-major behind the offset.  The order of the blocks in the next list is the order the atomics
// arrive in and NOT deterministic; no result depends on it (a pixel's samples depend on its own index only).
__global__ __launch_bounds__(256) void k_adaptive_decide(AdaptiveDecide D) {
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t unit = (uint64_t)blockIdx.x * kAdWavesPerGroup + wave_in_wg;
    if (unit >= (uint64_t)D.n_blocks) return;                                    // the last workgroup's spare waves
    const bool first = D.blocks == nullptr;
    const uint32_t block = first ? (uint32_t)unit : (uint32_t)__builtin_amdgcn_readfirstlane((int)D.blocks[unit]);
    const uint32_t blocks_x = (D.width + 7u) >> 3;
    const uint32_t by = block / blocks_x, bx = block - by * blocks_x;
    if (by * 8u >= D.height) return;                                             // purely defensive: not a block of this frame
    const uint32_t lane = __lane_id();
    const uint32_t px = bx * 8u + (lane & 7u), py = by * 8u + (lane >> 3);
    const bool valid = (px < D.width) & (py < D.height);
    const uint32_t pixel = py * D.width + px;
    const unsigned long long mask = __ballot(valid);
    const uint32_t count = (uint32_t)__popcll(mask);

    bool go_on = true;
    if (!first) {
        const double n = (double)D.n;
        double e = 0.0, m = 0.0;
        if (valid) {
            const double S1 = D.s1[pixel], S2 = D.s2[pixel];
            m = S1 / n;
            e = fn_error(S1, S2, D.n);
        }
        double se = 0.0, sm = 0.0;
        for (int i = 0; i < 64; ++i) { se += lane_double(e, i); sm += lane_double(m, i); }
        const double nb = (double)count;
        const double mean = sm / nb;
        const double den = mean < D.floor ? D.floor : mean;                      // max(mean, floor): a NaN stays one
        const double E = (se / nb) / den;
        go_on = !(E <= D.threshold) && D.last == 0;                              // a NaN keeps sampling, up to the ceiling
        if (!go_on && valid) {
            float *o = D.rgb + (size_t)pixel * 3;
            const float div = (float)D.n;
            o[0] = o[0] / div; o[1] = o[1] / div; o[2] = o[2] / div;             // render.hpp:72, as the frame of spp = n divides
            if (D.samples != nullptr) D.samples[pixel] = (uint32_t)D.n;
            if (D.noise != nullptr) D.noise[pixel] = (float)e;
        }
    }
    if (!go_on) return;
    uint64_t at_pixel, at_block;
    if (first) {
        const uint32_t y0 = by * 8u, bh = D.height - y0 < 8u ? D.height - y0 : 8u;   // adaptive_first_offset
        at_pixel = (uint64_t)y0 * D.width + (uint64_t)bx * 8u * bh;
        at_block = unit;
    } else {
        unsigned long long old = 0ull;
        if (lane == 0u) old = atomicAdd(D.count, (unsigned long long)count | (1ull << kAdCountBlockShift));
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)old);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(old >> 32));
        old = ((unsigned long long)hi << 32) | lo;
        at_pixel = old & ((1ull << kAdCountBlockShift) - 1ull);
        at_block = old >> kAdCountBlockShift;
    }
    if (lane == 0u) D.next_blocks[at_block] = block;
    if (valid) D.next_list[at_pixel + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = pixel;
}

}  // namespace dev

hipError_t launch_adaptive_rays(const dev::RenderArgs &A, int sample, const uint32_t *list, uint32_t n, rtk_ray *d_rays, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    if (!list || !d_rays || A.width == 0u || A.height == 0u || A.spp < 2 || sample < 0 || sample >= A.spp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_adaptive_rays, dim3((n + 255u) / 256u), dim3(256), 0, s, A, sample, list, n, d_rays);
    return hipGetLastError();
}

hipError_t launch_adaptive_accumulate(const uint32_t *list, uint32_t n, const float *colours, float *rgb, double *s1, double *s2,
                                      uint64_t frame_pixels, bool start, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    if (!list || !colours || !rgb || !s1 || !s2 || n > frame_pixels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_adaptive_accumulate, dim3((n + 255u) / 256u), dim3(256), 0, s, list, n, colours, rgb, s1, s2, start ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_adaptive_decide(const dev::AdaptiveDecide &D, hipStream_t s) {
    if (D.n_blocks == 0u) return hipSuccess;
    // whoever did not make the arguments consistent gets an error, not a kernel that indexes by them
    const uint64_t frame_blocks = adaptive_blocks(D.width, D.height);
    if (D.width == 0u || D.height == 0u || (uint64_t)D.width * D.height > kAdaptiveMaxPixels || D.n_blocks > frame_blocks) return hipErrorInvalidValue;
    if (!D.rgb || !D.s1 || !D.s2 || !D.next_blocks || !D.next_list) return hipErrorInvalidValue;
    if (D.blocks == nullptr ? D.n_blocks != frame_blocks : (D.n < 2 || D.count == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_adaptive_decide, dim3(adaptive_groups(D.n_blocks)), dim3(64u * kAdWavesPerGroup), 0, s, D);
    return hipGetLastError();
}

}  // namespace rtk
