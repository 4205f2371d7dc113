// Device helpers shared by the megakernel (kernels.hip) and the streaming pipeline (stream.hip).
#pragma once

#include "kernels.hpp"

namespace rtk {
namespace dev {

// Counter-based RNG.  The reference's thread_local minstd_rand (utils/rand.hpp:5-19) is seeded identically on every
// thread and handed out by a racy tile queue, so its stream cannot be reproduced.  Here a draw is
// keyed by the POSITION OF A RAY IN ITS SAMPLE'S RAY TREE: root key = f(seed, absolute pixel, sample); a secondary
// ray's key derives from its parent ray's key and its child index; draw j at a ray is a pure function of (key, j).
// Frames therefore depend neither on the wave / bucket / rank layout nor on the order in which a traversal visits
// the tree (recursive CPU code, the per-lane state machine and the level-by-level wavefront draw the same numbers).
// det_sincos is a fixed double-precision sin/cos (Cody-Waite + Taylor) standing in for
// std::sin/std::cos(float) at render.hpp:160-167: integer and IEEE-double operations only.
__device__ __forceinline__ uint32_t pcg_hash(uint32_t x) {
    const uint32_t s = x * 747796405u + 2891336453u;
    const uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
    return (w >> 22u) ^ w;
}
__device__ __forceinline__ uint32_t root_key(uint32_t seed_hash, uint32_t pixel, uint32_t sample) {
    return pcg_hash(sample + pcg_hash(pixel + seed_hash));                  // seed_hash = pcg_hash(seed)
}
__device__ __forceinline__ uint32_t child_key(uint32_t key, uint32_t child) { return pcg_hash(key ^ (0x632BE5ABu * (child + 1u))); }
__device__ __forceinline__ float urand_key(uint32_t key, uint32_t j) {
    const uint32_t h = pcg_hash(key + j * 0x9E3779B9u + 0x85EBCA6Bu);
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

static __device__ __noinline__ void det_sincos(float angle, float &s, float &c) {
    const double x = (double)angle;
    const double two_over_pi = 0.63661977236758134308;
    const double pio2_hi = 1.57079632673412561417e+00, pio2_lo = 6.07710050650619224932e-11;
    const double kf = __builtin_floor(x * two_over_pi + 0.5);
    const double r = (x - kf * pio2_hi) - kf * pio2_lo;
    const double r2 = r * r;
    double ps = -1.0 / 1307674368000.0;
    ps = ps * r2 + 1.0 / 6227020800.0;
    ps = ps * r2 - 1.0 / 39916800.0;
    ps = ps * r2 + 1.0 / 362880.0;
    ps = ps * r2 - 1.0 / 5040.0;
    ps = ps * r2 + 1.0 / 120.0;
    ps = ps * r2 - 1.0 / 6.0;
    const double sr = r + r * (r2 * ps);
    double pc = 1.0 / 20922789888000.0;
    pc = pc * r2 - 1.0 / 87178291200.0;
    pc = pc * r2 + 1.0 / 479001600.0;
    pc = pc * r2 - 1.0 / 3628800.0;
    pc = pc * r2 + 1.0 / 40320.0;
    pc = pc * r2 - 1.0 / 720.0;
    pc = pc * r2 + 1.0 / 24.0;
    pc = pc * r2 - 0.5;
    const double cr = 1.0 + r2 * pc;
    const long long k = (long long)kf;
    double sv, cv;
    switch ((int)(k & 3)) {
        case 0: sv = sr; cv = cr; break;
        case 1: sv = cr; cv = -sr; break;
        case 2: sv = -sr; cv = -cr; break;
        default: sv = -cr; cv = sr; break;
    }
    s = (float)sv;
    c = (float)cv;
}

// sample(texture, hit, uvs) (scene/texture/albedo.hpp:9-11, edge.hpp:12-21, checker.hpp:13-28, bitmap.hpp:46-59).
// hit_w is evaluated in double there (`1. - hit_u - hit_v` with a double literal) and rounded to float.
__device__ __forceinline__ V3 sample_texture(const DevTexture *T, const DevTriUv *uv, const float u, const float v,
                                             const uint8_t *tex_pixels) {
    const V3 a = mk(T->a[0], T->a[1], T->a[2]), b = mk(T->b[0], T->b[1], T->b[2]);
    if (T->kind == RTK_TEX_ALBEDO) return a;
    const float w = (float)((1.0 - (double)u) - (double)v);
    if (T->kind == RTK_TEX_EDGES) return (u < T->param || v < T->param || w < T->param) ? a : b;
    const float fx = (w * uv->uv[0] + u * uv->uv[2]) + v * uv->uv[4];          // hit_w * uvs.x + hit_u * uvs.y + hit_v * uvs.z
    const float fy = (w * uv->uv[1] + u * uv->uv[3]) + v * uv->uv[5];
    if (T->kind == RTK_TEX_BITMAP) {
        // bitmap.hpp:53-59: `size_t row = (1. - final_uv.y) * height` is a double product, `size_t column = final_uv.x * width` a
        // float one (the size_t converts to F); both truncate.  A negative value is undefined there: x86-64 yields 0 above -1 and
        // a huge number (clamped to the last row / column) below, which is what is done here.
        const int bw = T->bmp[0], bh = T->bmp[1];
        const double rd = (1.0 - (double)fy) * (double)bh;
        const float cf = fx * (float)bw;
        const long long ri = (long long)rd, ci = (long long)cf;      // NaN converts to 0 on the device; on x86 to INT64_MIN (last row)
        const int row = (ri < 0 || ri > bh - 1 || rd != rd) ? bh - 1 : (int)ri;
        const int col = (ci < 0 || ci > bw - 1 || cf != cf) ? bw - 1 : (int)ci;
        const uint8_t *px = tex_pixels + (size_t)T->bmp[2] + ((size_t)row * (size_t)bw + (size_t)col) * 3u;
        const float color_scale = (float)(1.0 / 255.0);              // bitmap.hpp:19
        return mk((float)px[0] * color_scale, (float)px[1] * color_scale, (float)px[2] * color_scale);
    }
    const int u2 = (int)(fx / T->param), v2 = (int)(fy / T->param);
    return ((u2 + v2) % 2 == 0) ? a : b;
}

// Unlit occlusion queries (RenderArgs::skip_unlit).  The light loop (render.hpp:184-208, :213-236) computes
// contrib = (intensity / area) * cosine, asks is_occluded, and adds `contrib * albedo` only if the answer is "clear".  When that
// addend compares equal to 0.0f in all three channels (+0 or -0) the answer cannot change the pixel, so the ray is counted but
// never traced, and the lane is treated as clear:
//  1. x + (+-0) has the bits of x for every x that is not -0 (a NaN stays the NaN it was).  The sums the addend goes into
//     (`final_color` there; acc, Frame::a[9..11] and k_combine's acc here) start as +0 and are only ever results of float
//     additions; under round-to-nearest a sum is -0 only if both operands are -0, so a chain that starts at +0 never holds -0.
//     Adding the +-0 (clear) and not adding it (occluded) give the same bits.
//  2. The test is on the addend, not on the cosine: a NaN or infinite contrib or albedo (inf * 0) makes a NaN addend, which does
//     not compare equal to zero, and the ray is traced as ever.  Lights of intensity 0, lights behind or in the plane of the
//     surface and black albedos need no case of their own.
//  3. is_occluded (render.hpp:110-131) has no effect but its accel.intersect calls: exactly one when 0 < radius and no material
//     is transmissive -- still counted in `rays`.  With transmissive materials the number of calls depends on the walk, and the
//     host leaves the rule off (as under collect_stats == 1, which reports the reference's per-ray work).
// One float per lane carries the albedo to whoever computes contrib (the helper waves of a light burst): |contrib * a_c| =
// round(|contrib| * |a_c|) is monotone in |a_c|, so all three channels are +-0 exactly when the channel of largest magnitude
// is; a NaN channel never is, hence the NaN.  An infinite channel gives inf or NaN, never 0.
__device__ __forceinline__ float albedo_reach(const V3 a) {
    const float x = __builtin_fabsf(a.x), y = __builtin_fabsf(a.y), z = __builtin_fabsf(a.z);
    const float m = x < y ? (y < z ? z : y) : (x < z ? z : x);
    return (x != x || y != y || z != z) ? __builtin_nanf("") : m;
}
__device__ __forceinline__ bool unlit_query(const float contrib, const float reach) { return contrib * reach == 0.0f; }

// Camera ray of pixel (px, py) (render.hpp:35-62); `key` is the sample's root key (draws 0 and 1 jitter the sample).
// `pos` [3], `M` [9]: the camera -- the launch arguments' own (camera_ray), or a view of the table of a views launch.
__device__ __forceinline__ Ray camera_ray_of(const RenderArgs &A, const float *pos, const float *M, const uint32_t px, const uint32_t py,
                                             const uint32_t key) {
    float rx = (float)px, ry = (float)py;
    if (A.spp == 1) { rx += 0.5f; ry += 0.5f; }
    else {
        rx += urand_key(key, 0u);
        ry += urand_key(key, 1u);
    }
    const float ndc_x = rx / A.width_f, ndc_y = ry / A.height_f;  // render.hpp:43-44 ((float)width, (float)height: RenderArgs)
    float sx = (2.0f * ndc_x) - 1.0f;
    float sy = 1.0f - (2.0f * ndc_y);
    sx *= A.aspect;
    sx *= A.tan_half_fov;                                       // render.hpp:55-57: float *= tanf(float) (host, api_frame.hip camera_args)
    sy *= A.tan_half_fov;
    // transpose(camera.matrix) * dir
    V3 d = mk(M[0] * sx + M[3] * sy + M[6] * -1.0f, M[1] * sx + M[4] * sy + M[7] * -1.0f,
              M[2] * sx + M[5] * sy + M[8] * -1.0f);
    d = normalized(d);
    return make_ray(mk(pos[0], pos[1], pos[2]), d);
}
__device__ __forceinline__ Ray camera_ray(const RenderArgs &A, const uint32_t px, const uint32_t py, const uint32_t key) {
    return camera_ray_of(A, A.cam_pos, A.cam_mat, px, py, key);
}

}  // namespace dev
}  // namespace rtk
