// The arithmetic of rtk_denoise_frame (rtk.h), one copy of each formula as in shade.hip.hpp: the prologue, the weight of a tap, the
// accumulation, the walk over the 25 taps of a pixel and the epilogue, as plain inline functions for host and device.  The kernels
// (denoise.hip) and the host check program (tests/cpp/denoise_math_check.cpp) both include it; tests/denoise_model.py is the same
// arithmetic in numpy.  Everything is float, in the order rtk.h writes it, and relies on -ffp-contract=off.  No HIP, no plan.
#pragma once

#ifndef RTK_DN_FN
#if defined(__HIPCC__)
#define RTK_DN_FN __host__ __device__ inline
#else
#define RTK_DN_FN inline
#endif
#endif
#if defined(__clang__)
#define RTK_DN_UNROLL _Pragma("unroll")
#else
#define RTK_DN_UNROLL
#endif

namespace rtk {
namespace dn {

constexpr float kCentreWeight = 0.140625f;         // (3/8)^2, given as a constant: the centre tap has no edge-stopping terms
constexpr float kDenEps = 1e-8f;

struct Rgbv { float r, g, b, var; };               // the filtered signal of a pixel: a 16-byte record
struct Guide { float nx, ny, nz, px, py, pz; };    // what steers the weights: never changes
struct Tap { Rgbv c; Guide g; };

RTK_DN_FN bool is_hit(float depth) { return depth >= 0.0f; }      // (a NaN is no hit)
RTK_DN_FN float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
RTK_DN_FN float max_of(float x, float f) { return x > f ? x : f; }
RTK_DN_FN float tap_h(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }     // h[i], i = d + 2

// rgb, albedo: three floats of the pixel (albedo null = no plane); noise: the pixel's value, null = no plane
RTK_DN_FN Rgbv prologue(const float *rgb, const float *albedo, const float *noise, bool hit, float albedo_floor) {
    Rgbv o;
    o.r = rgb[0]; o.g = rgb[1]; o.b = rgb[2];
    o.var = noise ? *noise * *noise : 1.0f;
    if (albedo && hit) {
        const float ar = max_of(albedo[0], albedo_floor), ag = max_of(albedo[1], albedo_floor), ab = max_of(albedo[2], albedo_floor);
        o.r = o.r / ar; o.g = o.g / ag; o.b = o.b / ab;
        const float la = lum(ar, ag, ab);
        o.var = o.var / (la * la);
    }
    return o;
}

// out[3] = the pixel's colour as it leaves; a miss, or a frame without albedo, leaves with c's bits
RTK_DN_FN void epilogue(const Rgbv &c, const float *albedo, bool hit, float albedo_floor, float *out) {
    if (albedo && hit) {
        out[0] = c.r * max_of(albedo[0], albedo_floor);
        out[1] = c.g * max_of(albedo[1], albedo_floor);
        out[2] = c.b * max_of(albedo[2], albedo_floor);
    } else {
        out[0] = c.r; out[1] = c.g; out[2] = c.b;
    }
}

// step 4 of rtk.h: hh = h[dy + 2] * h[dx + 2], lp = lum(c_p), den = sl2 * var_p + 1e-8f
RTK_DN_FN float tap_weight(float hh, const Guide &p, const Tap &q, float lp, float den, float sp2, int normal_power_log2) {
    float t = (p.nx * q.g.nx + p.ny * q.g.ny) + p.nz * q.g.nz;
    t = t > 0.0f ? t : 0.0f;
    for (int i = 0; i < normal_power_log2; ++i) t = t * t;
    const float dx = q.g.px - p.px, dy = q.g.py - p.py, dz = q.g.pz - p.pz;
    const float pd = (p.nx * dx + p.ny * dy) + p.nz * dz;
    const float wd = 1.0f / (1.0f + (pd * pd) / sp2);
    const float dl = lum(q.c.r, q.c.g, q.c.b) - lp;
    const float wl = 1.0f / (1.0f + (dl * dl) / den);
    return ((hh * t) * wd) * wl;
}

struct Sums { float r, g, b, v, w; };
RTK_DN_FN void accumulate(Sums &s, float w, const Rgbv &q) {
    s.r = s.r + w * q.r; s.g = s.g + w * q.g; s.b = s.b + w * q.b;
    s.v = s.v + (w * w) * q.var;
    s.w = s.w + w;
}

// One iteration for one HIT pixel p.  fetch(dx, dy, q) -> bool hands out the tap q = p + s * (dx, dy) of the previous iteration, or
// false when it lies outside the image or is no hit; it is never asked for the centre, which is p itself.
template <typename Fetch>
RTK_DN_FN Rgbv filter_pixel(const Tap &p, float sl2, float sp2, int normal_power_log2, Fetch &&fetch) {
    const float lp = lum(p.c.r, p.c.g, p.c.b), den = sl2 * p.c.var + kDenEps;
    Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    RTK_DN_UNROLL
    for (int dy = -2; dy <= 2; ++dy) {
        RTK_DN_UNROLL
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) { accumulate(s, kCentreWeight, p.c); continue; }
            Tap q;
            if (!fetch(dx, dy, q)) continue;
            accumulate(s, tap_weight(tap_h(dy + 2) * tap_h(dx + 2), p.g, q, lp, den, sp2, normal_power_log2), q.c);
        }
    }
    Rgbv o;
    o.r = s.r / s.w; o.g = s.g / s.w; o.b = s.b / s.w;
    o.var = s.v / (s.w * s.w);
    return o;
}

}  // namespace dn
}  // namespace rtk
