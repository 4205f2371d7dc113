// The arithmetic of rtk_temporal_accumulate (rtk.h), one copy of each step as in denoise_math.hpp: the projection of a pixel's
// world position into the previous view, the tests a tap of the history must pass, the accumulation of the four taps and the blend,
// as plain inline functions for host and device.  The kernel (temporal.hip) and the host check program
// (tests/cpp/temporal_math_check.cpp) both include it; tests/temporal_model.py is the same arithmetic in numpy.  Everything is
// float, in the order rtk.h writes it, and relies on -ffp-contract=off.  No transcendental function, and no float -> int
// conversion before the range test has passed.  No HIP, no plan.
#pragma once

#ifndef RTK_TP_FN
#if defined(__HIPCC__)
#define RTK_TP_FN __host__ __device__ inline
#else
#define RTK_TP_FN inline
#endif
#endif
#if defined(__clang__)
#define RTK_TP_UNROLL _Pragma("unroll")
#else
#define RTK_TP_UNROLL
#endif

namespace rtk {
namespace tp {

// what the host computes once per call (temporal_plan.hpp temporal_consts)
struct Consts {
    float cam[3], m[9];                // the PREVIOUS view: position, matrix row-major
    float th, aspect, wf, hf, nmax;    // tanf(fov / 2), w / h, (float)w, (float)h, (float)max_history
    float alpha_min, plane_tolerance, normal_min_dot;
};

struct Pixel { float c[3], var, P[3], n[3], depth; };          // the new frame at p: var = noise * noise or 1
struct Tap { float c[3], var, length; };                       // an accepted tap of the history: var = noise_q * noise_q or 1
struct Foot { int x0, y0; float tx, ty; };                     // the four taps (x0 + i, y0 + j) and their bilinear fractions
struct Sums { float c[3], v, l, w; };
struct Blend { float c[3], noise, length; };

RTK_TP_FN bool is_hit(float depth) { return depth >= 0.0f; }   // (a NaN is no hit)
RTK_TP_FN float max_of(float x, float f) { return x > f ? x : f; }
RTK_TP_FN float abs_of(float x) { return __builtin_fabsf(x); }

// step 2 of rtk.h up to its range test: where P lies in the previous frame, in pixels; false = not in front of that camera.
// (rtk_render_motion stops here: motion_math.hpp.)
RTK_TP_FN bool place(const Consts &k, const float P[3], float &fx, float &fy) {
    const float dx = P[0] - k.cam[0], dy = P[1] - k.cam[1], dz = P[2] - k.cam[2];
    const float cx = (k.m[0] * dx + k.m[1] * dy) + k.m[2] * dz;
    const float cy = (k.m[3] * dx + k.m[4] * dy) + k.m[5] * dz;
    const float cz = (k.m[6] * dx + k.m[7] * dy) + k.m[8] * dz;
    if (!(cz < 0.0f)) return false;
    const float iz = -cz;
    const float qx = cx / iz, qy = cy / iz;
    const float ux = (qx / k.th) / k.aspect, uy = qy / k.th;
    fx = ((ux + 1.0f) * 0.5f) * k.wf - 0.5f;
    fy = ((1.0f - uy) * 0.5f) * k.hf - 0.5f;
    return true;
}

// step 2 of rtk.h: false = P does not land in the previous frame
RTK_TP_FN bool project(const Consts &k, const float P[3], Foot &f) {
    float fx, fy;
    if (!place(k, P, fx, fy)) return false;
    if (!(fx > -1.0f && fx < k.wf && fy > -1.0f && fy < k.hf)) return false;      // (a NaN or an infinity fails)
    // only now: both lie in (-1, 16384), so the floors convert exactly
    const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
    f.x0 = (int)x0f; f.y0 = (int)y0f;
    f.tx = fx - x0f; f.ty = fy - y0f;
    return true;
}

// step 3, the tests in the order a tap loads its planes: depth and length first ...
RTK_TP_FN bool tap_alive(float depth_q, float length_q) { return depth_q >= 0.0f && length_q >= 1.0f; }
// ... then normal and position
RTK_TP_FN bool tap_on_surface(const Consts &k, const Pixel &p, const float nq[3], const float Pq[3]) {
    const float t = (p.n[0] * nq[0] + p.n[1] * nq[1]) + p.n[2] * nq[2];
    if (!(t >= k.normal_min_dot)) return false;
    const float ex = Pq[0] - p.P[0], ey = Pq[1] - p.P[1], ez = Pq[2] - p.P[2];
    const float pd = (p.n[0] * ex + p.n[1] * ey) + p.n[2] * ez;
    return abs_of(pd) <= k.plane_tolerance * p.depth;
}

RTK_TP_FN void accumulate(Sums &s, float w, const Tap &q) {
    s.c[0] = s.c[0] + w * q.c[0]; s.c[1] = s.c[1] + w * q.c[1]; s.c[2] = s.c[2] + w * q.c[2];
    s.v = s.v + (w * w) * q.var;
    s.l = s.l + w * q.length;
    s.w = s.w + w;
}

// Steps 2 and 3 for one HIT pixel p.  fetch(qx, qy, q) -> bool hands out the tap of the history at (qx, qy), or false when it lies
// outside the image or fails a test (tap_alive, the mesh ids, tap_on_surface).  -> history exists.
template <typename Fetch>
RTK_TP_FN bool history(const Consts &k, const Pixel &p, Sums &s, Fetch &&fetch) {
    s = Sums{{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f};
    Foot f;
    if (!project(k, p.P, f)) return false;
    RTK_TP_UNROLL
    for (int j = 0; j < 2; ++j) {
        RTK_TP_UNROLL
        for (int i = 0; i < 2; ++i) {
            const float w = (j ? f.ty : 1.0f - f.ty) * (i ? f.tx : 1.0f - f.tx);
            Tap q;
            if (!fetch(f.x0 + i, f.y0 + j, q)) continue;
            accumulate(s, w, q);
        }
    }
    return s.w > 0.0f;
}

// step 4
RTK_TP_FN Blend blend(const Consts &k, const Pixel &p, const Sums &s) {
    Blend o;
    const float hv = s.v / (s.w * s.w);
    float N = s.l / s.w + 1.0f;
    N = N < k.nmax ? N : k.nmax;
    const float a = max_of(1.0f / N, k.alpha_min), om = 1.0f - a;
    for (int ch = 0; ch < 3; ++ch) {
        const float hc = s.c[ch] / s.w;
        o.c[ch] = (om * hc) + (a * p.c[ch]);
    }
    const float var = ((om * om) * hv) + ((a * a) * p.var);
    o.noise = (float)__builtin_sqrt((double)var);
    o.length = N;
    return o;
}

}  // namespace tp
}  // namespace rtk
