// The statistic of rtk_render_frame_noise (rtk.h; item 3 of rtk_render_adaptive's contract at n = spp), once for host and device:
// the luminance of a sample colour, the update of a pixel's two running sums, and the standard error of its mean luminance.
// k_frame_moments (frame_noise.hip), k_adaptive_accumulate / k_adaptive_decide (adaptive.hip) and
// tests/cpp/frame_noise_plan_check.cpp all compile exactly these expressions; the library and the check are built with
// -ffp-contract=off, so no side fuses a product into a sum.
#pragma once

#if defined(__HIPCC__)
#define RTK_FN_HD __host__ __device__ inline
#else
#define RTK_FN_HD inline
#endif

namespace rtk {

// y of a sample colour, in float, in the order rtk.h writes it
RTK_FN_HD float fn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// S1 += y, S2 += y * y, in double; the callers add a pixel's samples in sample order
RTK_FN_HD void fn_add(double &s1, double &s2, float y) {
    s1 += (double)y;
    s2 += (double)y * (double)y;
}

// e_i at n samples (n >= 2): v = max(0, (S2 - S1 * S1 / n) / (n - 1)) / n, e = sqrt(v), all in double.  max(0, x) is written
// `x < 0 ? 0 : x`: rounding may leave x a hair below zero for a constant pixel (clamped), and a NaN stays one.
RTK_FN_HD double fn_error(double s1, double s2, int n_samples) {
    const double n = (double)n_samples;
    const double x = (s2 - s1 * s1 / n) / (n - 1.0);
    const double v = (x < 0.0 ? 0.0 : x) / n;
    return __builtin_sqrt(v);
}

}  // namespace rtk
