// The arithmetic that rtk_temporal_accumulate_clamped (rtk.h) adds to temporal_math.hpp, which it includes and leaves as it is:
// the box statistics of the NEW frame's neighbourhood (step 3a), the bounds they give (3b), the clamp of the history's colour (3c)
// and the blend with the variance floor and the shortened history of a clamped pixel (3d, 4).  One copy for the kernel
// (temporal_clamp.hip) and the host check program (tests/cpp/temporal_clamp_math_check.cpp); tests/temporal_clamp_model.py is the
// same arithmetic in numpy.  Everything is float, in the order rtk.h writes it, and relies on -ffp-contract=off.  No HIP, no plan.
#pragma once

#include "temporal_math.hpp"

namespace rtk {
namespace tp {

struct Box { float nf, s1[3], s2[3], sv; };                    // step 3a: accepted taps, sums of c and c * c per channel, sum of var
struct Bounds { float lo[3], hi[3]; };

RTK_TP_FN Box box_empty() { return Box{0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f}; }

// step 3a, one accepted tap: its colour and var = noise_q * noise_q or 1
RTK_TP_FN void box_add(Box &b, const float c[3], float var) {
    b.nf = b.nf + 1.0f;
    for (int ch = 0; ch < 3; ++ch) {
        b.s1[ch] = b.s1[ch] + c[ch];
        b.s2[ch] = b.s2[ch] + c[ch] * c[ch];
    }
    b.sv = b.sv + var;
}

// step 3b (nf >= 1: the centre tap always passes)
RTK_TP_FN Bounds bounds(const Box &b, float gamma) {
    Bounds o;
    for (int ch = 0; ch < 3; ++ch) {
        const float m = b.s1[ch] / b.nf;
        float d = b.s2[ch] / b.nf - m * m;
        d = d > 0.0f ? d : 0.0f;                                // (a NaN becomes 0: the bounds are then m, which is NaN as well)
        const float sg = (float)__builtin_sqrt((double)d);
        const float e = gamma * sg;
        o.lo[ch] = m - e;
        o.hi[ch] = m + e;
    }
    return o;
}

// step 3c: hc = sum_c / sum_w per channel, clamped in place -> whether some comparison fired
RTK_TP_FN bool clamp_to(const Bounds &b, float hc[3]) {
    bool clamped = false;
    for (int ch = 0; ch < 3; ++ch) {
        const float v = hc[ch];
        const bool below = v < b.lo[ch], above = v > b.hi[ch];
        hc[ch] = below ? b.lo[ch] : (above ? b.hi[ch] : v);
        clamped = clamped || below || above;
    }
    return clamped;
}

// steps 3b to 4 for a pixel with history: temporal_math.hpp blend with hc', the variance floor and the kept share of the length
RTK_TP_FN Blend blend_clamped(const Consts &k, float gamma, float history_keep, const Pixel &p, const Sums &s, const Box &b, bool *was_clamped = nullptr) {
    Blend o;
    float hc[3] = {s.c[0] / s.w, s.c[1] / s.w, s.c[2] / s.w};
    const bool clamped = clamp_to(bounds(b, gamma), hc);
    float hv = s.v / (s.w * s.w);
    float L = s.l / s.w;
    if (clamped) {
        const float vb = (b.sv / b.nf) / b.nf;
        hv = hv > vb ? hv : vb;
        L = L * history_keep;
    }
    float N = L + 1.0f;
    N = N < k.nmax ? N : k.nmax;
    const float a = max_of(1.0f / N, k.alpha_min), om = 1.0f - a;
    for (int ch = 0; ch < 3; ++ch) o.c[ch] = (om * hc[ch]) + (a * p.c[ch]);
    const float var = ((om * om) * hv) + ((a * a) * p.var);
    o.noise = (float)__builtin_sqrt((double)var);
    o.length = N;
    if (was_clamped) *was_clamped = clamped;
    return o;
}

}  // namespace tp
}  // namespace rtk
