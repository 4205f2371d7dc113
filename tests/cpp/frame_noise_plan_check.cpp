// Stand-alone host program over csrc/frame_noise_plan.hpp and csrc/frame_noise_math.hpp (tests/test_cpp_frame_noise_plan.py): the
// refusals in rtk.h's order, the workspace, what a batch does with the running sums, the adaptive call of the overflow redo, and
// the statistic against a recomputation in long double.  No HIP, no device.  Built with -ffp-contract=off, like the library.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "adaptive_plan.hpp"
#include "frame_noise_math.hpp"
#include "frame_noise_plan.hpp"

using namespace rtk;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static rtk_render_params good() {
    rtk_render_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = 70; p.height = 36; p.spp = 8; p.max_ray_depth = 5; p.fov_degrees = 90.0; p.trace_mode = RTK_TRACE_STREAM;
    return p;
}
static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }

static void refusals() {
    CHECK(frame_noise_refusal(good(), 70, 36) == nullptr);
    { auto p = good(); p.trace_mode = RTK_TRACE_AUTO; CHECK(frame_noise_refusal(p, 70, 36) == nullptr); }
    // every refusal alone, in all its forms
    for (int m : {RTK_TRACE_LANE, RTK_TRACE_WAVE, RTK_TRACE_GROUP4, RTK_TRACE_GROUP8, RTK_TRACE_GROUP16, RTK_TRACE_TWOPASS}) {
        auto p = good(); p.trace_mode = m; CHECK(says(frame_noise_refusal(p, 70, 36), "RTK_TRACE_AUTO or RTK_TRACE_STREAM"));
    }
    { auto p = good(); p.spp = 1; CHECK(says(frame_noise_refusal(p, 70, 36), "spp >= 2")); p.spp = 2; CHECK(frame_noise_refusal(p, 70, 36) == nullptr); }
    { auto p = good(); p.sample_count = 8; CHECK(says(frame_noise_refusal(p, 70, 36), "not progressive"));
      p.sample_count = 3; CHECK(says(frame_noise_refusal(p, 70, 36), "not progressive"));
      p.sample_begin = 2; p.sample_count = 2; CHECK(says(frame_noise_refusal(p, 70, 36), "not progressive")); }
    for (int st : {1, 2}) { auto p = good(); p.collect_stats = st; CHECK(says(frame_noise_refusal(p, 70, 36), "statistics")); }
    { auto p = good(); p.world_size = 2; CHECK(says(frame_noise_refusal(p, 70, 36), "not sharded")); p.world_size = 1; CHECK(frame_noise_refusal(p, 70, 36) == nullptr); }
    CHECK(frame_noise_refusal(good(), 1u << 16, 1u << 15) == nullptr);                          // 2^31 pixels are the most
    CHECK(says(frame_noise_refusal(good(), (1u << 16), (1u << 15) + 1u), "too many pixels"));
    CHECK(says(frame_noise_refusal(good(), 1u << 16, 1u << 16), "too many pixels"));
    // the order: a call that is wrong in the ways k, k + 1, ... names way k
    auto p = good();
    CHECK(says(frame_noise_refusal(p, 1u << 16, 1u << 16), "too many pixels"));
    p.world_size = 2; CHECK(says(frame_noise_refusal(p, 1u << 16, 1u << 16), "not sharded"));
    p.collect_stats = 1; CHECK(says(frame_noise_refusal(p, 1u << 16, 1u << 16), "statistics"));
    p.sample_begin = 1; p.sample_count = 1; CHECK(says(frame_noise_refusal(p, 1u << 16, 1u << 16), "not progressive"));
    p.spp = 1; p.sample_begin = 0; CHECK(says(frame_noise_refusal(p, 1u << 16, 1u << 16), "spp >= 2"));
    p.trace_mode = RTK_TRACE_GROUP4; CHECK(says(frame_noise_refusal(p, 1u << 16, 1u << 16), "RTK_TRACE_AUTO or RTK_TRACE_STREAM"));
    std::printf("refusals ok\n");
}

static void plan() {
    CHECK(kFrameNoiseMaxPixels == kAdaptiveMaxPixels);                                          // the redo takes every frame this call takes
    CHECK(frame_noise_workspace_bytes(0) == 0 && frame_noise_workspace_bytes(1) == 16 && frame_noise_workspace_bytes(2520) == 40320);
    CHECK(frame_noise_workspace_bytes(uint64_t(1) << 31) == uint64_t(1) << 35);                 // 64-bit safe
    // spp 8 in batches of 3: 3, 3, 2; one batch that is first and last; a batch per sample
    CHECK(frame_noise_batch(0, 3, 8).starts && !frame_noise_batch(0, 3, 8).ends);
    CHECK(!frame_noise_batch(3, 3, 8).starts && !frame_noise_batch(3, 3, 8).ends);
    CHECK(!frame_noise_batch(6, 2, 8).starts && frame_noise_batch(6, 2, 8).ends);
    CHECK(frame_noise_batch(0, 2, 2).starts && frame_noise_batch(0, 2, 2).ends);
    for (int s = 0; s < 8; ++s) { const FrameNoiseBatch b = frame_noise_batch(s, 1, 8); CHECK(b.starts == (s == 0) && b.ends == (s == 7)); }
    CHECK(frame_noise_batch(0x7FFFFFFF - 1, 1, 0x7FFFFFFF).ends && !frame_noise_batch(0x7FFFFFFF - 1, 0xFFFFFFFFu, 0x7FFFFFFF).ends);
    // the redo is an adaptive render that the adaptive call accepts and that has one checkpoint, the ceiling
    for (int spp : {2, 3, 8, 128, 0x7FFFFFFF}) {
        auto p = good(); p.spp = spp;
        const rtk_adaptive_params ap = frame_noise_redo(p);
        CHECK(ap.min_samples == spp && ap.step == 1 && ap.threshold == 0.0f && ap.floor == 1.0f);
        CHECK(adaptive_refusal(p, ap, 70, 36) == nullptr);
        CHECK(adaptive_next_checkpoint(0, spp, ap.min_samples, ap.step) == spp && adaptive_checkpoints(spp, ap.min_samples, ap.step) == 1);
    }
    std::printf("plan ok\n");
}

// e of a sequence as the kernel takes it: sums in sample order, in any split into batches
static double e_of(const std::vector<float> &y) {
    double s1 = 0.0, s2 = 0.0;
    for (float v : y) fn_add(s1, s2, v);
    return fn_error(s1, s2, int(y.size()));
}
// ... and recomputed in long double from the same floats
static long double e_long(const std::vector<float> &y, long double *S2_out) {
    long double S1 = 0.0L, S2 = 0.0L;
    for (float v : y) { S1 += (long double)v; S2 += (long double)v * (long double)v; }
    const long double n = (long double)y.size();
    long double x = (S2 - S1 * S1 / n) / (n - 1.0L);
    if (x < 0.0L) x = 0.0L;
    *S2_out = S2;
    return sqrtl(x / n);
}

static void math() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // y: float products and sums in the written order; -0 and +0 colours give +0 or -0, which the sums cannot tell apart
    const float r = 0.3f, g = 0.6f, b = 0.9f;
    const float t0 = 0.2126f * r, t1 = 0.7152f * g, t2 = 0.0722f * b;
    const float t01 = t0 + t1;
    CHECK(fn_lum(r, g, b) == t01 + t2);
    CHECK(fn_lum(0.0f, 0.0f, 0.0f) == 0.0f && fn_lum(-0.0f, -0.0f, -0.0f) == 0.0f && fn_lum(1.0f, 1.0f, 1.0f) == (0.2126f + 0.7152f) + 0.0722f);
    CHECK(std::isnan(fn_lum(nan, 0.0f, 0.0f)));
    { double s1 = 0.0, s2 = 0.0; fn_add(s1, s2, -0.0f); CHECK(s1 == 0.0 && !std::signbit(s1) && s2 == 0.0 && !std::signbit(s2));
      fn_add(s1, s2, 0.5f); fn_add(s1, s2, 0.25f); CHECK(s1 == 0.75 && s2 == 0.3125); }
    // 1. a constant y: every operation is exact (n * y and n * n * y * y fit 53 bits here), so v is exactly 0
    for (int n : {2, 4, 8, 16}) CHECK(e_of(std::vector<float>(size_t(n), 0.2126f)) == 0.0);
    for (int n : {3, 5, 7, 100}) CHECK(e_of(std::vector<float>(size_t(n), 0.75f)) == 0.0);
    CHECK(e_of(std::vector<float>(8, 0.0f)) == 0.0 && !std::signbit(e_of(std::vector<float>(8, 0.0f))));
    // 2. a constant y of 24 significant bits a hundred or a thousand times: the partial sums of S2 no longer fit 53 bits and round.
    //    The first one, searched in a fixed order, for which that leaves x < 0: max(0, x) makes it a zero, not the NaN a square root
    //    of it would be
    bool found = false;
    for (int n : {100, 1000}) {
        float y = 0.1f;
        for (int k = 0; k < 4096 && !found; ++k, y = std::nextafterf(y, 1.0f)) {
            double s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < n; ++i) fn_add(s1, s2, y);
            const double x = (s2 - s1 * s1 / double(n)) / (double(n) - 1.0);
            if (x < 0.0) {
                found = true;
                const double e = fn_error(s1, s2, n);
                CHECK(e == 0.0 && !std::isnan(e));
                std::printf("x < 0 by rounding: n = %d, y = %.9g, x = %.3g\n", n, double(y), x);
            }
        }
    }
    CHECK(found);
    // 3. a NaN sample stays one, wherever it stands
    for (size_t at : {size_t(0), size_t(3), size_t(7)}) {
        std::vector<float> y(8, 0.5f);
        y[at] = nan;
        CHECK(std::isnan(e_of(y)));
    }
    CHECK(std::isnan(e_of({std::numeric_limits<float>::infinity(), 1.0f})));                    // (inf - inf)
    // 4. sequences against long double.  With u = 2^-53: the products y * y are exact, S2 takes n - 1 rounded additions (relative
    //    (n - 1) u), S1 as many, which S1 * S1 doubles, and the product and the division by n add one u each; S1 * S1 / n <= S2
    //    (Cauchy-Schwarz), so S2 - S1 * S1 / n is off by at most 3 n u S2, and v = e * e by at most 3 n u S2 / (n (n - 1)), plus a
    //    relative 2^-50 for the remaining operations.
    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return float(lcg >> 8) * (1.0f / 16777216.0f); };
    const std::vector<std::vector<float>> fixed = {
        {0.0f, 1.0f}, {1.0f, 0.0f, 1.0f}, {0.25f, 0.5f, 0.125f, 0.75f, 0.0f, 1.0f, 0.375f, 0.625f}, {1.0e-20f, 2.0e-20f, 3.0e-20f},
        {1000.0f, 1000.25f, 999.75f, 1000.5f}, {0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.100000024f}};
    std::vector<std::vector<float>> seqs = fixed;
    for (int n : {2, 3, 8, 17, 128, 1000}) {
        std::vector<float> u, near;
        for (int i = 0; i < n; ++i) { u.push_back(next()); near.push_back(0.5f + next() * 1.0e-3f); }
        seqs.push_back(u); seqs.push_back(near);
    }
    for (const std::vector<float> &y : seqs) {
        long double S2 = 0.0L;
        const long double el = e_long(y, &S2);
        const double e = e_of(y);
        const long double n = (long double)y.size();
        const long double bound = 3.0L * n * ldexpl(1.0L, -53) * S2 / (n * (n - 1.0L)) + ldexpl(1.0L, -50) * el * el;
        CHECK(e >= 0.0 && fabsl((long double)e * e - el * el) <= bound);
    }
    CHECK(e_of({0.0f, 1.0f}) == 0.5);                                                           // S1 = S2 = 1: x = 0.5, v = 0.25
    std::printf("math ok\n");
}

int main() {
    refusals();
    plan();
    math();
    if (failures) { std::printf("FAILED %d checks\n", failures); return 1; }
    std::printf("all ok\n");
    return 0;
}
