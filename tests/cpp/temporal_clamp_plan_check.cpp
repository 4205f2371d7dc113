// Stand-alone host program over csrc/temporal_clamp_plan.hpp (tests/test_cpp_temporal_clamp_plan.py): the refusals of
// rtk_temporal_accumulate_clamped in rtk.h's order with the ends of the three new ranges, the two aliasing refusals, and the LDS a
// workgroup stages its tile in.  No HIP, no device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "temporal_clamp_plan.hpp"

using namespace rtk;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static rtk_temporal_params good() {
    rtk_temporal_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = 70; p.height = 36; p.fov_degrees = 60.0;
    p.alpha_min = 0.05f; p.plane_tolerance = 0.01f; p.normal_min_dot = 0.9f; p.max_history = 32;
    return p;
}
static rtk_temporal_clamp clamp(int32_t radius, float gamma, float keep) {
    rtk_temporal_clamp k;
    k.radius = radius; k.gamma = gamma; k.history_keep = keep; k.reserved = 0x5A5A5A5A;          // (ignored)
    return k;
}
static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }

static void ranges() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    static_assert(sizeof(rtk_temporal_clamp) == 16, "rtk.h says 16 bytes");
    CHECK(temporal_clamp_refusal(clamp(1, 1.0f, 1.0f)) == nullptr);
    for (int v : {0, -1, 4, 0x7FFFFFFF, int(0x80000000u)}) CHECK(says(temporal_clamp_refusal(clamp(v, 1.0f, 1.0f)), "radius"));
    for (int v : {1, 2, 3}) CHECK(temporal_clamp_refusal(clamp(v, 1.0f, 1.0f)) == nullptr);
    for (float v : {-1e-30f, -1.0f, inf, -inf, nan}) CHECK(says(temporal_clamp_refusal(clamp(1, v, 1.0f)), "gamma"));
    for (float v : {0.0f, -0.0f, 1e-30f, 1e30f, std::numeric_limits<float>::max()}) CHECK(temporal_clamp_refusal(clamp(1, v, 1.0f)) == nullptr);
    for (float v : {-1e-30f, 1.0001f, 2.0f, inf, -inf, nan}) CHECK(says(temporal_clamp_refusal(clamp(1, 1.0f, v)), "history_keep"));
    for (float v : {0.0f, -0.0f, 0.5f, 1.0f}) CHECK(temporal_clamp_refusal(clamp(1, 1.0f, v)) == nullptr);
    // the struct's order
    CHECK(says(temporal_clamp_refusal(clamp(1, 1.0f, nan)), "history_keep"));
    CHECK(says(temporal_clamp_refusal(clamp(1, nan, nan)), "gamma"));
    CHECK(says(temporal_clamp_refusal(clamp(0, nan, nan)), "radius"));
    std::printf("ranges ok\n");
}

static void order_and_aliasing() {
    float x[8] = {0.0f}, y[8] = {0.0f}, z[8] = {0.0f};
    uint32_t m[8] = {0u};
    rtk_view view;
    std::memset(&view, 0, sizeof(view));
    const rtk_temporal_frame cur = {x, x + 4, x, x, x, m};
    const rtk_temporal_history prev = {x, x, x, x, x, x, m, &view};
    const rtk_temporal_outputs out = {y, z, y};
    const rtk_temporal_clamp k = clamp(2, 1.5f, 0.5f);
    for (bool device : {false, true}) {
        CHECK(temporal_clamped_refusal(good(), k, cur, &prev, out, device) == nullptr);
        CHECK(temporal_clamped_refusal(good(), k, cur, nullptr, out, device) == nullptr);
    }
    // the aliasing refusals, rgb before noise; a NULL noise family aliases nothing
    { rtk_temporal_outputs o = out; o.rgb = const_cast<float *>(cur.rgb); CHECK(says(temporal_clamp_alias(cur, o), "out->rgb"));
      o.noise = const_cast<float *>(cur.noise); CHECK(says(temporal_clamp_alias(cur, o), "out->rgb"));
      o.rgb = y; CHECK(says(temporal_clamp_alias(cur, o), "out->noise")); }
    { rtk_temporal_frame c = cur; c.noise = nullptr; rtk_temporal_outputs o = out; o.noise = nullptr; CHECK(temporal_clamp_alias(c, o) == nullptr);
      CHECK(temporal_clamped_refusal(good(), k, c, nullptr, o, true) == nullptr); }
    CHECK(temporal_clamp_alias(cur, out) == nullptr);
    // the plain call allows what the clamped one refuses
    { rtk_temporal_outputs o = out; o.rgb = const_cast<float *>(cur.rgb); o.noise = const_cast<float *>(cur.noise);
      CHECK(temporal_missing_plane(cur, &prev, o) == nullptr && temporal_device_refusal(cur, &prev, o) == nullptr); }
    // the order: a call that is wrong in the ways k, k + 1, ... names way k.  Last to first: alignment, noise alias, rgb alias, the
    // mesh family, the noise family, a missing plane, history_keep, gamma, radius, the parameters
    const float nan = std::numeric_limits<float>::quiet_NaN();
    rtk_temporal_params p = good();
    rtk_temporal_clamp kk = k;
    rtk_temporal_frame c = cur;
    rtk_temporal_history h = prev;
    rtk_temporal_outputs o = out;
    c.position = reinterpret_cast<const float *>(reinterpret_cast<const char *>(x) + 2);
    CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "4-byte"));
    CHECK(temporal_clamped_refusal(p, kk, c, &h, o, false) == nullptr);                         // (the host variant has no such check)
    o.noise = const_cast<float *>(c.noise); CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "out->noise"));
    o.rgb = const_cast<float *>(c.rgb); CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "out->rgb"));
    h.mesh = nullptr; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "mesh planes"));
    h.noise = nullptr; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "noise planes"));
    h.view = nullptr; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "of the history"));
    o.length = nullptr; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "of the outputs"));
    c.depth = nullptr; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "of the new frame"));
    kk.history_keep = 1.5f; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "history_keep"));
    kk.gamma = nan; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "gamma"));
    kk.radius = 4; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "radius"));
    p.max_history = 0; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, true), "max_history"));
    p.width = 0; CHECK(says(temporal_clamped_refusal(p, kk, c, &h, o, false), "width must"));
    std::printf("order ok\n");
}

static void lds() {
    CHECK(temporal_clamp_side(1) == 18u && temporal_clamp_side(2) == 20u && temporal_clamp_side(3) == 22u);
    CHECK(temporal_clamp_lds_pixels(1) == 324u && temporal_clamp_lds_pixels(2) == 400u && temporal_clamp_lds_pixels(3) == 484u);
    CHECK(temporal_clamp_lds_bytes(1) == 6480u && temporal_clamp_lds_bytes(2) == 8000u && temporal_clamp_lds_bytes(3) == 9680u);
    for (int r = kTcMinRadius; r <= kTcMaxRadius; ++r) {
        std::printf("lds %d: %u pixels, %u bytes\n", r, temporal_clamp_lds_pixels(r), temporal_clamp_lds_bytes(r));
        // two staging passes of the 256 threads cover the square; seven workgroups per CU fit the LDS many times over
        CHECK(temporal_clamp_lds_pixels(r) <= 2u * kTpThreads);
        CHECK(7u * temporal_clamp_lds_bytes(r) <= kDnLdsPerCu);
        // the farthest tap of the tile's corner pixels lies inside the staged square
        const int side = int(temporal_clamp_side(r));
        CHECK(int(kDnTile) - 1 + 2 * r == side - 1);
    }
    std::printf("lds ok\n");
}

int main() {
    ranges();
    order_and_aliasing();
    lds();
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("all ok\n");
    return 0;
}
