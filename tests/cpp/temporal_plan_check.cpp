// Stand-alone host program over csrc/temporal_plan.hpp (tests/test_cpp_temporal_plan.py): the refusals in rtk.h's order, the
// planes and their families, the device variant's alignment, the scalars the kernel is handed and the bounds of the grid.  No HIP,
// no device.
//   usage: temporal_plan_check [WIDTH HEIGHT FOV_DEGREES ...]: for every triple, a line "scalars W H: aspect th wf hf" with the
//   four floats as hexadecimal words, for the test to compare with its own
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "temporal_plan.hpp"

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
static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }
static uint32_t word_of(float f) { uint32_t u; std::memcpy(&u, &f, sizeof(u)); return u; }

static void refusals() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(temporal_refusal(good()) == nullptr);
    // every refusal alone, in all its forms, and the ends of every range
    for (int v : {0, -1, 16385, 0x7FFFFFFF}) {
        { auto p = good(); p.width = v; CHECK(says(temporal_refusal(p), "width")); }
        { auto p = good(); p.height = v; CHECK(says(temporal_refusal(p), "height")); }
    }
    for (int v : {1, 16384}) { auto p = good(); p.width = v; p.height = v; CHECK(temporal_refusal(p) == nullptr); }
    for (double v : {0.0, -1.0, 180.0, 400.0, double(inf), double(-inf), double(nan)}) { auto p = good(); p.fov_degrees = v; CHECK(says(temporal_refusal(p), "fov_degrees")); }
    for (double v : {1e-3, 40.0, 179.0}) { auto p = good(); p.fov_degrees = v; CHECK(temporal_refusal(p) == nullptr); }
    for (float v : {0.0f, -0.0f, -1.0f, 1.0001f, inf, -inf, nan}) { auto p = good(); p.alpha_min = v; CHECK(says(temporal_refusal(p), "alpha_min")); }
    for (float v : {1e-30f, 1.0f}) { auto p = good(); p.alpha_min = v; CHECK(temporal_refusal(p) == nullptr); }
    for (float v : {0.0f, -0.0f, -1.0f, inf, -inf, nan}) { auto p = good(); p.plane_tolerance = v; CHECK(says(temporal_refusal(p), "plane_tolerance")); }
    for (float v : {-1.0001f, 1.0001f, inf, -inf, nan}) { auto p = good(); p.normal_min_dot = v; CHECK(says(temporal_refusal(p), "normal_min_dot")); }
    for (float v : {-1.0f, 0.0f, 1.0f}) { auto p = good(); p.normal_min_dot = v; CHECK(temporal_refusal(p) == nullptr); }
    for (int v : {0, -1, (1 << 20) + 1, 0x7FFFFFFF}) { auto p = good(); p.max_history = v; CHECK(says(temporal_refusal(p), "max_history")); }
    for (int v : {1, 1 << 20}) { auto p = good(); p.max_history = v; CHECK(temporal_refusal(p) == nullptr); }
    // the order: a call that is wrong in the ways k, k + 1, ... names way k
    auto p = good();
    p.max_history = 0; CHECK(says(temporal_refusal(p), "max_history"));
    p.normal_min_dot = nan; CHECK(says(temporal_refusal(p), "normal_min_dot"));
    p.plane_tolerance = 0.0f; CHECK(says(temporal_refusal(p), "plane_tolerance"));
    p.alpha_min = 2.0f; CHECK(says(temporal_refusal(p), "alpha_min"));
    p.fov_degrees = 0.0; CHECK(says(temporal_refusal(p), "fov_degrees"));
    p.height = 0; CHECK(says(temporal_refusal(p), "height"));
    p.width = 0; CHECK(says(temporal_refusal(p), "width must"));
    std::printf("refusals ok\n");
}

static void planes() {
    float x[8] = {0.0f};
    uint32_t m[8] = {0u};
    rtk_view view;
    std::memset(&view, 0, sizeof(view));
    const rtk_temporal_frame cur = {x, x, x, x, x, m};
    const rtk_temporal_history prev = {x, x, x, x, x, x, m, &view};
    const rtk_temporal_outputs out = {x, x, x};
    CHECK(temporal_missing_plane(cur, nullptr, out) == nullptr);
    CHECK(temporal_missing_plane(cur, &prev, out) == nullptr);
    for (int i = 0; i < 4; ++i) {
        rtk_temporal_frame b = cur;
        (i == 0 ? b.rgb : i == 1 ? b.position : i == 2 ? b.normal : b.depth) = nullptr;
        CHECK(says(temporal_missing_plane(b, &prev, out), "of the new frame"));
    }
    { rtk_temporal_outputs o = out; o.rgb = nullptr; CHECK(says(temporal_missing_plane(cur, &prev, o), "of the outputs")); }
    { rtk_temporal_outputs o = out; o.length = nullptr; CHECK(says(temporal_missing_plane(cur, nullptr, o), "of the outputs")); }
    for (int i = 0; i < 6; ++i) {
        rtk_temporal_history b = prev;
        if (i == 5) b.view = nullptr;
        else (i == 0 ? b.rgb : i == 1 ? b.length : i == 2 ? b.position : i == 3 ? b.normal : b.depth) = nullptr;
        CHECK(says(temporal_missing_plane(cur, &b, out), "of the history"));
    }
    // the families: every way to break the noise family, then the mesh family
    { rtk_temporal_frame c = cur; c.noise = nullptr; CHECK(says(temporal_missing_plane(c, &prev, out), "noise planes")); CHECK(says(temporal_missing_plane(c, nullptr, out), "noise planes")); }
    { rtk_temporal_outputs o = out; o.noise = nullptr; CHECK(says(temporal_missing_plane(cur, &prev, o), "noise planes")); CHECK(says(temporal_missing_plane(cur, nullptr, o), "noise planes")); }
    { rtk_temporal_history b = prev; b.noise = nullptr; CHECK(says(temporal_missing_plane(cur, &b, out), "noise planes")); }
    { rtk_temporal_frame c = cur; c.noise = nullptr; rtk_temporal_outputs o = out; o.noise = nullptr; rtk_temporal_history b = prev;
      CHECK(says(temporal_missing_plane(c, &b, o), "noise planes"));
      CHECK(temporal_missing_plane(c, nullptr, o) == nullptr);
      b.noise = nullptr; CHECK(temporal_missing_plane(c, &b, o) == nullptr); }
    { rtk_temporal_frame c = cur; c.mesh = nullptr; CHECK(says(temporal_missing_plane(c, &prev, out), "mesh planes")); CHECK(temporal_missing_plane(c, nullptr, out) == nullptr);
      rtk_temporal_history b = prev; b.mesh = nullptr; CHECK(says(temporal_missing_plane(cur, &b, out), "mesh planes")); CHECK(temporal_missing_plane(c, &b, out) == nullptr); }
    // noise before mesh; a missing plane before both
    { rtk_temporal_frame c = cur; c.noise = nullptr; c.mesh = nullptr; CHECK(says(temporal_missing_plane(c, &prev, out), "noise planes"));
      c.depth = nullptr; CHECK(says(temporal_missing_plane(c, &prev, out), "of the new frame")); }
    // the device variant's own: every plane, of every struct
    CHECK(temporal_device_refusal(cur, &prev, out) == nullptr);
    CHECK(temporal_device_refusal(cur, nullptr, out) == nullptr);
    const float *const odd = reinterpret_cast<const float *>(reinterpret_cast<const char *>(x) + 2);
    const uint32_t *const oddm = reinterpret_cast<const uint32_t *>(odd);
    for (int i = 0; i < 6; ++i) {
        rtk_temporal_frame b = cur;
        if (i == 5) b.mesh = oddm; else (i == 0 ? b.rgb : i == 1 ? b.noise : i == 2 ? b.position : i == 3 ? b.normal : b.depth) = odd;
        CHECK(says(temporal_device_refusal(b, nullptr, out), "4-byte"));
    }
    for (int i = 0; i < 7; ++i) {
        rtk_temporal_history b = prev;
        if (i == 6) b.mesh = oddm; else (i == 0 ? b.rgb : i == 1 ? b.noise : i == 2 ? b.length : i == 3 ? b.position : i == 4 ? b.normal : b.depth) = odd;
        CHECK(says(temporal_device_refusal(cur, &b, out), "4-byte"));
        CHECK(temporal_device_refusal(cur, nullptr, out) == nullptr);
    }
    for (int i = 0; i < 3; ++i) {
        rtk_temporal_outputs o = out;
        (i == 0 ? o.rgb : i == 1 ? o.noise : o.length) = const_cast<float *>(odd);
        CHECK(says(temporal_device_refusal(cur, &prev, o), "4-byte"));
    }
    std::printf("planes ok\n");
}

static void scalars(int argc, char **argv) {
    rtk_view view;
    for (int i = 0; i < 3; ++i) view.position[i] = 1.0f + float(i);
    for (int i = 0; i < 9; ++i) view.matrix[i] = 10.0f + float(i);
    auto p = good();
    volatile double fov_in = p.fov_degrees;
    p.fov_degrees = fov_in;
    const tp::Consts k = temporal_consts(p, &view);
    for (int i = 0; i < 3; ++i) CHECK(k.cam[i] == view.position[i]);
    for (int i = 0; i < 9; ++i) CHECK(k.m[i] == view.matrix[i]);
    CHECK(k.nmax == 32.0f && k.alpha_min == 0.05f && k.plane_tolerance == 0.01f && k.normal_min_dot == 0.9f);
    CHECK(k.wf == 70.0f && k.hf == 36.0f && k.aspect == 70.0f / 36.0f);
    // the one copy of the camera's expression; the angle is volatile, so that tanf is the C library's at run time on both sides
    // and not a constant the compiler folded with another rounding
    volatile double fov = 60.0;
    const CameraScalars c = camera_scalars(70u, 36u, fov);
    CHECK(word_of(k.th) == word_of(c.tan_half_fov) && word_of(k.aspect) == word_of(c.aspect));
    const float half = static_cast<float>(fov * (3.14159265358979323846 / 180.0)) / 2.0f;
    CHECK(k.th == std::tan(half));
    p.max_history = 1 << 20; CHECK(temporal_consts(p, nullptr).nmax == 1048576.0f);
    const tp::Consts none = temporal_consts(p, nullptr);
    for (int i = 0; i < 9; ++i) CHECK(none.m[i] == 0.0f);
    for (int a = 1; a + 2 < argc; a += 3) {
        auto q = good();
        q.width = std::atoi(argv[a]); q.height = std::atoi(argv[a + 1]); q.fov_degrees = std::atof(argv[a + 2]);
        CHECK(temporal_refusal(q) == nullptr);
        const tp::Consts s = temporal_consts(q, nullptr);
        std::printf("scalars %d %d: %08x %08x %08x %08x\n", q.width, q.height, word_of(s.aspect), word_of(s.th), word_of(s.wf), word_of(s.hf));
    }
    std::printf("scalars ok\n");
}

static void grid() {
    const int sizes[][2] = {{1, 1}, {5, 3}, {37, 19}, {70, 36}, {130, 70}, {16, 16}, {17, 16}, {1920, 1080}};
    for (const auto &wh : sizes) {
        auto p = good();
        p.width = wh[0]; p.height = wh[1];
        const DnTiling t = temporal_tiling(p);
        CHECK(t.n_tiles == t.tiles_per_image && t.n_tiles == uint64_t((wh[0] + 15) / 16) * uint64_t((wh[1] + 15) / 16));
        const uint32_t g = temporal_grid(t.n_tiles);
        CHECK(g >= 1u && g <= kTpMaxGrid && g <= t.n_tiles);
        // striding workgroups own every pixel exactly once, and never one outside the image
        std::vector<unsigned> seen(size_t(wh[0]) * size_t(wh[1]));
        for (uint32_t wg = 0; wg < g; ++wg)
            for (uint64_t tile = wg; tile < t.n_tiles; tile += g) {
                const DnTile T = denoise_tile(t, tile);
                CHECK(T.image == 0u && T.w >= 1u && T.h >= 1u && T.w <= kDnTile && T.h <= kDnTile);
                CHECK(T.x0 + T.w <= uint32_t(wh[0]) && T.y0 + T.h <= uint32_t(wh[1]));
                for (uint32_t y = T.y0; y < T.y0 + T.h; ++y)
                    for (uint32_t x = T.x0; x < T.x0 + T.w; ++x) seen[size_t(y) * size_t(wh[0]) + x] += 1;
            }
        for (unsigned s : seen) if (s != 1u) { CHECK(s == 1u); break; }
    }
    // the largest frame: 2^20 tiles, a bounded grid, and pixel and word indices that fit 32 bits
    auto p = good();
    p.width = kTpMaxSide; p.height = kTpMaxSide;
    const DnTiling t = temporal_tiling(p);
    CHECK(t.n_tiles == (uint64_t(1) << 20) && temporal_grid(t.n_tiles) == kTpMaxGrid);
    const DnTile last = denoise_tile(t, t.n_tiles - 1);
    CHECK(last.x0 + last.w == uint32_t(kTpMaxSide) && last.y0 + last.h == uint32_t(kTpMaxSide));
    CHECK(uint64_t(kTpMaxSide) * kTpMaxSide * 3u < (uint64_t(1) << 32));
    CHECK(temporal_grid(0) == 0u && temporal_grid(1) == 1u && temporal_grid(kTpMaxGrid + 1u) == kTpMaxGrid);
    CHECK(kTpThreads == 256u);
    std::printf("grid ok\n");
}

int main(int argc, char **argv) {
    refusals();
    planes();
    scalars(argc, argv);
    grid();
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("all ok\n");
    return 0;
}
