// Stand-alone host program over csrc/denoise_plan.hpp (tests/test_cpp_denoise_plan.py): the refusals in rtk.h's order, tiles that
// cover every pixel of every image exactly once, halo and LDS sizes per step, the staged / direct decision under the knob, and the
// workspace.  No HIP, no device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "denoise_plan.hpp"

using namespace rtk;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static rtk_denoise_params good() {
    rtk_denoise_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = 70; p.height = 36; p.iterations = 5; p.normal_power_log2 = 2;
    p.sigma_luminance = 1.5f; p.sigma_plane = 0.05f; p.albedo_floor = 0.01f;
    return p;
}
static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }

static void refusals() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(denoise_refusal(good(), 1) == nullptr);
    CHECK(denoise_refusal(good(), 0) == nullptr);
    // every refusal alone, in all its forms
    { auto p = good(); p.width = 0; CHECK(says(denoise_refusal(p, 1), "width and height")); p.width = -3; CHECK(says(denoise_refusal(p, 1), "width and height")); }
    { auto p = good(); p.height = 0; CHECK(says(denoise_refusal(p, 1), "width and height")); }
    { auto p = good(); p.width = 1 << 14; p.height = (1 << 14) + 1; CHECK(says(denoise_refusal(p, 1), "per image"));
      p.height = 1 << 14; CHECK(denoise_refusal(p, 1) == nullptr);
      p.width = 0x7FFFFFFF; p.height = 0x7FFFFFFF; CHECK(says(denoise_refusal(p, 1), "per image")); }
    for (int it : {0, -1, 9}) { auto p = good(); p.iterations = it; CHECK(says(denoise_refusal(p, 1), "iterations")); }
    for (int it : {1, 8}) { auto p = good(); p.iterations = it; CHECK(denoise_refusal(p, 1) == nullptr); }
    for (int np : {-1, 9}) { auto p = good(); p.normal_power_log2 = np; CHECK(says(denoise_refusal(p, 1), "normal_power_log2")); }
    for (int np : {0, 8}) { auto p = good(); p.normal_power_log2 = np; CHECK(denoise_refusal(p, 1) == nullptr); }
    for (float bad : {0.0f, -0.0f, -1.0f, inf, -inf, nan}) {
        { auto p = good(); p.sigma_luminance = bad; CHECK(says(denoise_refusal(p, 1), "sigma_luminance")); }
        { auto p = good(); p.sigma_plane = bad; CHECK(says(denoise_refusal(p, 1), "sigma_plane")); }
        { auto p = good(); p.albedo_floor = bad; CHECK(says(denoise_refusal(p, 1), "albedo_floor")); }
    }
    CHECK(says(denoise_refusal(good(), -1), "n_images"));
    { auto p = good(); p.width = 1 << 14; p.height = 1 << 14; CHECK(denoise_refusal(p, 8) == nullptr); CHECK(says(denoise_refusal(p, 9), "in total"));
      CHECK(says(denoise_refusal(p, 0x7FFFFFFF), "in total")); }
    { auto p = good(); p.width = 1; p.height = 1; CHECK(denoise_refusal(p, 0x7FFFFFFF) == nullptr); }
    // the order: a call that is wrong in the ways k, k + 1, ... names way k
    const char *const order[] = {"in total", "n_images", "albedo_floor", "sigma_plane", "sigma_luminance", "normal_power_log2", "iterations", "per image"};
    auto p = good();
    p.width = 1 << 14; p.height = 1 << 14;
    int32_t n = 9;
    CHECK(says(denoise_refusal(p, n), order[0]));
    n = -1; CHECK(says(denoise_refusal(p, n), order[1]));
    p.albedo_floor = 0.0f; CHECK(says(denoise_refusal(p, n), order[2]));
    p.sigma_plane = nan; CHECK(says(denoise_refusal(p, n), order[3]));
    p.sigma_luminance = -1.0f; CHECK(says(denoise_refusal(p, n), order[4]));
    p.normal_power_log2 = 9; CHECK(says(denoise_refusal(p, n), order[5]));
    p.iterations = 0; CHECK(says(denoise_refusal(p, n), order[6]));
    p.height = (1 << 14) + 1; CHECK(says(denoise_refusal(p, n), order[7]));
    p.width = 0; CHECK(says(denoise_refusal(p, n), "width and height"));
    // planes, then the device variant's own
    float x[8] = {0.0f};
    alignas(16) char ws[64] = {0};
    rtk_denoise_inputs in = {x, nullptr, nullptr, x, x, x};
    CHECK(denoise_missing_plane(in, x) == nullptr);
    CHECK(denoise_missing_plane(in, nullptr) != nullptr);
    for (int i = 0; i < 4; ++i) {
        rtk_denoise_inputs b = in;
        (i == 0 ? b.rgb : i == 1 ? b.normal : i == 2 ? b.position : b.depth) = nullptr;
        CHECK(denoise_missing_plane(b, x) != nullptr);
    }
    CHECK(denoise_device_refusal(in, x, ws, 64, 64) == nullptr);
    const float *const odd = reinterpret_cast<const float *>(reinterpret_cast<const char *>(x) + 2);
    for (int i = 0; i < 6; ++i) {
        rtk_denoise_inputs b = in;
        (i == 0 ? b.rgb : i == 1 ? b.noise : i == 2 ? b.albedo : i == 3 ? b.normal : i == 4 ? b.position : b.depth) = odd;
        CHECK(says(denoise_device_refusal(b, x, nullptr, 0, 64), "4-byte"));           // (before the workspace's)
    }
    CHECK(says(denoise_device_refusal(in, odd, nullptr, 0, 64), "4-byte"));
    CHECK(says(denoise_device_refusal(in, x, nullptr, 0, 64), "null workspace"));
    CHECK(says(denoise_device_refusal(in, x, ws + 4, 0, 64), "16-byte"));
    CHECK(says(denoise_device_refusal(in, x, ws, 63, 64), "smaller"));
    std::printf("refusals ok\n");
}

static void tiles_of(uint32_t w, uint32_t h, uint32_t n) {
    const DnTiling t = denoise_tiling(w, h, n);
    CHECK(t.tiles_x == (w + 15) / 16 && t.tiles_y == (h + 15) / 16 && t.n_tiles == uint64_t(t.tiles_x) * t.tiles_y * n);
    std::vector<unsigned char> seen(size_t(w) * h * n, 0);
    for (uint64_t i = 0; i < t.n_tiles; ++i) {
        const DnTile T = denoise_tile(t, i);
        CHECK(T.image < n && T.w >= 1 && T.w <= kDnTile && T.h >= 1 && T.h <= kDnTile && T.x0 % kDnTile == 0 && T.y0 % kDnTile == 0);
        CHECK(T.x0 + T.w <= w && T.y0 + T.h <= h);                                       // inside ONE image
        CHECK((T.w == kDnTile || T.x0 + T.w == w) && (T.h == kDnTile || T.y0 + T.h == h));
        for (uint32_t y = T.y0; y < T.y0 + T.h; ++y)
            for (uint32_t x = T.x0; x < T.x0 + T.w; ++x) seen[(size_t(T.image) * h + y) * w + x] += 1;
    }
    bool once = true;
    for (unsigned char s : seen) once = once && s == 1;
    CHECK(once);
}

static void tiles() {
    tiles_of(37, 19, 1); tiles_of(5, 3, 1); tiles_of(1, 1, 1); tiles_of(70, 36, 2); tiles_of(130, 70, 3); tiles_of(16, 16, 2);
    tiles_of(17, 33, 5); tiles_of(1, 1, 1000);
    // the largest shapes: the numbers stay in range
    DnTiling t = denoise_tiling(1u << 14, 1u << 14, 8);
    CHECK(t.n_tiles == uint64_t(1) << 23);
    DnTile T = denoise_tile(t, t.n_tiles - 1);
    CHECK(T.image == 7 && T.x0 == (1u << 14) - 16 && T.y0 == (1u << 14) - 16 && T.w == 16 && T.h == 16);
    t = denoise_tiling(1, 1, 1u << 31);
    CHECK(t.n_tiles == uint64_t(1) << 31);
    T = denoise_tile(t, t.n_tiles - 1);
    CHECK(T.image == (1u << 31) - 1 && T.x0 == 0 && T.y0 == 0 && T.w == 1 && T.h == 1);
    t = denoise_tiling(1, 1u << 28, 8);
    CHECK(t.tiles_per_image == uint64_t(1) << 24);
    T = denoise_tile(t, t.n_tiles - 1);
    CHECK(T.image == 7 && T.y0 == (1u << 28) - 16 && T.h == 16 && T.w == 1);
    CHECK(denoise_grid(0) == 0 && denoise_grid(5) == 5 && denoise_grid(uint64_t(1) << 31) == kDnMaxGrid);
    std::printf("tiles ok\n");
}

static void steps() {
    const uint32_t side[8] = {20, 24, 32, 48, 80, 144, 272, 528}, pitch[8] = {32, 32, 32, 48, 80, 144, 272, 528};
    for (int k = 0; k < kDnMaxIterations; ++k) {
        const uint32_t s = denoise_step(k);
        CHECK(s == 1u << k && denoise_halo(s) == 2 * s && denoise_lds_side(s) == side[k] && denoise_lds_pitch(s) == pitch[k]);
        CHECK(denoise_lds_pitch(s) % 16 == 0 && denoise_lds_pitch(s) >= denoise_lds_side(s) && denoise_lds_pitch(s) < denoise_lds_side(s) + 16);
        CHECK(denoise_lds_bytes(s) == pitch[k] * side[k] * 48u);
        // the farthest tap of the tile's last thread lies inside the halo'd tile
        CHECK(15u + denoise_halo(s) + 2u * s < denoise_lds_side(s));
    }
    CHECK(denoise_lds_bytes(1) == 30720 && denoise_lds_bytes(2) == 36864 && denoise_lds_bytes(4) == 49152 && denoise_lds_bytes(8) == 110592);
    CHECK(denoise_lds_bytes(uint32_t(kDnLdsStepLimit)) <= kDnLdsPerCu && denoise_lds_bytes(2u * kDnLdsStepLimit) > kDnLdsPerCu);
    std::printf("steps ok\n");
}

static void knob() {
    CHECK(denoise_lds_max_step(nullptr) == kDnLdsMaxStepDefault && denoise_lds_max_step("") == kDnLdsMaxStepDefault);
    CHECK(denoise_lds_max_step("0") == 0 && denoise_lds_max_step("1") == 1 && denoise_lds_max_step("4") == 4 && denoise_lds_max_step("8") == 8);
    CHECK(denoise_lds_max_step("9") == kDnLdsMaxStepDefault && denoise_lds_max_step("-1") == kDnLdsMaxStepDefault);
    CHECK(denoise_lds_max_step("x") == kDnLdsMaxStepDefault && denoise_lds_max_step("4x") == kDnLdsMaxStepDefault);
    CHECK(kDnLdsMaxStepDefault >= 0 && kDnLdsMaxStepDefault <= kDnLdsStepLimit);
    for (int k = 0; k < kDnMaxIterations; ++k) {
        const uint32_t s = denoise_step(k);
        CHECK(!denoise_staged(s, 0));                                  // 0 = never
        for (int m : {1, 2, 3, 4, 8}) CHECK(denoise_staged(s, m) == (s <= uint32_t(m)));
        CHECK(denoise_staged(s, 1000) == (s <= uint32_t(kDnLdsStepLimit)));          // whatever the knob: never a tile that does not fit
        if (denoise_staged(s, 1000)) CHECK(denoise_lds_bytes(s) <= kDnLdsPerCu);
    }
    std::printf("knob ok\n");
}

static void workspace() {
    for (int it = 1; it <= kDnMaxIterations; ++it)
        for (uint64_t px : {uint64_t(1), uint64_t(15), uint64_t(2520), uint64_t(1) << 28, uint64_t(1) << 31}) {
            const DnWorkspace w = denoise_workspace(px, it);
            CHECK(w.bytes <= 64u * px && w.bytes == (it > 1 ? 64u : 48u) * px);
            CHECK(w.g0 == 0 && w.g1 == 16u * px && w.c[0] == 32u * px && w.c[1] == (it > 1 ? 48u * px : w.c[0]));
            CHECK(w.g0 % 16 == 0 && w.g1 % 16 == 0 && w.c[0] % 16 == 0 && w.c[1] % 16 == 0);
            CHECK(w.c[1] + 16u * px <= w.bytes);
        }
    CHECK(denoise_workspace(uint64_t(1) << 31, 5).bytes == uint64_t(1) << 37);           // 64-bit safe
    CHECK(denoise_workspace(0, 5).bytes == 0);
    // an iteration reads one signal buffer and writes the other
    for (int k = 0; k < kDnMaxIterations; ++k) CHECK(denoise_source(k) == (k & 1));
    std::printf("workspace ok\n");
}

int main() {
    refusals();
    tiles();
    steps();
    knob();
    workspace();
    if (failures) { std::printf("FAILED %d checks\n", failures); return 1; }
    std::printf("all ok\n");
    return 0;
}
