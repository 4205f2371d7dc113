// Stand-alone host program over csrc/motion_plan.hpp (tests/test_cpp_motion_plan.py): the refusals in rtk.h's order with the ends of
// every range, the device variant's alignment, the scalars the kernel is handed, the stage of the host variant and the bounds of
// the grid.  No HIP, no device.
//   usage: motion_plan_check [WIDTH HEIGHT FOV_DEGREES ...]: for every triple, a line "scalars W H: aspect th wf hf" with the four
//   floats as hexadecimal words, for the test to compare with its own
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "motion_plan.hpp"
#include "stage_plan.hpp"

using namespace rtk;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static rtk_motion_params good() {
    rtk_motion_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = 70; p.height = 36; p.fov_degrees = 60.0;
    return p;
}
static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }
static uint32_t word_of(float f) { uint32_t u; std::memcpy(&u, &f, sizeof(u)); return u; }

static void refusals() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int accel = 0;                                   // (any address: the plan never looks behind it)
    uint32_t tri[4] = {0u};
    float x[8] = {0.0f};
    rtk_view view;
    std::memset(&view, 0, sizeof(view));
    const rtk_motion_outputs both = {x, x}, position = {x, nullptr}, motion = {nullptr, x}, none = {nullptr, nullptr};
    auto p = good();
    CHECK(motion_refusal(&accel, &p, tri, x, x, &view, &both) == nullptr);
    CHECK(motion_refusal(&accel, &p, tri, x, x, nullptr, &position) == nullptr);
    CHECK(motion_refusal(&accel, &p, tri, x, x, &view, &position) == nullptr);
    CHECK(motion_refusal(&accel, &p, tri, x, x, &view, &motion) == nullptr);
    // every NULL alone, whatever else is wrong
    auto bad = good();
    bad.width = 0;
    CHECK(says(motion_refusal(nullptr, &bad, tri, x, x, nullptr, &none), "null accel"));
    CHECK(says(motion_refusal(&accel, nullptr, tri, x, x, nullptr, &none), "null accel"));
    CHECK(says(motion_refusal(&accel, &bad, nullptr, x, x, nullptr, &none), "null accel"));
    CHECK(says(motion_refusal(&accel, &bad, tri, nullptr, x, nullptr, &none), "null accel"));
    CHECK(says(motion_refusal(&accel, &bad, tri, x, nullptr, nullptr, &none), "null accel"));
    CHECK(says(motion_refusal(&accel, &bad, tri, x, x, nullptr, nullptr), "null accel"));
    // the ends of every range
    for (int v : {0, -1, 16385, 0x7FFFFFFF, int(0x80000000u)}) {
        { auto q = good(); q.width = v; CHECK(says(motion_refusal(&accel, &q, tri, x, x, &view, &both), "width must")); }
        { auto q = good(); q.height = v; CHECK(says(motion_refusal(&accel, &q, tri, x, x, &view, &both), "height must")); }
    }
    for (int v : {1, 16384}) { auto q = good(); q.width = v; q.height = v; CHECK(motion_refusal(&accel, &q, tri, x, x, &view, &both) == nullptr); }
    for (double v : {0.0, -0.0, -1.0, 180.0, 400.0, inf, -inf, nan}) { auto q = good(); q.fov_degrees = v; CHECK(says(motion_refusal(&accel, &q, tri, x, x, &view, &both), "fov_degrees")); }
    for (double v : {1e-3, 40.0, 90.0, 179.999}) { auto q = good(); q.fov_degrees = v; CHECK(motion_refusal(&accel, &q, tri, x, x, &view, &both) == nullptr); }
    CHECK(says(motion_refusal(&accel, &p, tri, x, x, &view, &none), "both null"));
    CHECK(says(motion_refusal(&accel, &p, tri, x, x, nullptr, &motion), "needs prev_view"));
    CHECK(says(motion_refusal(&accel, &p, tri, x, x, nullptr, &both), "needs prev_view"));
    // the order: a call that is wrong in the ways k, k + 1, ... names way k
    auto q = good();
    CHECK(says(motion_refusal(&accel, &q, tri, x, x, nullptr, &motion), "needs prev_view"));
    CHECK(says(motion_refusal(&accel, &q, tri, x, x, nullptr, &none), "both null"));
    q.fov_degrees = nan; CHECK(says(motion_refusal(&accel, &q, tri, x, x, nullptr, &none), "fov_degrees"));
    q.height = 0; CHECK(says(motion_refusal(&accel, &q, tri, x, x, nullptr, &none), "height must"));
    q.width = 16385; CHECK(says(motion_refusal(&accel, &q, tri, x, x, nullptr, &none), "width must"));
    CHECK(says(motion_refusal(&accel, &q, tri, x, nullptr, nullptr, &none), "null accel"));
    std::printf("refusals ok\n");
}

static void alignment() {
    uint32_t tri[4] = {0u};
    float x[8] = {0.0f};
    const rtk_motion_outputs both = {x, x};
    CHECK(motion_device_refusal(tri, x, x, both) == nullptr);
    CHECK(motion_device_refusal(tri, x, x, rtk_motion_outputs{x, nullptr}) == nullptr);
    CHECK(motion_device_refusal(tri, x, x, rtk_motion_outputs{nullptr, x}) == nullptr);
    for (int by = 1; by < 4; ++by) {
        float *const odd = reinterpret_cast<float *>(reinterpret_cast<char *>(x) + by);
        const uint32_t *const oddt = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(tri) + by);
        CHECK(says(motion_device_refusal(oddt, x, x, both), "4-byte"));
        CHECK(says(motion_device_refusal(tri, odd, x, both), "4-byte"));
        CHECK(says(motion_device_refusal(tri, x, odd, both), "4-byte"));
        CHECK(says(motion_device_refusal(tri, x, x, rtk_motion_outputs{odd, x}), "4-byte"));
        CHECK(says(motion_device_refusal(tri, x, x, rtk_motion_outputs{x, odd}), "4-byte"));
        CHECK(says(motion_device_refusal(tri, x, x, rtk_motion_outputs{nullptr, odd}), "4-byte"));
    }
    std::printf("alignment ok\n");
}

static void scalars(int argc, char **argv) {
    rtk_view view;
    for (int i = 0; i < 3; ++i) view.position[i] = 1.0f + float(i);
    for (int i = 0; i < 9; ++i) view.matrix[i] = 10.0f + float(i);
    auto p = good();
    volatile double fov_in = p.fov_degrees;
    p.fov_degrees = fov_in;
    const tp::Consts k = motion_consts(p, &view);
    for (int i = 0; i < 3; ++i) CHECK(k.cam[i] == view.position[i]);
    for (int i = 0; i < 9; ++i) CHECK(k.m[i] == view.matrix[i]);
    CHECK(k.wf == 70.0f && k.hf == 36.0f && k.aspect == 70.0f / 36.0f);
    CHECK(k.nmax == 0.0f && k.alpha_min == 0.0f && k.plane_tolerance == 0.0f && k.normal_min_dot == 0.0f);
    // the one copy of the camera's expression; the angle is volatile, so that tanf is the C library's at run time on both sides
    volatile double fov = 60.0;
    const CameraScalars c = camera_scalars(70u, 36u, fov);
    CHECK(word_of(k.th) == word_of(c.tan_half_fov) && word_of(k.aspect) == word_of(c.aspect));
    const tp::Consts none = motion_consts(p, nullptr);
    for (int i = 0; i < 9; ++i) CHECK(none.m[i] == 0.0f);
    CHECK(word_of(none.th) == word_of(k.th));
    for (int a = 1; a + 2 < argc; a += 3) {
        auto q = good();
        q.width = std::atoi(argv[a]); q.height = std::atoi(argv[a + 1]); q.fov_degrees = std::atof(argv[a + 2]);
        const tp::Consts s = motion_consts(q, nullptr);
        std::printf("scalars %d %d: %08x %08x %08x %08x\n", q.width, q.height, word_of(s.aspect), word_of(s.th), word_of(s.wf), word_of(s.hf));
    }
    std::printf("scalars ok\n");
}

static void stage() {
    // the planes of the host variant in the order of kMvStage*: sizes, absent outputs, and the largest call
    const uint64_t sides[][3] = {{1, 1, 0}, {7, 5, 3}, {130, 70, 2012}, {16384, 16384, 0xFFFFFFF0ull}};
    for (const auto &s : sides) {
        const uint64_t n = s[0] * s[1], nv = s[2];
        CHECK(motion_stage_words(kMvStageTri, n, nv) == n && motion_stage_words(kMvStageBary, n, nv) == 2 * n);
        CHECK(motion_stage_words(kMvStageVerts, n, nv) == 3 * nv);
        CHECK(motion_stage_words(kMvStagePrevPosition, n, nv) == 3 * n && motion_stage_words(kMvStageMotion, n, nv) == 2 * n);
        for (int want = 1; want < 4; ++want) {
            StageLayout L;
            for (int i = 0; i < kMvStagePlanes; ++i)
                L.add(motion_stage_words(i, n, nv), i < kMvStagePrevPosition || (want >> (i - kMvStagePrevPosition) & 1) != 0);
            CHECK(L.n == kMvStagePlanes && L.fits());
            CHECK(L.present(kMvStageTri) && L.present(kMvStageBary) && L.present(kMvStageVerts));
            CHECK(L.present(kMvStagePrevPosition) == ((want & 1) != 0) && L.present(kMvStageMotion) == ((want & 2) != 0));
            uint64_t end = 0;
            for (int i = 0; i < kMvStagePlanes; ++i) {
                if (!L.present(i)) continue;
                CHECK(L.off[i] >= end && L.off[i] % kStageAlignWords == 0 && L.bytes[i] == 4 * motion_stage_words(i, n, nv));
                end = L.off[i] + motion_stage_words(i, n, nv);
            }
            CHECK(L.total >= end);
        }
    }
    CHECK(kMvStagePlanes == 5 && kMvStagePlanes <= kStageMaxPlanes);
    std::printf("stage ok\n");
}

static void grid() {
    const int sizes[][2] = {{1, 1}, {7, 5}, {37, 19}, {64, 64}, {130, 70}, {16, 16}, {17, 16}, {1920, 1080}};
    for (const auto &wh : sizes) {
        auto p = good();
        p.width = wh[0]; p.height = wh[1];
        const DnTiling t = motion_tiling(p);
        CHECK(t.n_tiles == t.tiles_per_image && t.n_tiles == uint64_t((wh[0] + 15) / 16) * uint64_t((wh[1] + 15) / 16));
        const uint32_t g = motion_grid(t.n_tiles);
        CHECK(g >= 1u && g <= kMvMaxGrid && g <= t.n_tiles);
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
    // the largest frame: 2^20 tiles, a bounded grid; the first and last tile of the last stride lie inside
    auto p = good();
    p.width = kMvMaxSide; p.height = kMvMaxSide;
    const DnTiling t = motion_tiling(p);
    CHECK(t.n_tiles == (uint64_t(1) << 20) && motion_grid(t.n_tiles) == kMvMaxGrid);
    const DnTile last = denoise_tile(t, t.n_tiles - 1);
    CHECK(last.x0 + last.w == uint32_t(kMvMaxSide) && last.y0 + last.h == uint32_t(kMvMaxSide));
    CHECK(uint64_t(kMvMaxSide) * kMvMaxSide * 3u < (uint64_t(1) << 32));
    CHECK(motion_grid(0) == 0u && motion_grid(1) == 1u && motion_grid(kMvMaxGrid) == kMvMaxGrid && motion_grid(kMvMaxGrid + 1u) == kMvMaxGrid);
    CHECK(kMvThreads == 256u);
    std::printf("grid ok\n");
}

int main(int argc, char **argv) {
    refusals();
    alignment();
    scalars(argc, argv);
    stage();
    grid();
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("all ok\n");
    return 0;
}
