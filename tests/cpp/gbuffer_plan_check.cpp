// gbuffer_plan.hpp on the host: the plan of rtk_render_gbuffer (tests/test_cpp_gbuffer_plan.py).  Pins worked out by hand: the plane
// masks, the refusals in rtk.h's order, blocks per view and workgroups for 1x1, 8x8, 9x7, 70x45 and unit counts that are no
// multiple of four, element counts of the planes, the grids, and the cut into launches of whole views -- at a lowered limit and at
// the real one for 70,000 views of 3840x2160, a size no GPU test reaches.  Plain g++, no HIP.  Prints "masks ok", "refusals ok",
// "units ok", "elements ok", "grids ok", "launches ok", "large ok", "all ok"; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gbuffer_plan.hpp"

using namespace rtk;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s (line %d): ", #cond, __LINE__);           \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
            if (++g_failed > 20) std::exit(1);                               \
        }                                                                    \
    } while (0)

bool has(const char *why, const char *word) { return why != nullptr && std::strstr(why, word) != nullptr; }

void masks() {
    static_assert(sizeof(rtk_gbuffer) == 64, "eight pointers");
    float f[4];
    uint32_t u[4];
    rtk_gbuffer o;
    std::memset(&o, 0, sizeof(o));
    CHECK(gbuffer_mask(o) == 0u, "empty");
    o.depth = f;
    CHECK(gbuffer_mask(o) == kGbDepth, "depth %u", gbuffer_mask(o));
    o.material = u;
    CHECK(gbuffer_mask(o) == (kGbDepth | kGbMaterial), "depth + material %u", gbuffer_mask(o));
    o.position = o.normal = o.albedo = o.bary = f; o.tri = o.mesh = u;
    CHECK(gbuffer_mask(o) == kGbAllPlanes, "all %u", gbuffer_mask(o));
    uint32_t bytes = 0;
    for (int i = 0; i < kGbPlanes; ++i) bytes += 4u * kGbComps[i];
    CHECK(bytes == 60u, "bytes per pixel %u", bytes);
    CHECK(gbuffer_plane(o, 1) == f && gbuffer_plane(o, 5) == u && gbuffer_plane(o, 7) == u, "plane pointers by index");
    if (g_failed == 0) std::printf("masks ok\n");
}

rtk_render_params params(int spp, int world, int stats) {
    rtk_render_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = 8; p.height = 8; p.spp = spp; p.world_size = world; p.collect_stats = stats;
    return p;
}

void refusals() {
    const int before = g_failed;
    const rtk_render_params ok = params(4, 1, 0);
    CHECK(gbuffer_refusal(ok, 0, false, 2, kGbDepth, 8, 8) == nullptr && gbuffer_refusal(ok, 3, true, 1, kGbMesh, 8, 8) == nullptr, "valid calls");
    CHECK(gbuffer_refusal(ok, 0, false, 0, kGbDepth, 8, 8) == nullptr, "n_views == 0 with views is no refusal");
    // each refusal wins over everything behind it in the list
    CHECK(has(gbuffer_refusal(params(4, 2, 1), 4, true, -1, 0u, 8, 8), "sample"), "sample first");
    CHECK(has(gbuffer_refusal(params(4, 2, 1), -1, true, -1, 0u, 8, 8), "sample"), "negative sample");
    CHECK(has(gbuffer_refusal(params(4, 2, 1), 0, true, -1, 0u, 8, 8), "sharded"), "world_size");
    CHECK(has(gbuffer_refusal(params(4, 1, 1), 0, true, -1, 0u, 8, 8), "statistics"), "collect_stats");
    CHECK(has(gbuffer_refusal(ok, 0, true, -1, 0u, 8, 8), "n_views must be >= 0"), "negative n_views");
    CHECK(has(gbuffer_refusal(ok, 0, true, 0, 0u, 8, 8), "n_views must be 1"), "null views, n_views 0");
    CHECK(has(gbuffer_refusal(ok, 0, true, 2, 0u, 8, 8), "n_views must be 1"), "null views, n_views 2");
    CHECK(has(gbuffer_refusal(ok, 0, true, 1, 0u, 8, 8), "no plane"), "no plane, accel camera");
    CHECK(has(gbuffer_refusal(ok, 0, false, 0, 0u, 8, 8), "no plane"), "no plane comes before n_views == 0");
    CHECK(has(gbuffer_refusal(ok, 0, false, 0x7FFFFFFF, kGbDepth, 65536, 65536), "too many pixels"), "2^63 pixels");
    CHECK(gbuffer_refusal(ok, 0, false, 1 << 24, kGbDepth, 65536, 65536) == nullptr, "2^56 pixels are the most");
    CHECK(has(gbuffer_refusal(ok, 0, false, (1 << 24) + 1, kGbDepth, 65536, 65536), "too many pixels"), "one view more");
    if (g_failed == before) std::printf("refusals ok\n");
}

void units() {
    const int before = g_failed;
    struct { uint32_t w, h; uint64_t blocks; } sizes[] = {{1, 1, 1}, {8, 8, 1}, {9, 7, 2}, {7, 9, 2}, {9, 9, 4}, {16, 16, 4}, {70, 45, 54},
                                                          {160, 90, 240}, {1920, 1080, 32400}, {3840, 2160, 129600}, {65536, 65536, uint64_t(1) << 26}};
    for (const auto &s : sizes) CHECK(gbuffer_blocks(s.w, s.h) == s.blocks, "%ux%u: %llu", s.w, s.h, (unsigned long long)gbuffer_blocks(s.w, s.h));
    CHECK(gbuffer_blocks_x(70) == 9 && gbuffer_blocks_x(1) == 1 && gbuffer_blocks_x(8) == 1 && gbuffer_blocks_x(9) == 2, "blocks_x");
    // units that are no multiple of four: the last workgroup has spare waves
    const uint64_t groups[][2] = {{0, 0}, {1, 1}, {2, 1}, {3, 1}, {4, 1}, {5, 2}, {54, 14}, {162, 41}, {32400, 8100}, {(uint64_t(1) << 30) + 1, (uint64_t(1) << 28) + 1}};
    for (const auto &g : groups) CHECK(gbuffer_groups(g[0]) == g[1], "%llu units", (unsigned long long)g[0]);
    // three views of 70x45: 162 units, view-major, in 41 workgroups that straddle the views (54 is no multiple of 4)
    const GbufferPlan P = plan_gbuffer(3, 70, 45);
    CHECK(P.units_per_view == 54 && P.total_units == 162 && P.launches.size() == 1, "3 x 70x45");
    if (P.launches.size() == 1) {
        const GbufferLaunch &L = P.launches[0];
        CHECK(L.first_view == 0 && L.n_views == 3 && L.n_units == 162 && L.groups == 41 && L.grid_x == 41 && L.grid_y == 1, "its launch");
    }
    const GbufferPlan one = plan_gbuffer(1, 1, 1);
    CHECK(one.launches.size() == 1 && one.launches[0].n_units == 1 && one.launches[0].groups == 1, "1x1");
    CHECK(plan_gbuffer(0, 70, 45).launches.empty() && plan_gbuffer(0, 70, 45).total_units == 0, "no views, no launch");
    if (g_failed == before) std::printf("units ok\n");
}

void elements() {
    const int before = g_failed;
    const uint32_t comps[kGbPlanes] = {1, 3, 3, 3, 2, 1, 1, 1};
    for (int i = 0; i < kGbPlanes; ++i) {
        CHECK(gbuffer_plane_elems(i, 3, 70, 45) == uint64_t(3) * 70 * 45 * comps[i], "plane %d", i);
        CHECK(gbuffer_plane_elems(i, 0, 70, 45) == 0, "plane %d without views", i);
    }
    // past 2^32 elements and past 2^32 bytes: 64 views of 8192x8192 pixels, and the largest call the plan lets through
    CHECK(gbuffer_plane_elems(1, 64, 8192, 8192) == (uint64_t(3) << 32), "64 x 8192^2 x 3");
    CHECK(gbuffer_plane_elems(3, uint64_t(1) << 24, 65536, 65536) == 3 * (uint64_t(1) << 56), "the most: 3 * 2^56, 12 * 2^56 bytes < 2^60");
    if (g_failed == before) std::printf("elements ok\n");
}

void grids() {
    const int before = g_failed;
    const uint64_t cases[] = {0, 1, 41, kGbGridX - 1, kGbGridX, kGbGridX + 1, 3 * uint64_t(kGbGridX), (uint64_t(1) << 28) - 1, uint64_t(1) << 28, (uint64_t(1) << 28) + 7};
    for (const uint64_t groups : cases) {
        uint32_t gx = 77, gy = 77;
        gbuffer_grid(groups, gx, gy);
        const uint64_t covered = uint64_t(gx) * gy;
        CHECK(covered >= groups && gx <= kGbGridX && gy <= 65535u, "%llu groups: %u x %u", (unsigned long long)groups, gx, gy);
        CHECK(groups == 0 ? covered == 0 : covered - groups < gx, "%llu groups: at most one partial row spare", (unsigned long long)groups);
        // 256 threads a workgroup: both dimensions stay below the runtime's 2^32 threads
        CHECK(uint64_t(gx) * 256u < (uint64_t(1) << 32), "threads along x");
    }
    if (g_failed == before) std::printf("grids ok\n");
}

void launches() {
    const int before = g_failed;
    // 7 views of 9x7 (2 units each) at 5 units a launch: whole views, 2 + 2 + 2 + 1
    const GbufferPlan P = plan_gbuffer(7, 9, 7, 5);
    CHECK(P.units_per_view == 2 && P.total_units == 14 && P.launches.size() == 4, "launches %zu", P.launches.size());
    uint64_t next = 0, units = 0;
    for (const GbufferLaunch &L : P.launches) {
        CHECK(L.first_view == next, "launches follow each other");
        CHECK(L.n_units == L.n_views * 2u && L.n_units <= 5u && L.groups == (L.n_units + 3u) / 4u, "whole views within the limit");
        next += L.n_views; units += L.n_units;
    }
    CHECK(next == 7 && units == 14, "all views, all units");
    // a view larger than the limit gets a launch of its own
    const GbufferPlan big = plan_gbuffer(3, 70, 45, 10);
    CHECK(big.launches.size() == 3 && big.launches[2].first_view == 2 && big.launches[2].n_units == 54, "one view a launch");
    // exactly at the limit: one launch; one unit less room: two
    CHECK(plan_gbuffer(4, 8, 8, 4).launches.size() == 1 && plan_gbuffer(4, 8, 8, 3).launches.size() == 2, "the limit is inclusive");
    if (g_failed == before) std::printf("launches ok\n");
}

void large() {
    const int before = g_failed;
    // 70,000 views of 4K: 9,072,000,000 units, past 2^32; 8,285 views (1,073,736,000 units <= 2^30) a launch, 9 launches
    const GbufferPlan P = plan_gbuffer(70000, 3840, 2160);
    CHECK(P.units_per_view == 129600 && P.total_units == 9072000000ull, "units %llu", (unsigned long long)P.total_units);
    CHECK(P.launches.size() == 9, "launches %zu", P.launches.size());
    uint64_t next = 0, units = 0;
    for (const GbufferLaunch &L : P.launches) {
        CHECK(L.first_view == next, "launches follow each other");
        CHECK(uint64_t(L.n_views) * 129600u == L.n_units && L.n_units <= kGbLaunchUnits, "whole views, unit numbers inside 32 bits");
        CHECK(uint64_t(L.grid_x) * L.grid_y >= L.groups && L.groups == (L.n_units + 3u) / 4u && L.grid_x <= kGbGridX, "grid");
        next += L.n_views; units += L.n_units;
    }
    CHECK(next == 70000 && units == P.total_units, "all views, all units");
    if (P.launches.size() == 9) {
        CHECK(P.launches[0].n_views == 8285 && P.launches[8].n_views == 70000 - 8 * 8285 && P.launches[0].grid_x == kGbGridX && P.launches[0].grid_y == 256, "8,285 views a launch");
        // where the last launch's planes begin: 66,280 views of 8,294,400 pixels, times three floats -- far past 2^32
        CHECK(gbuffer_plane_elems(1, P.launches[8].first_view, 3840, 2160) == 66280ull * 8294400ull * 3ull, "plane offset of the last launch");
    }
    // the largest view there is: 2^26 units, one launch each
    const GbufferPlan huge = plan_gbuffer(17, 65536, 65536);
    CHECK(huge.units_per_view == (1u << 26) && huge.launches.size() == 2 && huge.launches[0].n_views == 16 && huge.launches[0].n_units == (1u << 30) &&
          huge.launches[0].groups == (1u << 28) && huge.launches[1].n_views == 1, "17 views of 65536^2");
    if (g_failed == before) std::printf("large ok\n");
}

}  // namespace

int main() {
    masks();
    refusals();
    units();
    elements();
    grids();
    launches();
    large();
    if (g_failed != 0) return 1;
    std::printf("all ok\n");
    return 0;
}
