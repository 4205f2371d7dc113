// gbuffer_specular_plan.hpp on the host: what the plan of rtk_render_gbuffer_specular adds to gbuffer_plan.hpp
// (tests/test_cpp_gbuffer_specular_plan.py).  Pins worked out by hand: the twelve plane masks in the struct's order, the refusals in
// rtk.h's order with "no plane" between the views and the size of the call, and the element counts of the planes up to the
// largest call.  Plain g++, no HIP.  Prints "masks ok", "refusals ok", "elements ok", "all ok"; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gbuffer_specular_plan.hpp"

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
    static_assert(sizeof(rtk_gbuffer_specular) == 96, "twelve pointers");
    float f[12];
    uint32_t u[4];
    rtk_gbuffer_specular o;
    std::memset(&o, 0, sizeof(o));
    CHECK(gbuffer_specular_mask(o) == 0u, "empty");
    o.depth = f;
    CHECK(gbuffer_specular_mask(o) == kGsDepth, "depth %u", gbuffer_specular_mask(o));
    o.last_ray = f + 1;
    CHECK(gbuffer_specular_mask(o) == (kGsDepth | kGsLastRay), "depth + last_ray %u", gbuffer_specular_mask(o));
    o.position = f + 2; o.normal = f + 3; o.surface_position = f + 4; o.surface_normal = f + 5; o.albedo = f + 6; o.bary = f + 7;
    o.tri = u; o.mesh = u + 1; o.material = u + 2; o.bounces = u + 3;
    CHECK(gbuffer_specular_mask(o) == kGsAllPlanes && kGsAllPlanes == 4095u, "all %u", gbuffer_specular_mask(o));
    // plane i is field i of the struct, and bit i of the mask
    const void *want[kGsPlanes] = {f, f + 2, f + 3, f + 4, f + 5, f + 6, f + 7, u, u + 1, u + 2, u + 3, f + 1};
    const uint32_t bit[kGsPlanes] = {kGsDepth, kGsPosition, kGsNormal, kGsSurfacePosition, kGsSurfaceNormal, kGsAlbedo, kGsBary,
                                     kGsTri, kGsMesh, kGsMaterial, kGsBounces, kGsLastRay};
    for (int i = 0; i < kGsPlanes; ++i) {
        CHECK(gbuffer_specular_plane(o, i) == want[i], "plane %d", i);
        CHECK(bit[i] == 1u << i, "bit %d", i);
        CHECK(std::memcmp(reinterpret_cast<const char *>(&o) + 8 * i, &want[i], 8) == 0, "field %d of the struct", i);
    }
    uint32_t bytes = 0;
    for (int i = 0; i < kGsPlanes; ++i) bytes += 4u * kGsComps[i];
    CHECK(bytes == 112u, "bytes per pixel %u", bytes);
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
    CHECK(gbuffer_specular_refusal(ok, 0, false, 2, kGsDepth, 8, 8) == nullptr, "valid call");
    CHECK(gbuffer_specular_refusal(ok, 3, true, 1, kGsLastRay, 8, 8) == nullptr, "valid call, a plane above rtk_gbuffer's eight");
    CHECK(gbuffer_specular_refusal(ok, 0, false, 2, kGsBounces, 8, 8) == nullptr, "bounces alone");
    CHECK(gbuffer_specular_refusal(ok, 0, false, 0, kGsDepth, 8, 8) == nullptr, "n_views == 0 with views is no refusal");
    // each refusal wins over everything behind it in the list
    CHECK(has(gbuffer_specular_refusal(params(4, 2, 1), 4, true, -1, 0u, 8, 8), "sample"), "sample first");
    CHECK(has(gbuffer_specular_refusal(params(4, 2, 1), 0, true, -1, 0u, 8, 8), "sharded"), "world_size");
    CHECK(has(gbuffer_specular_refusal(params(4, 1, 1), 0, true, -1, 0u, 8, 8), "statistics"), "collect_stats");
    CHECK(has(gbuffer_specular_refusal(ok, 0, true, -1, 0u, 8, 8), "n_views must be >= 0"), "negative n_views");
    CHECK(has(gbuffer_specular_refusal(ok, 0, true, 0, 0u, 8, 8), "n_views must be 1"), "null views, n_views 0");
    CHECK(has(gbuffer_specular_refusal(ok, 0, true, 2, 0u, 8, 8), "n_views must be 1"), "null views, n_views 2");
    CHECK(has(gbuffer_specular_refusal(ok, 0, true, 1, 0u, 8, 8), "no plane"), "no plane, accel camera");
    CHECK(has(gbuffer_specular_refusal(ok, 0, false, 0, 0u, 8, 8), "rtk_gbuffer_specular"), "no plane names its struct, before n_views == 0");
    CHECK(has(gbuffer_specular_refusal(ok, 0, false, 2, 4096u, 8, 8), "no plane"), "bits above the twelve are no planes");
    // "no plane" before the size of the call; with a plane the size is judged
    CHECK(has(gbuffer_specular_refusal(ok, 0, false, 0x7FFFFFFF, 0u, 65536, 65536), "no plane"), "no plane before too many pixels");
    CHECK(has(gbuffer_specular_refusal(ok, 0, false, 0x7FFFFFFF, kGsDepth, 65536, 65536), "too many pixels"), "2^63 pixels");
    CHECK(gbuffer_specular_refusal(ok, 0, false, 1 << 24, kGsDepth, 65536, 65536) == nullptr, "2^56 pixels exactly");
    CHECK(has(gbuffer_specular_refusal(ok, 0, false, (1 << 24) + 1, kGsDepth, 65536, 65536), "too many pixels"), "2^56 + 2^32 pixels");
    if (g_failed == before) std::printf("refusals ok\n");
}

void elements() {
    const int before = g_failed;
    const uint32_t comps[kGsPlanes] = {1, 3, 3, 3, 3, 3, 2, 1, 1, 1, 1, 6};
    for (int i = 0; i < kGsPlanes; ++i) {
        CHECK(kGsComps[i] == comps[i], "comps %d", i);
        CHECK(gbuffer_specular_plane_elems(i, 3, 13, 9) == 351ull * comps[i], "13 x 9 x 3, plane %d", i);
        CHECK(gbuffer_specular_plane_elems(i, 0, 13, 9) == 0ull, "no views, plane %d", i);
        // past 2^32 elements, and the largest call: 2^56 pixels of 6 dwords are 3 * 2^57 dwords, 3 * 2^59 bytes
        CHECK(gbuffer_specular_plane_elems(i, 70000, 3840, 2160) == 580608000000ull * comps[i], "70,000 views of 3840 x 2160, plane %d", i);
        CHECK(gbuffer_specular_plane_elems(i, 1u << 24, 65536, 65536) == (uint64_t(comps[i]) << 56), "2^56 pixels, plane %d", i);
    }
    CHECK((gbuffer_specular_plane_elems(11, 1u << 24, 65536, 65536) * 4u) / 4u == (uint64_t(6) << 56), "the widest plane's bytes do not wrap");
    // units, grids and launches are rtk_render_gbuffer's: the same plan for the same views
    const GbufferPlan p = plan_gbuffer(3, 13, 9);
    CHECK(p.units_per_view == 4u && p.total_units == 12u && p.launches.size() == 1u && p.launches[0].groups == 3u, "13 x 9 x 3: 12 units, 3 workgroups");
    if (g_failed == before) std::printf("elements ok\n");
}

}  // namespace

int main() {
    masks();
    refusals();
    elements();
    if (g_failed != 0) return 1;
    std::printf("all ok\n");
    return 0;
}
