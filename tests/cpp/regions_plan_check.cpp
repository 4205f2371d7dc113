// regions_plan.hpp on the host: the plan of rtk_render_regions (tests/test_cpp_regions.py).  Pins worked out by hand for ragged
// rectangles, the packed offsets, the cut into launches at 150 units, then the sweep against the pairwise check on 2,000 seeded
// random lists.  Plain g++, no HIP.  Prints "units ok", "packed ok", "launches ok", "validity ok", "sweep N lists M overlapping
// ok", "large ok"; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "regions_plan.hpp"

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

// the ragged list of the issue: 1x1, 9x7, 8x8, a 1x200 row -- and an empty rectangle between them, which gets no entry
const rtk_rect kRagged[] = {{5, 5, 6, 6}, {10, 20, 19, 27}, {3, 3, 3, 9}, {16, 8, 24, 16}, {0, 100, 200, 101}};

bool brute_overlap(const std::vector<rtk_rect> &r) {
    for (size_t i = 0; i < r.size(); ++i)
        for (size_t j = i + 1; j < r.size(); ++j)
            if (regions_pair_overlaps(r[i], r[j])) return true;
    return false;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {                                                   // xorshift64*, seeded: the lists are the same every run
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return uint32_t((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

void units() {
    CHECK(region_blocks(kRagged[0]) == 1 && region_blocks(kRagged[1]) == 2 && region_blocks(kRagged[3]) == 1 && region_blocks(kRagged[4]) == 25,
          "blocks %u %u %u %u", region_blocks(kRagged[0]), region_blocks(kRagged[1]), region_blocks(kRagged[3]), region_blocks(kRagged[4]));
    CHECK(region_blocks({0, 0, 9, 9}) == 4 && region_blocks({0, 0, 8, 9}) == 2 && region_blocks({7, 7, 7, 7}) == 0, "9x9, 8x9, empty");
    const RegionsPlan P = plan_regions(kRagged, 5, RTK_REGIONS_IN_FRAME, 200, 131072);
    CHECK(P.entries.size() == 4 && P.launches.size() == 1, "entries %zu launches %zu", P.entries.size(), P.launches.size());
    if (P.entries.size() != 4 || P.launches.size() != 1) return;
    const uint32_t first_unit[4] = {0, 1, 3, 4};
    const uint64_t first_pixel[4] = {0, 1, 64, 128};
    for (int i = 0; i < 4; ++i) {
        const RegionEntry &e = P.entries[i];
        CHECK(e.first_unit == first_unit[i] && e.first_pixel == first_pixel[i], "entry %d: unit %u pixel %llu", i, e.first_unit, (unsigned long long)e.first_pixel);
        CHECK(e.pitch == 200 && e.base == 0, "entry %d in frame: pitch %u base %lld", i, e.pitch, (long long)e.base);
    }
    CHECK(P.entries[1].x0 == 10 && P.entries[1].y0 == 20 && P.entries[1].w == 9 && P.entries[1].h == 7, "9x7 entry");
    CHECK(P.entries[3].x0 == 0 && P.entries[3].y0 == 100 && P.entries[3].w == 200 && P.entries[3].h == 1, "row entry");
    CHECK(P.launches[0].first_entry == 0 && P.launches[0].n_entries == 4 && P.launches[0].n_units == 29 && P.launches[0].n_pixels == 328,
          "launch {%u %u %u %llu}", P.launches[0].first_entry, P.launches[0].n_entries, P.launches[0].n_units, (unsigned long long)P.launches[0].n_pixels);
    CHECK(P.total_units == 29 && P.total_pixels == 328, "totals %llu %llu", (unsigned long long)P.total_units, (unsigned long long)P.total_pixels);
    std::printf("units ok\n");
}

void packed() {
    const std::vector<uint64_t> off = regions_packed_offsets(kRagged, 5);
    const uint64_t expect[6] = {0, 3, 192, 192, 384, 984};
    for (int i = 0; i < 6; ++i) CHECK(off[i] == expect[i], "offset %d: %llu", i, (unsigned long long)off[i]);
    const RegionsPlan P = plan_regions(kRagged, 5, RTK_REGIONS_PACKED, 200, 131072);
    // every pixel of every rectangle lands at its dense place: 3 * (base + py * pitch + px) == offset + 3 * (row * w + column)
    size_t e = 0;
    for (int r = 0; r < 5; ++r) {
        if (region_empty(kRagged[r])) continue;
        const RegionEntry &E = P.entries[e++];
        for (int32_t y = kRagged[r].y0; y < kRagged[r].y1; ++y)
            for (int32_t x = kRagged[r].x0; x < kRagged[r].x1; ++x) {
                const int64_t at = 3 * (E.base + int64_t(y) * E.pitch + x);
                const int64_t want = int64_t(off[r]) + 3 * (int64_t(y - kRagged[r].y0) * (kRagged[r].x1 - kRagged[r].x0) + (x - kRagged[r].x0));
                CHECK(at == want, "rect %d pixel (%d, %d): %lld, expected %lld", r, x, y, (long long)at, (long long)want);
            }
    }
    // overlapping rectangles of a packed call: each its own copy, one behind the other
    const rtk_rect two[2] = {{0, 0, 4, 4}, {2, 2, 6, 5}};
    const RegionsPlan Q = plan_regions(two, 2, RTK_REGIONS_PACKED, 64, 131072);
    CHECK(Q.entries.size() == 2 && Q.entries[1].base == 16 - 2 * 4 - 2 && Q.entries[1].pitch == 4 && Q.total_pixels == 28, "overlapping pair");
    std::printf("packed ok\n");
}

void launches() {
    // 64x64 = 64 units each: two fit 150, a third does not; 128x104 = 208 units is larger than the limit and goes alone
    const rtk_rect r[] = {{0, 0, 64, 64}, {64, 0, 128, 64}, {0, 64, 64, 128}, {0, 0, 0, 0}, {0, 128, 128, 232}, {0, 232, 8, 240}, {8, 232, 16, 240}};
    const RegionsPlan P = plan_regions(r, 7, RTK_REGIONS_PACKED, 128, 150);
    CHECK(P.launches.size() == 4, "launches %zu", P.launches.size());
    if (P.launches.size() != 4) return;
    const uint32_t fe[4] = {0, 2, 3, 4}, ne[4] = {2, 1, 1, 2}, nu[4] = {128, 64, 208, 2};
    const uint64_t np[4] = {8192, 4096, 13312, 128};
    uint64_t packed_pixels = 0;
    for (int l = 0; l < 4; ++l) {
        const RegionLaunch &L = P.launches[l];
        CHECK(L.first_entry == fe[l] && L.n_entries == ne[l] && L.n_units == nu[l] && L.n_pixels == np[l], "launch %d: {%u %u %u %llu}", l,
              L.first_entry, L.n_entries, L.n_units, (unsigned long long)L.n_pixels);
        // prefixes start over in every launch; the packed offsets run through the call
        uint32_t units = 0;
        uint64_t pixels = 0;
        for (uint32_t i = 0; i < L.n_entries; ++i) {
            const RegionEntry &E = P.entries[L.first_entry + i];
            CHECK(E.first_unit == units && E.first_pixel == pixels, "launch %d entry %u prefixes", l, i);
            CHECK(E.base + int64_t(E.y0) * E.pitch + E.x0 == int64_t(packed_pixels), "launch %d entry %u packed offset", l, i);
            units += uint32_t((E.w + 7) / 8) * uint32_t((E.h + 7) / 8);
            pixels += uint64_t(E.w) * uint64_t(E.h);
            packed_pixels += uint64_t(E.w) * uint64_t(E.h);
        }
    }
    // a limit every rectangle fits under leaves one launch; a limit of 1 gives every rectangle its own
    CHECK(plan_regions(r, 7, RTK_REGIONS_IN_FRAME, 128, 1000).launches.size() == 1, "limit 1000");
    CHECK(plan_regions(r, 7, RTK_REGIONS_IN_FRAME, 128, 1).launches.size() == 6, "limit 1");
    CHECK(plan_regions(r, 0, RTK_REGIONS_IN_FRAME, 128, 150).launches.empty(), "no rectangles");
    std::printf("launches ok\n");
}

void validity() {
    CHECK(region_valid({0, 0, 200, 120}, 200, 120), "the whole frame");
    CHECK(region_valid({199, 119, 200, 120}, 200, 120) && region_valid({200, 120, 200, 120}, 200, 120), "last pixel; empty at the far corner");
    CHECK(!region_valid({0, 0, 201, 120}, 200, 120) && !region_valid({0, 0, 200, 121}, 200, 120), "one past the frame");
    CHECK(!region_valid({-1, 0, 5, 5}, 200, 120) && !region_valid({0, -1, 5, 5}, 200, 120), "negative corner");
    CHECK(!region_valid({5, 0, 4, 5}, 200, 120) && !region_valid({0, 5, 5, 4}, 200, 120), "inside out");
    std::printf("validity ok\n");
}

void sweep() {
    // touching edges and corners are disjoint; an empty rectangle overlaps nothing, wherever it lies
    const rtk_rect touch[] = {{0, 0, 8, 8}, {8, 0, 16, 8}, {0, 8, 8, 16}, {8, 8, 16, 16}, {4, 4, 4, 12}, {2, 2, 9, 2}};
    CHECK(!regions_overlap(touch, 6), "touching rectangles are disjoint");
    const rtk_rect one_pixel[] = {{0, 0, 8, 8}, {7, 7, 9, 9}};
    CHECK(regions_overlap(one_pixel, 2), "one shared pixel");
    const rtk_rect nested[] = {{0, 0, 100, 100}, {200, 0, 300, 100}, {40, 40, 41, 41}};
    CHECK(regions_overlap(nested, 3), "a pixel inside a large rectangle that entered long before");
    const rtk_rect same[] = {{3, 3, 5, 5}, {3, 3, 5, 5}};
    CHECK(regions_overlap(same, 2), "the same rectangle twice");
    int n_lists = 0, n_overlapping = 0;
    for (int list = 0; list < 2000; ++list) {
        // half of the lists are cut from a grid with random insets (mostly disjoint, edges that touch), half are free
        std::vector<rtk_rect> r;
        const bool grid = (list & 1) == 0;
        const int count = 1 + int(rnd(40));
        for (int i = 0; i < count; ++i) {
            rtk_rect q;
            if (grid) {
                const int32_t cx = int32_t(rnd(8)) * 16, cy = int32_t(rnd(8)) * 16;
                q.x0 = cx + int32_t(rnd(4)); q.y0 = cy + int32_t(rnd(4));
                q.x1 = cx + 16 - int32_t(rnd(4)); q.y1 = cy + 16 - int32_t(rnd(4));
                if (rnd(8) == 0) q.x1 = q.x0;                                // some are empty
                if (rnd(8) == 0) { q.x1 = cx + 16 + int32_t(rnd(2)); }        // some reach the next cell's edge, or one pixel into it
            } else {
                q.x0 = int32_t(rnd(120)); q.y0 = int32_t(rnd(120));
                q.x1 = q.x0 + int32_t(rnd(24)); q.y1 = q.y0 + int32_t(rnd(24));
            }
            r.push_back(q);
        }
        const bool want = brute_overlap(r), got = regions_overlap(r.data(), r.size());
        CHECK(want == got, "list %d of %d rectangles: sweep %d, pairwise %d", list, count, int(got), int(want));
        n_lists += 1; n_overlapping += want ? 1 : 0;
    }
    CHECK(n_overlapping > 200 && n_overlapping < 1800, "the lists exercise both answers: %d of %d overlap", n_overlapping, n_lists);
    std::printf("sweep %d lists %d overlapping ok\n", n_lists, n_overlapping);
}

void large() {
    // 65,536 disjoint 8x8 rectangles of a 2048x2048 grid, then the same with the last one moved onto the first
    std::vector<rtk_rect> r;
    for (int32_t y = 0; y < 256; ++y)
        for (int32_t x = 0; x < 256; ++x) r.push_back({x * 8, y * 8, x * 8 + 8, y * 8 + 8});
    CHECK(!regions_overlap(r.data(), r.size()), "65,536 disjoint rectangles");
    r.back() = {7, 7, 9, 9};
    CHECK(regions_overlap(r.data(), r.size()), "65,536 rectangles, one pair overlapping");
    const RegionsPlan P = plan_regions(r.data(), r.size(), RTK_REGIONS_IN_FRAME, 2048, 131072);
    CHECK(P.entries.size() == 65536 && P.launches.size() == 1 && P.total_units == 65536, "one launch of 65,536 units");
    std::printf("large ok\n");
}

}  // namespace

int main() {
    units();
    packed();
    launches();
    validity();
    sweep();
    large();
    if (g_failed) return 1;
    std::printf("all ok\n");
    return 0;
}
