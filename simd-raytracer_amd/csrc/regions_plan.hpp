// Host plan of rtk_render_regions (api_regions.hip): what the rectangles of a call are allowed to be, which of them overlap,
// where each one's 8x8 pixel blocks sit among the units of a launch, where its pixels sit in the output, and how a call of many
// units is cut into launches of whole rectangles.  Plain integers, no HIP, no accel: tests/cpp/regions_plan_check.cpp runs it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rtk.h"

namespace rtk {

constexpr int32_t kMaxRegions = 65536;                        // rectangles of one call at most (rtk.h)

// One rectangle as the kernels see it (k_render<..., REGIONS>, k_region_rays, k_region_accumulate): 40 bytes, read through the
// scalar cache.  Pixel (px, py) of the frame, inside the rectangle, lives at float 3 * (base + py * pitch + px) of the output:
//   RTK_REGIONS_IN_FRAME   pitch = the frame's width, base = 0
//   RTK_REGIONS_PACKED     pitch = the rectangle's width, base = (pixels of the rectangles before it) - y0 * pitch - x0
// so the kernels do not know the layouts apart.  first_unit / first_pixel count from the start of the LAUNCH the entry belongs to.
struct RegionEntry {
    int32_t x0, y0, w, h;
    uint32_t first_unit;                                      // 8x8 blocks of the launch's entries before this one
    uint32_t pitch;
    int64_t base;
    uint64_t first_pixel;                                     // pixels of the launch's entries before this one
};
static_assert(sizeof(RegionEntry) == 40, "RegionEntry is read by the device as it is laid out here");

struct RegionLaunch { uint32_t first_entry, n_entries, n_units; uint64_t n_pixels; };

struct RegionsPlan {
    std::vector<RegionEntry> entries;                         // the rectangles that have pixels, in the caller's order
    std::vector<RegionLaunch> launches;                       // whole entries each, in order
    uint64_t total_pixels = 0;                                // sum of the areas (overlaps of a packed call count twice)
    uint64_t total_units = 0;
};

inline bool region_empty(const rtk_rect &r) { return r.x0 == r.x1 || r.y0 == r.y1; }
inline uint64_t region_area(const rtk_rect &r) { return uint64_t(r.x1 - r.x0) * uint64_t(r.y1 - r.y0); }
inline uint32_t region_blocks(const rtk_rect &r) {            // 8x8 blocks anchored at the rectangle's own corner
    return uint32_t((r.x1 - r.x0 + 7) / 8) * uint32_t((r.y1 - r.y0 + 7) / 8);
}

// inside the frame and not inside out; an empty rectangle is legal anywhere inside [0, width] x [0, height]
inline bool region_valid(const rtk_rect &r, int64_t width, int64_t height) {
    return r.x0 >= 0 && r.y0 >= 0 && r.x1 >= r.x0 && r.y1 >= r.y0 && r.x1 <= width && r.y1 <= height;
}

inline bool regions_pair_overlaps(const rtk_rect &a, const rtk_rect &b) {
    if (region_empty(a) || region_empty(b)) return false;
    return a.x0 < b.x1 && b.x0 < a.x1 && a.y0 < b.y1 && b.y0 < a.y1;
}

// Do two rectangles share a pixel?  A sweep down the frame: the rectangles sorted by y0 enter a set of "open" rectangles ordered
// by x0 and leave it when the sweep passes their y1.  The open ones are pairwise disjoint in x as long as no overlap has been
// found, so a newcomer only has to be compared with its two neighbours in x.  O(n log n); 65,536 rectangles are a few
// milliseconds where the pairwise check is two thousand million comparisons.
inline bool regions_overlap(const rtk_rect *rects, size_t n) {
    std::vector<uint32_t> by_y0, by_y1;
    for (size_t i = 0; i < n; ++i)
        if (!region_empty(rects[i])) by_y0.push_back(uint32_t(i));
    by_y1 = by_y0;
    std::sort(by_y0.begin(), by_y0.end(), [&](uint32_t a, uint32_t b) { return rects[a].y0 < rects[b].y0; });
    std::sort(by_y1.begin(), by_y1.end(), [&](uint32_t a, uint32_t b) { return rects[a].y1 < rects[b].y1; });
    // open rectangles as a sorted vector of (x0, index): insertion is a memmove, cheap next to the sorts at these sizes
    std::vector<std::pair<int32_t, uint32_t>> open;
    size_t leave = 0;
    for (const uint32_t i : by_y0) {
        const rtk_rect &r = rects[i];
        for (; leave < by_y1.size() && rects[by_y1[leave]].y1 <= r.y0; ++leave) {      // rows [y0, y1): y1 == r.y0 only touches
            const uint32_t j = by_y1[leave];
            const auto it = std::lower_bound(open.begin(), open.end(), std::make_pair(rects[j].x0, j));
            if (it != open.end() && it->second == j) open.erase(it);
        }
        const auto at = std::lower_bound(open.begin(), open.end(), std::make_pair(r.x0, uint32_t(0)));
        if (at != open.end() && rects[at->second].x0 < r.x1) return true;              // the neighbour to the right starts inside r
        if (at != open.begin() && rects[(at - 1)->second].x1 > r.x0) return true;      // the neighbour to the left reaches into r
        open.insert(std::lower_bound(open.begin(), open.end(), std::make_pair(r.x0, i)), std::make_pair(r.x0, i));
    }
    return false;
}

// The table and the launches.  `rects` are valid (region_valid) and, under RTK_REGIONS_IN_FRAME, disjoint.  limit_units: units of
// one launch at most (rtk_knobs::views_launch_units); a rectangle larger than that gets a launch of its own.  Packed offsets count
// every rectangle of the CALL, so the launches of a call write one packed buffer.
inline RegionsPlan plan_regions(const rtk_rect *rects, size_t n, int layout, uint32_t frame_width, uint64_t limit_units) {
    RegionsPlan P;
    uint64_t packed = 0;
    RegionLaunch L = {0u, 0u, 0u, 0ull};
    for (size_t i = 0; i < n; ++i) {
        const rtk_rect &r = rects[i];
        if (region_empty(r)) continue;
        const uint32_t blocks = region_blocks(r);
        if (L.n_entries > 0 && uint64_t(L.n_units) + blocks > limit_units) {
            P.launches.push_back(L);
            L = {uint32_t(P.entries.size()), 0u, 0u, 0ull};
        }
        RegionEntry e;
        e.x0 = r.x0; e.y0 = r.y0; e.w = r.x1 - r.x0; e.h = r.y1 - r.y0;
        e.first_unit = L.n_units; e.first_pixel = L.n_pixels;
        if (layout == RTK_REGIONS_PACKED) {
            e.pitch = uint32_t(e.w);
            e.base = int64_t(packed) - int64_t(e.y0) * int64_t(e.w) - int64_t(e.x0);
        } else {
            e.pitch = frame_width;
            e.base = 0;
        }
        P.entries.push_back(e);
        L.n_entries += 1; L.n_units += blocks; L.n_pixels += region_area(r);
        packed += region_area(r);
        P.total_units += blocks;
    }
    if (L.n_entries > 0) P.launches.push_back(L);
    P.total_pixels = packed;
    return P;
}

// float offset of rectangle r in the packed output: 3 * (area of the rectangles before it)
inline std::vector<uint64_t> regions_packed_offsets(const rtk_rect *rects, size_t n) {
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + 3 * region_area(rects[i]);
    return off;
}

}  // namespace rtk
