// Drives hip_accel::render_regions / render_regions_into (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the
// reference's types: the floor and mirror of views_check.cpp at 16 x 16, cut into tiles of the reference's render_tile shape
// (std::size_t corners).  Prints first what needs no device (no tiles, tiles without pixels, a tile past the frame refused), then
// every tile of the packed call by bits and how it compares with the crop of render_frame, then the in-frame call: the tiles'
// pixels and a count of the pixels outside them that kept the sentinel.  tests/test_cpp_regions.py compares the bits with the CPU
// oracle.  Without a device the adapter's exception is printed and the exit status is 3.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <vector>

#include "hip_accel.hpp"

using F = float;

struct tile { std::size_t x0, y0, x1, y1; };     // render_tile, render/tile/tile.hpp

static mesh_object<F> mesh_of(std::size_t material, std::size_t mesh_idx, const vec3<F> (&v)[4], const vec3<F> &n) {
    mesh_object<F> m{};
    m.material_idx = material;
    m.vertices = {v[0], v[1], v[2], v[3]};
    const std::size_t idx[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (const auto &i : idx) {
        triangle<F> t{};
        t.v0 = m.vertices[i[0]]; t.v1 = m.vertices[i[1]]; t.v2 = m.vertices[i[2]];
        t.normal = n;
        t.vertex_indices = {i[0], i[1], i[2]};
        t.mesh_idx = mesh_idx;
        m.triangles.push_back(t);
    }
    return m;
}

static std::uint32_t bits(F f) {
    std::uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}

static bool same(const color<F> &a, const color<F> &b) {
    return bits(a.red) == bits(b.red) && bits(a.green) == bits(b.green) && bits(a.blue) == bits(b.blue);
}

int main() {
    using A = hip_accel<F, 1e-6f>;
    scene<F> sc{};
    sc.config = {{0.25f, 0.5f, 0.75f}, 16, 16, 64};
    sc.viewpoint = {{0.f, 0.f, 0.f}, {{1, 0, 0, 0, 1, 0, 0, 0, 1}}};
    sc.lights.push_back({{0.f, 3.f, -2.f}, 150.f});
    sc.materials.push_back(diffuse_material<F>{{0.9f, 0.6f, 0.3f}, false});
    sc.materials.push_back(reflective_material<F>{{1.f, 1.f, 1.f}, false});
    const vec3<F> floor_v[4] = {{-3.f, -1.f, 0.f}, {3.f, -1.f, 0.f}, {3.f, -1.f, -6.f}, {-3.f, -1.f, -6.f}};
    const vec3<F> wall_v[4] = {{-1.5f, -1.f, -4.f}, {1.5f, -1.f, -4.f}, {1.5f, 1.f, -4.f}, {-1.5f, 1.f, -4.f}};
    sc.meshes.push_back(mesh_of(0, 0, floor_v, {0.f, 1.f, 0.f}));
    sc.meshes.push_back(mesh_of(1, 1, wall_v, {0.f, 0.f, 1.f}));
    // (tests/test_cpp_regions.py holds the same numbers) a ragged tile, one that overlaps it, one pixel, one without pixels, a row
    const tile packed_tiles[5] = {{1, 2, 12, 9}, {8, 6, 16, 16}, {15, 0, 16, 1}, {4, 4, 4, 9}, {0, 11, 16, 12}};
    const tile frame_tiles[4] = {{1, 2, 12, 9}, {12, 2, 16, 16}, {15, 0, 16, 1}, {0, 11, 12, 12}};
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        rtk_render_params fp = A::default_params();
        fp.width = 16; fp.height = 16;
        const auto none = accel.render_regions(std::span<const tile>(), fp);
        const tile hollow[2] = {{3, 3, 3, 9}, {16, 16, 16, 16}};
        const auto empty = accel.render_regions(std::span<const tile>(hollow, 2), fp);
        std::printf("no tiles %zu hollow %zu %zu %zu\n", none.size(), empty.size(), empty[0].size(), empty[1].size());
        int refused = 0;
        const tile past[1] = {{0, 0, 17, 16}};
        try { (void)accel.render_regions(std::span<const tile>(past, 1), fp); } catch (const std::exception &) { refused = 1; }
        std::printf("past the frame refused %d\n", refused);
        std::fflush(stdout);

        rtk_counters total{}, whole{};
        const auto tiles = accel.render_regions(std::span<const tile>(packed_tiles, 5), fp, &total);
        const auto frame = accel.render_frame(fp, &whole);
        std::size_t equal = 0, pixels = 0;
        for (std::size_t t = 0; t < 5; ++t) {
            const tile &q = packed_tiles[t];
            std::printf("tile %zu shape %zu %zu\n", t, tiles[t].size(), tiles[t].empty() ? std::size_t(0) : tiles[t][0].size());
            for (std::size_t y = q.y0; y < q.y1; ++y)
                for (std::size_t x = q.x0; x < q.x1; ++x) {
                    const auto &a = tiles[t][y - q.y0][x - q.x0];
                    equal += same(a, frame[y][x]);
                    pixels += 1;
                    std::printf("tile %zu pixel %zu %08x %08x %08x\n", t, y * 16 + x, bits(a.red), bits(a.green), bits(a.blue));
                }
        }
        std::printf("packed same %zu of %zu primary %llu\n", equal, pixels, (unsigned long long)total.primary);

        std::vector<std::vector<color<F>>> image(16, std::vector<color<F>>(16, color<F>{-7.f, -7.f, -7.f}));
        rtk_counters in_frame{};
        accel.render_regions_into(image, std::span<const tile>(frame_tiles, 4), fp, &in_frame);
        std::size_t inside = 0, inside_same = 0, outside_kept = 0;
        for (std::size_t y = 0; y < 16; ++y)
            for (std::size_t x = 0; x < 16; ++x) {
                bool in = false;
                for (const tile &q : frame_tiles) in = in || (x >= q.x0 && x < q.x1 && y >= q.y0 && y < q.y1);
                if (in) { inside += 1; inside_same += same(image[y][x], frame[y][x]); }
                else outside_kept += same(image[y][x], color<F>{-7.f, -7.f, -7.f});
            }
        std::printf("in frame same %zu of %zu outside kept %zu of %zu primary %llu\n", inside_same, inside, outside_kept, 256 - inside,
                    (unsigned long long)in_frame.primary);
        // the frame cut into four quarters: their rays add up to the frame's
        const tile quarters[4] = {{0, 0, 8, 8}, {8, 0, 16, 8}, {0, 8, 8, 16}, {8, 8, 16, 16}};
        rtk_counters q4{};
        (void)accel.render_regions(std::span<const tile>(quarters, 4), fp, &q4);
        std::printf("quarters rays %llu frame rays %llu primary %llu\n", (unsigned long long)q4.rays, (unsigned long long)whole.rays, (unsigned long long)q4.primary);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
