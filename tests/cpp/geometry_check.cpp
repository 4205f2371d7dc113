// Drives hip_accel::update_geometry (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the reference's
// types: the floor and mirror of update_check.cpp, built, then given other TRIANGLES: the floor keeps only its second triangle,
// the mirror gets a third (its first again, wound the other way), and the mirror's vertices move as they do there.  Prints the
// 16 x 16 frame of the changed scene by bits and a few hits, so tests/test_cpp_geometry.py can compare them with the CPU oracle
// built from the same arrays.  Without a device the adapter's exception is printed and the exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <vector>

#include "hip_accel.hpp"

using F = float;

static mesh_object<F> mesh_of(std::size_t material, std::size_t mesh_idx, const vec3<F> (&v)[4], const std::vector<std::array<std::size_t, 3>> &idx,
                              const vec3<F> &n) {
    mesh_object<F> m{};
    m.material_idx = material;
    m.vertices = {v[0], v[1], v[2], v[3]};
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
    const std::vector<std::array<std::size_t, 3>> two = {{0, 1, 2}, {0, 2, 3}};
    sc.meshes.push_back(mesh_of(0, 0, floor_v, two, {0.f, 1.f, 0.f}));
    sc.meshes.push_back(mesh_of(1, 1, wall_v, two, {0.f, 0.f, 1.f}));
    // the changed scene (tests/test_cpp_geometry.py holds the same numbers)
    const vec3<F> wall_m[4] = {{-1.5f, -0.5f, -5.f}, {1.5f, -0.5f, -4.5f}, {1.5f, 1.5f, -4.5f}, {-1.5f, 1.5f, -5.f}};
    scene<F> changed = sc;
    changed.meshes.clear();
    changed.meshes.push_back(mesh_of(0, 0, floor_v, {{0, 2, 3}}, {0.f, 1.f, 0.f}));
    changed.meshes.push_back(mesh_of(1, 1, wall_m, {{0, 1, 2}, {0, 2, 3}, {0, 2, 1}}, {0.f, 0.f, 1.f}));
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        rtk_render_params fp = A::default_params();
        fp.width = 16; fp.height = 16;
        accel.update_geometry(std::make_shared<const scene<F>>(changed));
        const auto a = accel.render_frame(fp);
        // back to the scene as built, then the same change again
        accel.update_geometry(std::make_shared<const scene<F>>(sc));
        accel.update_geometry(std::make_shared<const scene<F>>(changed));
        rtk_counters cn{};
        const auto b = accel.render_frame(fp, &cn);
        std::size_t same = 0;
        for (std::size_t y = 0; y < 16; ++y)
            for (std::size_t x = 0; x < 16; ++x) {
                same += bits(a[y][x].red) == bits(b[y][x].red) && bits(a[y][x].green) == bits(b[y][x].green) && bits(a[y][x].blue) == bits(b[y][x].blue);
                std::printf("pixel %zu %08x %08x %08x\n", y * 16 + x, bits(b[y][x].red), bits(b[y][x].green), bits(b[y][x].blue));
            }
        std::printf("same %zu rays %llu\n", same, (unsigned long long)cn.rays);
        rtk_tree_info ti{};
        rtk_accel_tree_info(accel.handle(), &ti);
        std::printf("triangles %d\n", ti.n_triangles);
        // one ray at the moved mirror from behind, without culling: the hit is the mirror's THIRD triangle or one of the first two
        // (the same surface); its record is rebuilt from the changed scene's triangle list
        const auto h = accel.intersect<false>(ray3<F>{vec3<F>{0.5f, 0.f, 0.f}, vec3<F>{0.f, 0.f, -1.f}});
        if (h) std::printf("hit t %08x mesh %zu\n", bits(h->distance), h->mesh_idx);
        else std::printf("hit none\n");
        // the floor's first triangle is gone: a ray straight down onto it now misses, one onto the second still hits
        const auto gone = accel.intersect<true>(ray3<F>{vec3<F>{2.f, 0.f, -1.f}, vec3<F>{0.f, -1.f, 0.f}});
        const auto kept = accel.intersect<true>(ray3<F>{vec3<F>{-2.f, 0.f, -5.f}, vec3<F>{0.f, -1.f, 0.f}});
        std::printf("gone %d kept %d\n", gone ? 1 : 0, kept ? 1 : 0);
        bool threw = false;
        scene<F> other = changed;
        other.meshes[1].vertices.pop_back();
        try { accel.update_geometry(std::make_shared<const scene<F>>(other)); } catch (const std::invalid_argument &) { threw = true; }
        std::printf("other vertex count throws %d\n", threw ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
