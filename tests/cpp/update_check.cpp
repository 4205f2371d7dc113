// Drives hip_accel::update_vertices (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the reference's
// types: the floor and mirror of radiance_check.cpp, built, then moved (the mirror pushed back, turned and raised, the floor
// lowered on one side) through both overloads.  Prints the 16 x 16 frame of the moved scene by bits and a few hits, so
// tests/test_cpp_update.py can compare them with the CPU oracle built from the moved vertices.  Without a device the adapter's
// exception is printed and the exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <vector>

#include "hip_accel.hpp"

using F = float;

static mesh_object<F> quad(std::size_t material, std::size_t mesh_idx, const vec3<F> (&v)[4], const vec3<F> &n) {
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
    sc.meshes.push_back(quad(0, 0, floor_v, {0.f, 1.f, 0.f}));
    sc.meshes.push_back(quad(1, 1, wall_v, {0.f, 0.f, 1.f}));
    // the moved scene (tests/test_cpp_update.py holds the same numbers)
    const vec3<F> floor_m[4] = {{-3.f, -1.5f, 0.f}, {3.f, -1.f, 0.f}, {3.f, -1.f, -6.f}, {-3.f, -1.5f, -6.f}};
    const vec3<F> wall_m[4] = {{-1.5f, -0.5f, -5.f}, {1.5f, -0.5f, -4.5f}, {1.5f, 1.5f, -4.5f}, {-1.5f, 1.5f, -5.f}};
    scene<F> moved = sc;
    moved.meshes.clear();
    moved.meshes.push_back(quad(0, 0, floor_m, {0.f, 1.f, 0.f}));
    moved.meshes.push_back(quad(1, 1, wall_m, {0.f, 0.f, 1.f}));
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        rtk_render_params fp = A::default_params();
        fp.width = 16; fp.height = 16;
        std::vector<vec3<F>> flat;
        for (const auto &m : moved.meshes) flat.insert(flat.end(), m.vertices.begin(), m.vertices.end());
        accel.update_vertices(flat);
        const auto a = accel.render_frame(fp);
        // back, then the same through the overload that takes the moved scene
        std::vector<vec3<F>> back;
        for (const auto &m : sc.meshes) back.insert(back.end(), m.vertices.begin(), m.vertices.end());
        accel.update_vertices(back);
        accel.update_vertices(std::make_shared<const scene<F>>(moved));
        rtk_counters cn{};
        const auto b = accel.render_frame(fp, &cn);
        std::size_t same = 0;
        for (std::size_t y = 0; y < 16; ++y)
            for (std::size_t x = 0; x < 16; ++x) {
                same += bits(a[y][x].red) == bits(b[y][x].red) && bits(a[y][x].green) == bits(b[y][x].green) && bits(a[y][x].blue) == bits(b[y][x].blue);
                std::printf("pixel %zu %08x %08x %08x\n", y * 16 + x, bits(b[y][x].red), bits(b[y][x].green), bits(b[y][x].blue));
            }
        std::printf("same %zu rays %llu\n", same, (unsigned long long)cn.rays);
        // one ray at the moved mirror: the hit carries the moved scene's triangle (scene_ptr was swapped)
        const auto h = accel.intersect<true>(ray3<F>{vec3<F>{0.f, 0.5f, 0.f}, vec3<F>{0.f, 0.f, -1.f}});
        if (h) std::printf("hit t %08x mesh %zu moved %d\n", bits(h->distance), h->mesh_idx, accel.scene_ptr->meshes[1].vertices[0].z == -5.f ? 1 : 0);
        else std::printf("hit none\n");
        bool threw = false;
        try { accel.update_vertices(std::vector<vec3<F>>(3)); } catch (const std::invalid_argument &) { threw = true; }
        std::printf("wrong size throws %d\n", threw ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
