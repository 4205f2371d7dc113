// Drives hip_accel::set_lights / lights_now, set_materials / materials_now and set_background / background_now
// (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the reference's types, on the floor and mirror of
// views_check.cpp.  Prints the round trips first (that part needs no device), then one 16 x 16 frame per state by bits -- the
// scene as built; two other lights; the wall turned into glass and the floor recoloured; another background -- so
// tests/test_cpp_scene_state.py can compare them with the CPU oracle.  Without a device the adapter's exception is printed on the
// first frame and the exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <variant>
#include <vector>

#include "hip_accel.hpp"

using F = float;

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

template <typename A>
static void frame(const A &accel, int state) {
    rtk_render_params fp = A::default_params();
    fp.width = 16; fp.height = 16;
    rtk_counters cn{};
    const auto px = accel.render_frame(fp, &cn);
    for (std::size_t y = 0; y < 16; ++y)
        for (std::size_t x = 0; x < 16; ++x)
            std::printf("state %d pixel %zu %08x %08x %08x\n", state, y * 16 + x, bits(px[y][x].red), bits(px[y][x].green), bits(px[y][x].blue));
    std::printf("state %d rays %llu\n", state, (unsigned long long)cn.rays);
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
    // (tests/test_cpp_scene_state.py holds the same numbers)
    const std::vector<light<F>> lights = {{{2.f, 2.5f, -1.f}, 90.f}, {{-1.5f, 1.f, -3.f}, -0.0f}};
    const std::vector<material_variant<F>> materials = {diffuse_material<F>{{0.2f, 0.7f, 0.4f}, true}, refractive_material<F>{1.5f, false}};
    const color<F> background{-0.0f, 0.125f, 0.5f};
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        const auto l0 = accel.lights_now();
        bool round = l0.size() == 1 && bits(l0[0].position.y) == bits(3.f) && bits(l0[0].intensity) == bits(150.f);
        accel.set_lights(lights);
        const auto l1 = accel.lights_now();
        round = round && l1.size() == 2 && bits(l1[1].intensity) == bits(-0.0f) && bits(l1[0].position.x) == bits(2.f) && bits(l1[1].position.z) == bits(-3.f);
        accel.set_lights(std::span<const light<F>>());
        round = round && accel.lights_now().empty();
        const auto m0 = accel.materials_now();
        round = round && m0.size() == 2 && std::holds_alternative<diffuse_material<F>>(m0[0]) && std::holds_alternative<reflective_material<F>>(m0[1]) &&
                bits(std::get<diffuse_material<F>>(m0[0]).albedo.green) == bits(0.6f);
        accel.set_materials(materials);
        const auto m1 = accel.materials_now();
        round = round && std::holds_alternative<refractive_material<F>>(m1[1]) && bits(std::get<refractive_material<F>>(m1[1]).ior) == bits(1.5f) &&
                std::get<diffuse_material<F>>(m1[0]).smooth_shading && bits(std::get<diffuse_material<F>>(m1[0]).albedo.red) == bits(0.2f);
        const color<F> b0 = accel.background_now();
        accel.set_background(background);
        const color<F> b1 = accel.background_now();
        round = round && bits(b0.blue) == bits(0.75f) && bits(b1.red) == bits(-0.0f) && bits(b1.green) == bits(0.125f);
        bool refused = false;
        try { accel.set_materials(std::span<const material_variant<F>>(materials.data(), 1)); } catch (const std::exception &) { refused = true; }
        std::printf("round trip %d refused %d\n", round ? 1 : 0, refused ? 1 : 0);
        std::fflush(stdout);
        // back to the scene as built, then one state after the other
        accel.set_lights(sc.lights);
        accel.set_materials(sc.materials);
        accel.set_background(sc.config.background_color);
        frame(accel, 0);
        accel.set_lights(lights);
        frame(accel, 1);
        accel.set_materials(materials);
        frame(accel, 2);
        accel.set_background(background);
        frame(accel, 3);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
