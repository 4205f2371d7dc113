// Drives hip_accel::set_camera / camera_now / render_views (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins
// for the reference's types: the floor and mirror of update_check.cpp seen from three cameras -- the scene's own, one moved up and
// to the right, one turned half round (it looks away from everything).  Prints the camera round trip first (that part needs no
// device), then the three 16 x 16 views by bits and how set_camera + render_frame compares with them, so
// tests/test_cpp_views.py can compare them with the CPU oracle.  Without a device the adapter's exception is printed and the
// exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
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
    // (tests/test_cpp_views.py holds the same numbers)
    const camera<F> cams[3] = {sc.viewpoint,
                               {{1.f, 0.5f, 0.25f}, {{0.96f, 0.f, 0.28f, 0.f, 1.f, 0.f, -0.28f, 0.f, 0.96f}}},
                               {{0.f, 0.f, 0.f}, {{-1, 0, 0, 0, 1, 0, 0, 0, -1}}}};
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        const camera<F> built = accel.camera_now();
        accel.set_camera(cams[1]);
        const camera<F> moved = accel.camera_now();
        bool round = built.position.x == 0.f && built.matrix.m[0] == 1.f && built.matrix.m[8] == 1.f;
        round = round && bits(moved.position.x) == bits(cams[1].position.x) && bits(moved.position.z) == bits(cams[1].position.z);
        for (std::size_t i = 0; i < 9; ++i) round = round && bits(moved.matrix.m[i]) == bits(cams[1].matrix.m[i]);
        std::printf("round trip %d\n", round ? 1 : 0);
        std::fflush(stdout);
        accel.set_camera(cams[0]);
        rtk_render_params fp = A::default_params();
        fp.width = 16; fp.height = 16;
        rtk_counters total{};
        const auto views = accel.render_views(std::span<const camera<F>>(cams, 3), fp, &total);
        std::size_t same = 0;
        unsigned long long rays = 0;
        for (std::size_t v = 0; v < 3; ++v) {
            accel.set_camera(cams[v]);
            rtk_counters cn{};
            const auto one = accel.render_frame(fp, &cn);
            rays += cn.rays;
            for (std::size_t y = 0; y < 16; ++y)
                for (std::size_t x = 0; x < 16; ++x) {
                    const auto &a = views[v][y][x];
                    const auto &b = one[y][x];
                    same += bits(a.red) == bits(b.red) && bits(a.green) == bits(b.green) && bits(a.blue) == bits(b.blue);
                    std::printf("view %zu pixel %zu %08x %08x %08x\n", v, y * 16 + x, bits(a.red), bits(a.green), bits(a.blue));
                }
        }
        std::printf("same %zu rays %llu of %llu primary %llu\n", same, (unsigned long long)total.rays, rays, (unsigned long long)total.primary);
        const auto none = accel.render_views(std::span<const camera<F>>(), fp);
        std::printf("no views %zu\n", none.size());
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
