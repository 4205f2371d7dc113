// Drives hip_accel::render_gbuffer_specular (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the reference's
// types: the floor and mirror of views_check.cpp seen from its three cameras.  Prints first what needs no device (a call without
// planes and a sample outside [0, spp) are refused), then the twelve planes of the three 16 x 16 views by bits, a call for two
// planes alone and the accel's own camera, so tests/test_cpp_gbuffer_specular.py can compare them with the model over the CPU
// oracle.  Without a device the adapter's exception is printed and the exit status is 3.
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
        rtk_render_params fp = A::default_params();
        fp.width = 16; fp.height = 16;
        int refused = 0;
        try { (void)accel.render_gbuffer_specular(fp, 0, std::span<const camera<F>>(cams, 3), 0u); } catch (const std::exception &) { refused += 1; }
        try { (void)accel.render_gbuffer_specular(fp, 1, std::span<const camera<F>>(cams, 3)); } catch (const std::exception &) { refused += 1; }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        const auto g = accel.render_gbuffer_specular(fp, 0, std::span<const camera<F>>(cams, 3));
        std::printf("shape %zu %zu %zu\n", g.views, g.height, g.width);
        const auto row = [](const std::vector<float> &plane, std::size_t p, std::size_t comps) {
            for (std::size_t c = 0; c < comps; ++c) std::printf(" %08x", bits(plane[p * comps + c]));
        };
        for (std::size_t v = 0; v < 3; ++v)
            for (std::size_t i = 0; i < 256; ++i) {
                const std::size_t p = v * 256 + i;
                std::printf("view %zu pixel %zu %08x %08x %08x %08x %08x", v, i, bits(g.depth[p]), g.tri[p], g.mesh[p], g.material[p], g.bounces[p]);
                row(g.position, p, 3); row(g.normal, p, 3); row(g.surface_position, p, 3); row(g.surface_normal, p, 3); row(g.albedo, p, 3);
                row(g.bary, p, 2); row(g.last_ray, p, 6);
                std::printf("\n");
            }
        // two planes alone, and the accel's own camera: the same bits
        const auto d = accel.render_gbuffer_specular(fp, 0, std::span<const camera<F>>(cams, 3), A::specular_depth | A::specular_bounces);
        std::size_t same = 0;
        for (std::size_t p = 0; p < 768; ++p) same += bits(d.depth[p]) == bits(g.depth[p]) && d.bounces[p] == g.bounces[p];
        accel.set_camera(cams[1]);
        const auto own = accel.render_gbuffer_specular(fp, 0, std::span<const camera<F>>(), A::specular_depth | A::specular_mesh);
        std::size_t same_own = 0;
        for (std::size_t p = 0; p < 256; ++p) same_own += bits(own.depth[p]) == bits(g.depth[256 + p]) && own.mesh[p] == g.mesh[256 + p];
        std::printf("two planes same %zu others empty %d own camera same %zu of %zu views %zu\n", same,
                    (d.tri.empty() && d.albedo.empty() && d.position.empty() && d.last_ray.empty()) ? 1 : 0, same_own, own.depth.size(), own.views);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
