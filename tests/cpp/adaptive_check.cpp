// Drives hip_accel::render_adaptive (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the reference's types: the
// floor and mirror of views_check.cpp, 16 x 16, diffuse GI, at most 4 samples with checkpoints 2, 3, 4.  Prints first what needs no
// device (min_samples above spp and a negative threshold are refused), then every pixel's sample count, colour and noise by bits
// and the counters, so tests/test_cpp_adaptive.py can compare them with the CPU oracle's frames of 2, 3 and 4 samples.  Without a
// device the adapter's exception is printed and the exit status is 3.
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
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        // (tests/test_cpp_adaptive.py holds the same numbers)
        rtk_render_params fp = A::default_params();
        fp.width = 16; fp.height = 16; fp.spp = 4; fp.max_ray_depth = 3; fp.diffuse_rays = 2;
        const rtk_adaptive_params ap = {2, 1, 0.02f, 0.01f};
        int refused = 0;
        try { (void)accel.render_adaptive(fp, rtk_adaptive_params{5, 1, 0.02f, 0.01f}); } catch (const std::exception &) { refused += 1; }
        try { (void)accel.render_adaptive(fp, rtk_adaptive_params{2, 1, -1.0f, 0.01f}); } catch (const std::exception &) { refused += 1; }
        std::printf("refused %d\n", refused);
        std::fflush(stdout);
        rtk_counters cn{};
        const auto r = accel.render_adaptive(fp, ap, &cn);
        std::printf("shape %zu %zu samples %zu noise %zu\n", r.height, r.width, r.samples.size(), r.noise.size());
        for (std::size_t y = 0; y < r.height; ++y)
            for (std::size_t x = 0; x < r.width; ++x) {
                const std::size_t i = y * r.width + x;
                std::printf("pixel %zu %u %08x %08x %08x %08x\n", i, r.samples[i], bits(r.pixels[y][x].red), bits(r.pixels[y][x].green),
                            bits(r.pixels[y][x].blue), bits(r.noise[i]));
            }
        std::printf("rays %llu primary %llu\n", static_cast<unsigned long long>(cn.rays), static_cast<unsigned long long>(cn.primary));
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
