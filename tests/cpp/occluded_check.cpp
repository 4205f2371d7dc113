// Drives hip_accel::occluded_batch (simd-raytracer_amd/hip_accel.hpp) against the test-only stand-ins for the reference's
// types: a refractive quad at z = -2 in front of an opaque quad at z = -4 that covers x < 0 only.
// Prints one line per query for tests/test_cpp_occluded.py to compare with tests/occlusion_model.py; without a device the
// adapter's exception is printed and the exit status is 3.
#include <cstdio>
#include <exception>
#include <memory>
#include <vector>

#include "hip_accel.hpp"

using F = float;

static mesh_object<F> quad(std::size_t material, std::size_t mesh_idx, F x0, F x1, F z) {
    mesh_object<F> m{};
    m.material_idx = material;
    m.vertices = {{x0, -2.f, z}, {x1, -2.f, z}, {x1, 2.f, z}, {x0, 2.f, z}};
    const std::size_t idx[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (const auto &i : idx) {
        triangle<F> t{};
        t.v0 = m.vertices[i[0]]; t.v1 = m.vertices[i[1]]; t.v2 = m.vertices[i[2]];
        t.normal = {0.f, 0.f, 1.f};
        t.vertex_indices = {i[0], i[1], i[2]};
        t.mesh_idx = mesh_idx;
        m.triangles.push_back(t);
    }
    return m;
}

int main() {
    using A = hip_accel<F, 1e-6f>;
    scene<F> sc{};
    sc.config = {{0.f, 0.f, 0.f}, 16, 16, 64};
    sc.viewpoint = {{0.f, 0.f, 0.f}, {{1, 0, 0, 0, 1, 0, 0, 0, 1}}};
    sc.lights.push_back({{0.f, 0.f, -6.f}, 100.f});
    sc.materials.push_back(refractive_material<F>{1.5f, false});
    sc.materials.push_back(diffuse_material<F>{{1.f, 1.f, 1.f}, false});
    sc.meshes.push_back(quad(0, 0, -2.f, 2.f, -2.f));       // glass, all of x in [-2, 2]
    sc.meshes.push_back(quad(1, 1, -2.f, 0.f, -4.f));       // opaque, x in [-2, 0] only
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        const vec3<F> down{0.f, 0.f, -1.f};
        const std::vector<ray3<F>> rays = {
            ray3<F>({-1.f, 0.5f, 0.f}, down),     // glass, then the opaque quad within max_t        -> occluded
            ray3<F>({1.f, 0.5f, 0.f}, down),      // glass only                                      -> clear
            ray3<F>({-1.f, 0.5f, 0.f}, down),     // max_t ends between the quads                    -> clear
            ray3<F>({-1.f, 0.5f, 0.f}, down),     // max_t ends in front of the glass                -> clear
            ray3<F>({-1.f, 0.5f, 0.f}, down),     // max_t = distance of the glass: the guard ends it -> clear
            ray3<F>({5.f, 0.5f, 0.f}, down),      // past everything                                 -> clear
            ray3<F>({-1.f, 0.5f, -3.f}, down),    // starts between the quads                        -> occluded
            ray3<F>({-1.f, 0.5f, 0.f}, {0.f, 0.f, -2.f}),   // direction of length 2: max_t in units of t -> occluded
        };
        const std::vector<F> max_t = {10.f, 10.f, 3.f, 1.f, 2.f, 10.f, 10.f, 2.5f};
        const F biases[2] = {1e-4f, -1e-4f};      // a negative bias re-hits the glass it just left: the step limit
        for (const F bias : biases) {
            const auto out = accel.occluded_batch(rays, max_t, bias);
            for (std::size_t i = 0; i < rays.size(); ++i)
                std::printf("query bias=%.9g o=(%.9g,%.9g,%.9g) d=(%.9g,%.9g,%.9g) max_t=%.9g answer=%u\n", bias, rays[i].origin.x,
                            rays[i].origin.y, rays[i].origin.z, rays[i].direction.x, rays[i].direction.y, rays[i].direction.z,
                            max_t[i], (unsigned)out[i]);
        }
        std::printf("empty %zu\n", accel.occluded_batch({}, {}, 1e-4f).size());
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        return 3;
    }
    return 0;
}
