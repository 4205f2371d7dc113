// hip_accel.hpp — header-only adapter that models the reference's `accelerator` concept
// (render/accel/accel.hpp:8-12) on top of the rtk C-ABI (include/rtk.h).
//
// Drop it next to the reference's headers and change ONE line of src/main.cpp:
//     using A = kd_tree_simd_accel<F, static_cast<F>(epsilon)>;      // src/main.cpp:37
// to  using A = hip_accel<F, static_cast<F>(epsilon)>;
// Everything the reference's callers need is here: a constructor from std::shared_ptr<const scene<F>>
// (src/main.cpp:41, kd_tree_simd.hpp:100), the public `scene_ptr` member that render_frame / color_hit /
// is_occluded dereference (render/render.hpp:21,113,136), and
//     template <bool cull> std::optional<hit<F>> intersect(const ray3<F>&) const noexcept;
// `intersect` is one synchronous one-ray launch (correct, slow — it exists so the reference's own CPU
// render_frame can drive the GPU tree ray by ray).  The fast paths are `intersect_batch` (one ray per lane)
// and `render_frame` (the whole render loop device-side, replacing render/render.hpp:18-108).
#pragma once

#include <cstdio>
#include <exception>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <span>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <variant>
#include <vector>

#include <raytracer/core/math/ray3.hpp>
#include <raytracer/render/hit.hpp>
#include <raytracer/scene/scene.hpp>

#include "rtk.h"

template <typename F, F eps, std::size_t max_depth = 8, std::size_t max_leaf_size = 64>
struct hip_accel {
    static_assert(std::is_same_v<F, float>, "the rtk engine computes in float (the reference instantiates F = float, src/main.cpp:36)");

    std::shared_ptr<const scene<F>> scene_ptr;

    explicit hip_accel(std::shared_ptr<const scene<F>> scene_ptr_, bool normalize_hit_normal = true, int device = -1)
        : scene_ptr(std::move(scene_ptr_)) {
        const scene<F> &sc = *scene_ptr;
        // flatten scene<F> exactly as parse_scene_file laid it out (io/json/loader.hpp:235-265)
        std::vector<int32_t> mesh_material, mesh_nverts, mesh_ntris, mat_kind, mat_smooth, mat_texture, mesh_has_uvs, tex_kind;
        std::vector<float> vertices, mat_albedo, mat_ior, light_pos, light_intensity, uvs, tex_a, tex_b, tex_param;
        std::vector<uint32_t> indices;
        std::vector<uint8_t> tex_pixels;                  // bitmap_texture::texture back as the bytes stbi_load gave (bitmap.hpp:26-28)
        std::vector<int32_t> tex_bitmap;                  // [n_textures][3] byte offset, width, height
        // scene.textures is keyed by name (scene/scene.hpp:18); the C-ABI refers to textures by index
        std::vector<std::string> texture_names;
        for (const auto &[name, tv] : sc.textures) {
            const int32_t first_byte = static_cast<int32_t>(tex_pixels.size());
            const rtk_texture t = to_texture(tv, tex_pixels);
            const int32_t bmp[3] = {t.kind == RTK_TEX_BITMAP ? first_byte : 0, t.width, t.height};
            tex_bitmap.insert(tex_bitmap.end(), bmp, bmp + 3);
            texture_names.push_back(name);
            tex_kind.push_back(t.kind); tex_param.push_back(t.param);
            tex_a.insert(tex_a.end(), t.color_a, t.color_a + 3); tex_b.insert(tex_b.end(), t.color_b, t.color_b + 3);
        }
        for (const auto &mesh : sc.meshes) {
            mesh_material.push_back(static_cast<int32_t>(mesh.material_idx));
            mesh_nverts.push_back(static_cast<int32_t>(mesh.vertices.size()));
            mesh_ntris.push_back(static_cast<int32_t>(mesh.triangles.size()));
            for (const auto &v : mesh.vertices) { vertices.push_back(v.x); vertices.push_back(v.y); vertices.push_back(v.z); }
            const bool has_uvs = mesh.uvs.size() >= mesh.vertices.size() && !mesh.uvs.empty();
            mesh_has_uvs.push_back(has_uvs ? 1 : 0);
            if (has_uvs) for (std::size_t i = 0; i < mesh.vertices.size(); ++i) { uvs.push_back(mesh.uvs[i].x); uvs.push_back(mesh.uvs[i].y); }
            for (const auto &t : mesh.triangles)
                for (int k = 0; k < 3; ++k) indices.push_back(static_cast<uint32_t>(t.vertex_indices[k]));
            first_triangle_.push_back(n_triangles_);
            n_triangles_ += mesh.triangles.size();
        }
        for (const auto &mv : sc.materials) {
            float albedo[3] = {0.f, 0.f, 0.f};
            float ior = 1.f;
            int kind = RTK_MAT_DIFFUSE, smooth = 0, texture = -1;
            std::visit([&](const auto &m) {
                using M = std::decay_t<decltype(m)>;
                smooth = m.smooth_shading ? 1 : 0;
                if constexpr (std::is_same_v<M, diffuse_material<F>>) kind = RTK_MAT_DIFFUSE;
                else if constexpr (std::is_same_v<M, reflective_material<F>>) kind = RTK_MAT_REFLECTIVE;
                else if constexpr (std::is_same_v<M, refractive_material<F>>) { kind = RTK_MAT_REFRACTIVE; ior = m.ior; }
                else if constexpr (std::is_same_v<M, constant_material<F>>) kind = RTK_MAT_CONSTANT;
                else {                                    // texture_material (scene/material/texture.hpp)
                    kind = RTK_MAT_TEXTURE;
                    for (std::size_t ti = 0; ti < texture_names.size(); ++ti) if (texture_names[ti] == m.texture) texture = static_cast<int>(ti);
                    if (texture < 0) throw std::invalid_argument("hip_accel: material uses unknown texture '" + m.texture + "'");
                }
                if constexpr (requires { m.albedo; }) { albedo[0] = m.albedo.red; albedo[1] = m.albedo.green; albedo[2] = m.albedo.blue; }
            }, mv);
            mat_kind.push_back(kind); mat_smooth.push_back(smooth); mat_ior.push_back(ior); mat_texture.push_back(texture);
            mat_albedo.insert(mat_albedo.end(), albedo, albedo + 3);
        }
        for (const auto &l : sc.lights) {
            light_pos.push_back(l.position.x); light_pos.push_back(l.position.y); light_pos.push_back(l.position.z);
            light_intensity.push_back(l.intensity);
        }
        rtk_scene_desc d{};
        d.n_meshes = static_cast<int32_t>(mesh_material.size());
        d.mesh_material = mesh_material.data(); d.mesh_nverts = mesh_nverts.data(); d.mesh_ntris = mesh_ntris.data();
        d.vertices = vertices.data(); d.indices = indices.data();
        d.n_materials = static_cast<int32_t>(mat_kind.size());
        d.mat_kind = mat_kind.data(); d.mat_albedo = mat_albedo.data(); d.mat_ior = mat_ior.data(); d.mat_smooth = mat_smooth.data();
        d.mat_texture = mat_texture.data(); d.uvs = uvs.data(); d.mesh_has_uvs = mesh_has_uvs.data();
        d.n_textures = static_cast<int32_t>(tex_kind.size());
        d.tex_kind = tex_kind.data(); d.tex_color_a = tex_a.data(); d.tex_color_b = tex_b.data(); d.tex_param = tex_param.data();
        d.tex_pixels = tex_pixels.data(); d.tex_bitmap = tex_bitmap.data();
        d.n_lights = static_cast<int32_t>(light_intensity.size());
        d.light_pos = light_pos.data(); d.light_intensity = light_intensity.data();
        d.cam_pos[0] = sc.viewpoint.position.x; d.cam_pos[1] = sc.viewpoint.position.y; d.cam_pos[2] = sc.viewpoint.position.z;
        for (int i = 0; i < 9; ++i) d.cam_mat[i] = sc.viewpoint.matrix.m[static_cast<std::size_t>(i)];
        d.background[0] = sc.config.background_color.red; d.background[1] = sc.config.background_color.green;
        d.background[2] = sc.config.background_color.blue;
        d.width = static_cast<int32_t>(sc.config.image_width); d.height = static_cast<int32_t>(sc.config.image_height);
        d.bucket_size = static_cast<int32_t>(sc.config.bucket_size);

        rtk_scene *rs = nullptr;
        check(rtk_scene_create(&d, &rs));
        rtk_accel_params ap{};
        ap.max_depth = static_cast<int32_t>(max_depth); ap.max_leaf_size = static_cast<int32_t>(max_leaf_size);
        ap.eps = eps; ap.normalize_hit_normal = normalize_hit_normal ? 1 : 0; ap.device = device;
        rtk_accel *ra = nullptr;
        const int rc = rtk_accel_build(rs, &ap, &ra);
        rtk_scene_destroy(rs);                       // the accel keeps its own copy (as kd_tree_simd.hpp:106-107 does)
        check(rc);
        accel_ = std::shared_ptr<rtk_accel>(ra, rtk_accel_destroy);
        texture_names_ = std::move(texture_names);
    }

    // accel.template intersect<cull>(ray) — render/accel/accel.hpp:9-10
    template <bool backface_culling>
    [[nodiscard]] std::optional<hit<F>> intersect(const ray3<F> &ray) const noexcept {
        rtk_ray r{{ray.origin.x, ray.origin.y, ray.origin.z}, {ray.direction.x, ray.direction.y, ray.direction.z}};
        rtk_hit h{};
        // intersect is noexcept in the reference (kd_tree_simd.hpp:188) and has no error channel: a device failure must not be
        // read as "the ray missed" (a silently black frame), so it ends the program with the library's message.
        if (rtk_accel_intersect(accel_.get(), &r, 1, backface_culling ? 1 : 0, RTK_TRACE_AUTO, &h) != RTK_OK) {
            std::fprintf(stderr, "hip_accel::intersect: %s\n", rtk_last_error());
            std::terminate();
        }
        return to_hit(ray, h);
    }

    // one ray per lane; out[i] corresponds to rays[i]
    template <bool backface_culling>
    [[nodiscard]] std::vector<std::optional<hit<F>>> intersect_batch(const std::vector<ray3<F>> &rays) const {
        std::vector<rtk_ray> in(rays.size());
        for (std::size_t i = 0; i < rays.size(); ++i)
            in[i] = rtk_ray{{rays[i].origin.x, rays[i].origin.y, rays[i].origin.z},
                            {rays[i].direction.x, rays[i].direction.y, rays[i].direction.z}};
        std::vector<rtk_hit> out(rays.size());
        check(rtk_accel_intersect(accel_.get(), in.data(), in.size(), backface_culling ? 1 : 0, RTK_TRACE_AUTO, out.data()));
        std::vector<std::optional<hit<F>>> res(rays.size());
        for (std::size_t i = 0; i < rays.size(); ++i) res[i] = to_hit(rays[i], out[i]);
        return res;
    }

    // is_occluded(accel, rays[i], max_t[i]) (render/render.hpp:110-131) for a batch, one query per lane: RTK_OCC_CLEAR,
    // RTK_OCC_OCCLUDED, or RTK_OCC_STEP_LIMIT for a query the reference would still be stepping after RTK_OCCLUDED_MAX_STEPS hits
    [[nodiscard]] std::vector<std::uint8_t> occluded_batch(const std::vector<ray3<F>> &rays, const std::vector<F> &max_t, F shadow_bias) const {
        if (max_t.size() != rays.size()) throw std::invalid_argument("hip_accel::occluded_batch: one max_t per ray");
        std::vector<rtk_ray> in(rays.size());
        for (std::size_t i = 0; i < rays.size(); ++i)
            in[i] = rtk_ray{{rays[i].origin.x, rays[i].origin.y, rays[i].origin.z},
                            {rays[i].direction.x, rays[i].direction.y, rays[i].direction.z}};
        std::vector<std::uint8_t> out(rays.size());
        check(rtk_accel_occluded(accel_.get(), in.data(), max_t.data(), in.size(), shadow_bias, RTK_TRACE_AUTO, out.data(), nullptr));
        return out;
    }

    // `intersect<cull>(rays[i])` followed by color_hit(accel, hit, 0), or the background colour on a miss (render/render.hpp:64-69,
    // 133-308), for a batch: the colour every ray sees, out[i] for rays[i].  ids (empty, or one per ray): the pixel index of each
    // ray's RNG root key (diffuse GI only; empty = the ray's index).  params: default_radiance_params()
    [[nodiscard]] std::vector<color<F>> radiance_batch(const std::vector<ray3<F>> &rays, const rtk_radiance_params &params,
                                                       const std::vector<std::uint32_t> &ids = {}, rtk_counters *counters = nullptr) const {
        if (!ids.empty() && ids.size() != rays.size()) throw std::invalid_argument("hip_accel::radiance_batch: one id per ray");
        std::vector<rtk_ray> in(rays.size());
        for (std::size_t i = 0; i < rays.size(); ++i)
            in[i] = rtk_ray{{rays[i].origin.x, rays[i].origin.y, rays[i].origin.z},
                            {rays[i].direction.x, rays[i].direction.y, rays[i].direction.z}};
        std::vector<float> rgb(rays.size() * 3);
        check(rtk_accel_radiance(accel_.get(), in.data(), ids.empty() ? nullptr : ids.data(), in.size(), &params, rgb.data(), counters));
        std::vector<color<F>> out(rays.size());
        for (std::size_t i = 0; i < rays.size(); ++i) out[i] = color<F>{rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]};
        return out;
    }

    // The accel after the scene's vertex positions changed: what constructing a new accel from the moved scene would hold, rebuilt
    // on the device (rtk_accel_update_vertices).  `vertices`: all meshes concatenated in mesh order, as many as the scene has.
    // CAUTION: this overload moves the ACCEL ONLY.  *scene_ptr stays the old scene, and intersect / intersect_batch fill
    // hit.face_normal and hit.uvs from it (to_hit): distances, u, v, hit_normal and mesh_idx are the moved scene's, face_normal is
    // the OLD triangle's.  It is meant for callers that use render_frame / radiance_batch / occluded_batch or never read
    // face_normal; everyone else moves a copy of the scene and calls update_vertices(moved_scene) below, which swaps scene_ptr.
    void update_vertices(const std::vector<vec3<F>> &vertices) {
        std::size_t n = 0;
        for (const auto &mesh : scene_ptr->meshes) n += mesh.vertices.size();
        if (vertices.size() != n) throw std::invalid_argument("hip_accel::update_vertices: one position per vertex of the scene");
        std::vector<float> flat;
        flat.reserve(n * 3 + 3);
        for (const auto &v : vertices) { flat.push_back(v.x); flat.push_back(v.y); flat.push_back(v.z); }
        if (flat.empty()) flat.push_back(0.f);            // (an empty scene still hands over a pointer)
        check(rtk_accel_update_vertices(accel_.get(), flat.data()));
    }

    // The same from a moved copy of the scene (same meshes, same triangles, other vertex positions); scene_ptr then points to it.
    void update_vertices(std::shared_ptr<const scene<F>> moved) {
        if (!moved || moved->meshes.size() != scene_ptr->meshes.size()) throw std::invalid_argument("hip_accel::update_vertices: another topology");
        std::vector<vec3<F>> vertices;
        for (std::size_t m = 0; m < moved->meshes.size(); ++m) {
            if (moved->meshes[m].vertices.size() != scene_ptr->meshes[m].vertices.size() ||
                moved->meshes[m].triangles.size() != scene_ptr->meshes[m].triangles.size())
                throw std::invalid_argument("hip_accel::update_vertices: another topology");
            vertices.insert(vertices.end(), moved->meshes[m].vertices.begin(), moved->meshes[m].vertices.end());
        }
        update_vertices(vertices);
        scene_ptr = std::move(moved);
    }

    // The accel after the scene's meshes got other TRIANGLES as well (rtk_accel_update_geometry): `changed` has the same meshes with
    // the same number of vertices each (positions may differ) and any triangle lists over them -- fewer, more, none.  Materials,
    // uvs, lights and camera are taken to be the old ones.  scene_ptr then points to it, so hits carry its triangles.
    void update_geometry(std::shared_ptr<const scene<F>> changed) {
        if (!changed || changed->meshes.size() != scene_ptr->meshes.size()) throw std::invalid_argument("hip_accel::update_geometry: other meshes");
        std::vector<float> vertices;
        std::vector<uint32_t> indices;
        std::vector<int32_t> mesh_ntris;
        std::vector<std::size_t> first;
        std::size_t total = 0;
        for (std::size_t m = 0; m < changed->meshes.size(); ++m) {
            const auto &mesh = changed->meshes[m];
            if (mesh.vertices.size() != scene_ptr->meshes[m].vertices.size())
                throw std::invalid_argument("hip_accel::update_geometry: a mesh keeps its number of vertices");
            for (const auto &v : mesh.vertices) { vertices.push_back(v.x); vertices.push_back(v.y); vertices.push_back(v.z); }
            for (const auto &t : mesh.triangles)
                for (int k = 0; k < 3; ++k) indices.push_back(static_cast<uint32_t>(t.vertex_indices[k]));
            mesh_ntris.push_back(static_cast<int32_t>(mesh.triangles.size()));
            first.push_back(total);
            total += mesh.triangles.size();
        }
        if (vertices.empty()) vertices.push_back(0.f);    // (an empty scene still hands over a pointer)
        if (mesh_ntris.empty()) mesh_ntris.push_back(0);
        check(rtk_accel_update_geometry(accel_.get(), vertices.data(), indices.empty() ? nullptr : indices.data(), mesh_ntris.data()));
        first_triangle_ = std::move(first);
        n_triangles_ = total;
        scene_ptr = std::move(changed);
    }

    // The camera of later frames (rtk_accel_set_camera): what constructing a new accel from the scene with this viewpoint would
    // render.  Moves the ACCEL ONLY: scene_ptr->viewpoint stays (the scene is const); camera_now() reads the accel's back.
    void set_camera(const camera<F> &c) {
        const rtk_view v = to_view(c);
        check(rtk_accel_set_camera(accel_.get(), &v));
    }
    [[nodiscard]] camera<F> camera_now() const {
        rtk_view v{};
        check(rtk_accel_get_camera(accel_.get(), &v));
        camera<F> c{};
        c.position = vec3<F>{v.position[0], v.position[1], v.position[2]};
        for (std::size_t i = 0; i < 9; ++i) c.matrix.m[i] = v.matrix[i];
        return c;
    }

    // Lights, materials and background of later frames (rtk_accel_set_lights / _set_materials / _set_background): what constructing
    // a new accel from the scene with these would render.  Like set_camera they move the ACCEL ONLY (the scene is const); the
    // *_now() members read the accel's back.  The number of lights is free; materials are one per material of the scene, and a
    // texture_material names one of the scene's textures.
    void set_lights(std::span<const light<F>> lights) {
        std::vector<rtk_light> in(lights.size());
        for (std::size_t i = 0; i < lights.size(); ++i)
            in[i] = rtk_light{{lights[i].position.x, lights[i].position.y, lights[i].position.z}, lights[i].intensity};
        check(rtk_accel_set_lights(accel_.get(), in.empty() ? nullptr : in.data(), static_cast<int32_t>(in.size())));
    }
    [[nodiscard]] std::vector<light<F>> lights_now() const {
        int32_t n = 0;
        check(rtk_accel_get_lights(accel_.get(), nullptr, 0, &n));
        std::vector<rtk_light> in(static_cast<std::size_t>(n) + 1);
        check(rtk_accel_get_lights(accel_.get(), in.data(), n, &n));
        std::vector<light<F>> out(static_cast<std::size_t>(n));
        for (std::size_t i = 0; i < out.size(); ++i)
            out[i] = light<F>{vec3<F>{in[i].position[0], in[i].position[1], in[i].position[2]}, in[i].intensity};
        return out;
    }

    void set_materials(std::span<const material_variant<F>> materials) {
        if (materials.size() != scene_ptr->materials.size()) throw std::invalid_argument("hip_accel::set_materials: one material per material of the scene");
        std::vector<rtk_material> in(materials.size() + 1);
        for (std::size_t i = 0; i < materials.size(); ++i) in[i] = to_material(materials[i]);
        check(rtk_accel_set_materials(accel_.get(), in.data(), static_cast<int32_t>(materials.size())));
    }
    [[nodiscard]] std::vector<material_variant<F>> materials_now() const {
        std::vector<rtk_material> in(scene_ptr->materials.size() + 1);
        check(rtk_accel_get_materials(accel_.get(), in.data()));
        std::vector<material_variant<F>> out;
        for (std::size_t i = 0; i + 1 < in.size(); ++i) {
            const rtk_material &m = in[i];
            const color<F> albedo{m.albedo[0], m.albedo[1], m.albedo[2]};
            const bool smooth = m.smooth != 0;
            switch (m.kind) {
                case RTK_MAT_REFLECTIVE: out.emplace_back(reflective_material<F>{albedo, smooth}); break;
                case RTK_MAT_REFRACTIVE: out.emplace_back(refractive_material<F>{m.ior, smooth}); break;
                case RTK_MAT_CONSTANT: out.emplace_back(constant_material<F>{albedo, smooth}); break;
                case RTK_MAT_TEXTURE: out.emplace_back(texture_material<F>{texture_names_.at(static_cast<std::size_t>(m.texture)), smooth}); break;
                default: out.emplace_back(diffuse_material<F>{albedo, smooth}); break;
            }
        }
        return out;
    }

    void set_background(const color<F> &c) {
        const float rgb[3] = {c.red, c.green, c.blue};
        check(rtk_accel_set_background(accel_.get(), rgb));
    }
    [[nodiscard]] color<F> background_now() const {
        float rgb[3] = {0.f, 0.f, 0.f};
        check(rtk_accel_get_background(accel_.get(), rgb));
        return color<F>{rgb[0], rgb[1], rgb[2]};
    }

    // Textures and uvs of later frames (rtk_accel_set_textures / _set_texture_pixels / _set_uvs), in the same way: the accel moves,
    // the scene is const.  set_textures replaces the whole table, by name and in the caller's order (a texture_material handed to a
    // later set_materials names one of THESE); a table that drops a texture some live material uses is refused.  A bitmap comes
    // back as its image<F>: bitmap_texture can only be made from a file (scene/texture/bitmap.hpp:43).
    using named_texture = std::pair<std::string, texture_variant<F>>;
    using texture_now = std::variant<albedo_texture<F>, edge_texture<F>, checker_texture<F>, image<F>>;
    void set_textures(std::span<const named_texture> textures) {
        std::vector<rtk_texture> in(textures.size() + 1);
        std::vector<std::vector<uint8_t>> texels(textures.size());
        std::vector<const uint8_t *> pixels(textures.size() + 1, nullptr);
        std::vector<std::string> names;
        for (std::size_t i = 0; i < textures.size(); ++i) {
            in[i] = to_texture(textures[i].second, texels[i]);
            pixels[i] = texels[i].data();
            names.push_back(textures[i].first);
        }
        check(rtk_accel_set_textures(accel_.get(), in.data(), static_cast<int32_t>(textures.size()), pixels.data()));
        texture_names_ = std::move(names);
    }
    [[nodiscard]] std::vector<std::pair<std::string, texture_now>> textures_now() const {
        int32_t n = 0;
        check(rtk_accel_get_textures(accel_.get(), nullptr, 0, &n));
        std::vector<rtk_texture> in(static_cast<std::size_t>(n) + 1);
        check(rtk_accel_get_textures(accel_.get(), in.data(), n, &n));
        std::vector<std::pair<std::string, texture_now>> out;
        for (std::size_t i = 0; i < static_cast<std::size_t>(n); ++i) {
            const rtk_texture &t = in[i];
            const color<F> a{t.color_a[0], t.color_a[1], t.color_a[2]}, b{t.color_b[0], t.color_b[1], t.color_b[2]};
            const std::string &name = texture_names_.at(i);
            if (t.kind == RTK_TEX_EDGES) out.emplace_back(name, edge_texture<F>{a, b, t.param});
            else if (t.kind == RTK_TEX_CHECKER) out.emplace_back(name, checker_texture<F>{a, b, t.param});
            else if (t.kind == RTK_TEX_BITMAP) {
                const std::size_t w = static_cast<std::size_t>(t.width), h = static_cast<std::size_t>(t.height);
                std::vector<uint8_t> bytes(w * h * 3);
                std::size_t got = 0;
                check(rtk_accel_get_texture_pixels(accel_.get(), static_cast<int32_t>(i), bytes.data(), bytes.size(), &got));
                const F color_scale = F(1.0 / 255.0);                             // bitmap.hpp:19
                std::vector<std::vector<color<F>>> px(h, std::vector<color<F>>(w));
                for (std::size_t r = 0; r < h; ++r) for (std::size_t c = 0; c < w; ++c) {
                    const uint8_t *p = bytes.data() + (r * w + c) * 3;
                    px[r][c] = color<F>{static_cast<F>(p[0]) * color_scale, static_cast<F>(p[1]) * color_scale, static_cast<F>(p[2]) * color_scale};
                }
                out.emplace_back(name, image<F>(h, w, std::move(px)));
            } else out.emplace_back(name, albedo_texture<F>{a});
        }
        return out;
    }
    // new texels for the bitmap texture `name`; the size may differ from before
    void set_texture_pixels(const std::string &name, const image<F> &im) {
        std::vector<uint8_t> texels;
        int32_t w = 0, h = 0;
        to_texels(im, w, h, texels);
        texels.push_back(0);                                                      // (a valid pointer for an empty image: the library judges the size)
        check(rtk_accel_set_texture_pixels(accel_.get(), static_cast<int32_t>(texture_index(name, "hip_accel::set_texture_pixels")), w, h, texels.data()));
    }
    // one uv per vertex, all meshes' vertices one behind the other (a mesh without uvs has zeros, loader.hpp:199-207)
    void set_uvs(std::span<const vec2<F>> uvs) {
        std::size_t nv = 0;
        for (const auto &mesh : scene_ptr->meshes) nv += mesh.vertices.size();
        if (uvs.size() != nv) throw std::invalid_argument("hip_accel::set_uvs: one uv per vertex of the scene");
        std::vector<float> flat;
        flat.reserve(nv * 2 + 2);
        for (const auto &uv : uvs) { flat.push_back(uv.x); flat.push_back(uv.y); }
        flat.push_back(0.f);
        check(rtk_accel_set_uvs(accel_.get(), flat.data()));
    }
    [[nodiscard]] std::vector<vec2<F>> uvs_now() const {
        std::size_t nv = 0;
        for (const auto &mesh : scene_ptr->meshes) nv += mesh.vertices.size();
        std::vector<float> flat(nv * 2 + 2);
        check(rtk_accel_get_uvs(accel_.get(), flat.data()));
        std::vector<vec2<F>> out(nv);
        for (std::size_t i = 0; i < nv; ++i) out[i] = vec2<F>{flat[i * 2], flat[i * 2 + 1]};
        return out;
    }

    // One whole frame per camera from one call (rtk_render_views): image v is what set_camera(views[v]) + render_frame(params)
    // gives, and the accel's own camera stays.  counters: totals over the views.
    [[nodiscard]] std::vector<std::vector<std::vector<color<F>>>> render_views(std::span<const camera<F>> views, const rtk_render_params &params,
                                                                              rtk_counters *counters = nullptr) const {
        if (params.sample_begin != 0 || (params.sample_count != 0 && params.sample_count != params.spp))
            throw std::invalid_argument("hip_accel::render_views renders whole frames (sample_begin = 0, all spp samples)");
        std::size_t n = 0;
        check(rtk_render_output_floats(accel_.get(), &params, &n));
        std::vector<rtk_view> in(views.size());
        for (std::size_t v = 0; v < views.size(); ++v) in[v] = to_view(views[v]);
        std::vector<float> rgb(n * views.size() + 1);
        check(rtk_render_views(accel_.get(), &params, in.empty() ? nullptr : in.data(), static_cast<int32_t>(views.size()), rgb.data(), counters));
        const std::size_t w = params.width > 0 ? static_cast<std::size_t>(params.width) : scene_ptr->config.image_width;
        const std::size_t h = n / 3 / w;
        std::vector<std::vector<std::vector<color<F>>>> out(views.size(), std::vector<std::vector<color<F>>>(h, std::vector<color<F>>(w)));
        for (std::size_t v = 0; v < views.size(); ++v)
            for (std::size_t y = 0; y < h; ++y)
                for (std::size_t x = 0; x < w; ++x) {
                    const float *px = rgb.data() + v * n + (y * w + x) * 3;
                    out[v][y][x] = color<F>{px[0], px[1], px[2]};
                }
        return out;
    }

    // What the camera rays hit, as planes (rtk_render_gbuffer): hit<F> of intersect<true>(camera ray of `sample`) for every pixel of
    // every view, field by field.  `planes`: the gbuffer_* bits wanted; a plane that is not wanted stays empty.  Every plane is
    // [views][height][width] flattened (x fastest), position / normal / albedo with 3 and bary with 2 floats per pixel.  No views =
    // the accel's own camera (one view).  A miss: depth -1, ids 0xFFFFFFFF, albedo the background, zeros elsewhere.
    enum : unsigned {
        gbuffer_depth = 1u, gbuffer_position = 2u, gbuffer_normal = 4u, gbuffer_albedo = 8u, gbuffer_bary = 16u, gbuffer_tri = 32u,
        gbuffer_mesh = 64u, gbuffer_material = 128u, gbuffer_all = 255u
    };
    struct gbuffer_result {
        std::size_t views = 0, width = 0, height = 0;
        std::vector<float> depth, position, normal, albedo, bary;
        std::vector<std::uint32_t> tri, mesh, material;
    };
    [[nodiscard]] gbuffer_result render_gbuffer(const rtk_render_params &params, std::int32_t sample, std::span<const camera<F>> views,
                                                unsigned planes = gbuffer_all) const {
        std::size_t n = 0;
        check(rtk_render_output_floats(accel_.get(), &params, &n));
        gbuffer_result r;
        r.views = views.empty() ? 1 : views.size();
        r.width = params.width > 0 ? static_cast<std::size_t>(params.width) : scene_ptr->config.image_width;
        r.height = n / 3 / r.width;
        const std::size_t pixels = r.views * r.width * r.height;
        rtk_gbuffer out{};
        const auto want = [&](unsigned bit, auto &plane, std::size_t comps) {
            if (planes & bit) plane.resize(pixels * comps + 1);              // (+ 1: a valid pointer for a call without pixels)
            return (planes & bit) ? plane.data() : nullptr;
        };
        out.depth = want(gbuffer_depth, r.depth, 1); out.position = want(gbuffer_position, r.position, 3);
        out.normal = want(gbuffer_normal, r.normal, 3); out.albedo = want(gbuffer_albedo, r.albedo, 3); out.bary = want(gbuffer_bary, r.bary, 2);
        out.tri = want(gbuffer_tri, r.tri, 1); out.mesh = want(gbuffer_mesh, r.mesh, 1); out.material = want(gbuffer_material, r.material, 1);
        std::vector<rtk_view> in(views.size());
        for (std::size_t v = 0; v < views.size(); ++v) in[v] = to_view(views[v]);
        check(rtk_render_gbuffer(accel_.get(), &params, sample, in.empty() ? nullptr : in.data(), static_cast<std::int32_t>(r.views), &out));
        const auto trim = [&](auto &plane, std::size_t comps) { if (!plane.empty()) plane.resize(pixels * comps); };
        trim(r.depth, 1); trim(r.position, 3); trim(r.normal, 3); trim(r.albedo, 3); trim(r.bary, 2); trim(r.tri, 1); trim(r.mesh, 1); trim(r.material, 1);
        return r;
    }

    // The first surface that is shaded behind mirrors and glass, as planes (rtk_render_gbuffer_specular): the end of every camera
    // ray's specular chain under params.max_ray_depth and its biases.  depth, position and normal place the end hit in the virtual
    // world behind the mirrors; surface_position, surface_normal, albedo, bary and the ids are the end hit's own; bounces the
    // secondary rays traced; last_ray (6 floats per pixel) the ray that found it.  Planes, views and layout as render_gbuffer.
    enum : unsigned {
        specular_depth = 1u, specular_position = 2u, specular_normal = 4u, specular_surface_position = 8u, specular_surface_normal = 16u,
        specular_albedo = 32u, specular_bary = 64u, specular_tri = 128u, specular_mesh = 256u, specular_material = 512u,
        specular_bounces = 1024u, specular_last_ray = 2048u, specular_all = 4095u
    };
    struct gbuffer_specular_result {
        std::size_t views = 0, width = 0, height = 0;
        std::vector<float> depth, position, normal, surface_position, surface_normal, albedo, bary, last_ray;
        std::vector<std::uint32_t> tri, mesh, material, bounces;
    };
    [[nodiscard]] gbuffer_specular_result render_gbuffer_specular(const rtk_render_params &params, std::int32_t sample,
                                                                  std::span<const camera<F>> views, unsigned planes = specular_all) const {
        std::size_t n = 0;
        check(rtk_render_output_floats(accel_.get(), &params, &n));
        gbuffer_specular_result r;
        r.views = views.empty() ? 1 : views.size();
        r.width = params.width > 0 ? static_cast<std::size_t>(params.width) : scene_ptr->config.image_width;
        r.height = n / 3 / r.width;
        const std::size_t pixels = r.views * r.width * r.height;
        rtk_gbuffer_specular out{};
        const auto want = [&](unsigned bit, auto &plane, std::size_t comps) {
            if (planes & bit) plane.resize(pixels * comps + 1);              // (+ 1: a valid pointer for a call without pixels)
            return (planes & bit) ? plane.data() : nullptr;
        };
        out.depth = want(specular_depth, r.depth, 1); out.position = want(specular_position, r.position, 3);
        out.normal = want(specular_normal, r.normal, 3); out.surface_position = want(specular_surface_position, r.surface_position, 3);
        out.surface_normal = want(specular_surface_normal, r.surface_normal, 3); out.albedo = want(specular_albedo, r.albedo, 3);
        out.bary = want(specular_bary, r.bary, 2); out.tri = want(specular_tri, r.tri, 1); out.mesh = want(specular_mesh, r.mesh, 1);
        out.material = want(specular_material, r.material, 1); out.bounces = want(specular_bounces, r.bounces, 1);
        out.last_ray = want(specular_last_ray, r.last_ray, 6);
        std::vector<rtk_view> in(views.size());
        for (std::size_t v = 0; v < views.size(); ++v) in[v] = to_view(views[v]);
        check(rtk_render_gbuffer_specular(accel_.get(), &params, sample, in.empty() ? nullptr : in.data(), static_cast<std::int32_t>(r.views), &out));
        const auto trim = [&](auto &plane, std::size_t comps) { if (!plane.empty()) plane.resize(pixels * comps); };
        trim(r.depth, 1); trim(r.position, 3); trim(r.normal, 3); trim(r.surface_position, 3); trim(r.surface_normal, 3); trim(r.albedo, 3);
        trim(r.bary, 2); trim(r.tri, 1); trim(r.mesh, 1); trim(r.material, 1); trim(r.bounces, 1); trim(r.last_ray, 6);
        return r;
    }

    // Where each pixel's surface point was in the previous pose (rtk_render_motion): from ONE view of a render_gbuffer result with
    // its tri and bary planes, the vertices of the previous pose (all meshes concatenated in mesh order, as update_vertices takes
    // them) and, for `motion`, the previous camera.  prev_position [h][w] x 3 floats (0 on a miss) is what rtk_temporal_accumulate
    // takes as the new frame's position after an update; motion [h][w] x 2 floats is previous place minus present place in pixels
    // (both words 0x7FC00000 where there is none).  Without a previous camera motion stays empty.
    struct motion_result {
        std::size_t width = 0, height = 0;
        std::vector<float> prev_position, motion;
    };
    [[nodiscard]] motion_result render_motion(const gbuffer_result &g, std::size_t view, const std::vector<vec3<F>> &prev_vertices,
                                              double fov_degrees, const camera<F> *prev_camera = nullptr) const {
        const std::size_t pixels = g.width * g.height;
        if (view >= g.views || g.tri.size() < (view + 1) * pixels || g.bary.size() < (view + 1) * pixels * 2)
            throw std::invalid_argument("hip_accel::render_motion: the g-buffer has no tri and bary planes of that view");
        std::size_t n = 0;
        for (const auto &mesh : scene_ptr->meshes) n += mesh.vertices.size();
        if (prev_vertices.size() != n) throw std::invalid_argument("hip_accel::render_motion: one position per vertex of the scene");
        std::vector<float> flat;
        flat.reserve(n * 3 + 3);
        for (const auto &v : prev_vertices) { flat.push_back(v.x); flat.push_back(v.y); flat.push_back(v.z); }
        flat.resize(n * 3 + 3);                                              // (a valid pointer for a scene without vertices)
        motion_result r;
        r.width = g.width; r.height = g.height;
        r.prev_position.resize(pixels * 3 + 1);
        if (prev_camera) r.motion.resize(pixels * 2 + 1);
        const rtk_motion_params p{static_cast<std::int32_t>(g.width), static_cast<std::int32_t>(g.height), fov_degrees};
        const rtk_motion_outputs out{r.prev_position.data(), prev_camera ? r.motion.data() : nullptr};
        rtk_view pv{};
        if (prev_camera) pv = to_view(*prev_camera);
        check(rtk_render_motion(accel_.get(), &p, g.tri.data() + view * pixels, g.bary.data() + view * pixels * 2, flat.data(),
                                prev_camera ? &pv : nullptr, &out));
        r.prev_position.resize(pixels * 3);
        if (prev_camera) r.motion.resize(pixels * 2);
        return r;
    }

    // Rectangles of the frame `params` describes, all in one call (rtk_render_regions).  Tile: anything with x0, y0, x1, y1 --
    // the reference's render_tile (render/tile/tile.hpp), what its single / region / bucket schedulers hand to tile_worker, or
    // rtk_rect.  Every pixel is what render_frame(params) gives there; counters: the call's totals.
    // RTK_REGIONS_PACKED: image r is tile r alone, [y1-y0][x1-x0]; tiles may overlap.
    template <typename Tile>
    [[nodiscard]] std::vector<std::vector<std::vector<color<F>>>> render_regions(std::span<const Tile> tiles, const rtk_render_params &params,
                                                                                rtk_counters *counters = nullptr) const {
        whole_samples(params, "hip_accel::render_regions");
        const std::vector<rtk_rect> in = to_rects(tiles);
        std::size_t total = 0;
        for (const rtk_rect &r : in) total += r.x1 > r.x0 && r.y1 > r.y0 ? static_cast<std::size_t>(r.x1 - r.x0) * static_cast<std::size_t>(r.y1 - r.y0) : 0;
        std::vector<float> rgb(total * 3 + 1);
        check(rtk_render_regions(accel_.get(), &params, in.empty() ? nullptr : in.data(), static_cast<int32_t>(in.size()), RTK_REGIONS_PACKED,
                                 rgb.data(), counters));
        std::vector<std::vector<std::vector<color<F>>>> out(in.size());
        const float *px = rgb.data();
        for (std::size_t r = 0; r < in.size(); ++r) {
            const std::size_t w = static_cast<std::size_t>(in[r].x1 - in[r].x0), h = static_cast<std::size_t>(in[r].y1 - in[r].y0);
            out[r].assign(h, std::vector<color<F>>(w));
            for (std::size_t y = 0; y < h; ++y)
                for (std::size_t x = 0; x < w; ++x, px += 3) out[r][y][x] = color<F>{px[0], px[1], px[2]};
        }
        return out;
    }

    // RTK_REGIONS_IN_FRAME: the tiles' pixels of `image` ([h][w], the frame of `params`) are rendered, every other pixel of it is
    // left as it is.  The tiles must be pairwise disjoint.
    template <typename Tile>
    void render_regions_into(std::vector<std::vector<color<F>>> &image, std::span<const Tile> tiles, const rtk_render_params &params,
                             rtk_counters *counters = nullptr) const {
        whole_samples(params, "hip_accel::render_regions_into");
        std::size_t n = 0;
        check(rtk_render_output_floats(accel_.get(), &params, &n));
        const std::size_t w = params.width > 0 ? static_cast<std::size_t>(params.width) : scene_ptr->config.image_width;
        const std::size_t h = n / 3 / w;
        if (image.size() != h) throw std::invalid_argument("hip_accel::render_regions_into: the image has not the frame's height");
        for (const auto &row : image)
            if (row.size() != w) throw std::invalid_argument("hip_accel::render_regions_into: the image has not the frame's width");
        const std::vector<rtk_rect> in = to_rects(tiles);
        std::vector<float> rgb(n + 1);
        check(rtk_render_regions(accel_.get(), &params, in.empty() ? nullptr : in.data(), static_cast<int32_t>(in.size()), RTK_REGIONS_IN_FRAME,
                                 rgb.data(), counters));
        for (const rtk_rect &r : in)
            for (std::size_t y = static_cast<std::size_t>(r.y0); y < static_cast<std::size_t>(r.y1); ++y)
                for (std::size_t x = static_cast<std::size_t>(r.x0); x < static_cast<std::size_t>(r.x1); ++x) {
                    const float *px = rgb.data() + (y * w + x) * 3;
                    image[y][x] = color<F>{px[0], px[1], px[2]};
                }
    }

    // render_frame<A,F>(accel, BUCKET_TILES) with the whole loop device-side; pixels [h][w] as in image<F>
    [[nodiscard]] std::vector<std::vector<color<F>>> render_frame(const rtk_render_params &params, rtk_counters *counters = nullptr) const {
        // this returns a finished image: a partial pass of a progressive frame (sample_begin / sample_count) needs the running
        // sums of the passes before it, which live in the caller's buffer -- use rtk_render_frame / _device for those
        if (params.sample_begin != 0 || (params.sample_count != 0 && params.sample_count != params.spp))
            throw std::invalid_argument("hip_accel::render_frame renders whole frames (sample_begin = 0, all spp samples)");
        std::size_t n = 0;
        check(rtk_render_output_floats(accel_.get(), &params, &n));
        std::vector<float> rgb(n);
        check(rtk_render_frame(accel_.get(), &params, rgb.data(), counters));
        const std::size_t w = params.width > 0 ? static_cast<std::size_t>(params.width) : scene_ptr->config.image_width;
        const std::size_t h = n / 3 / w;
        std::vector<std::vector<color<F>>> px(h, std::vector<color<F>>(w));
        for (std::size_t y = 0; y < h; ++y)
            for (std::size_t x = 0; x < w; ++x)
                px[y][x] = color<F>{rgb[(y * w + x) * 3], rgb[(y * w + x) * 3 + 1], rgb[(y * w + x) * 3 + 2]};
        return px;
    }

    // A frame whose 8x8 pixel blocks stop taking samples once they have converged (rtk_render_adaptive): params.spp is the
    // ceiling.  pixels [h][w]; samples and noise are [h * w], x fastest.  Every pixel is the pixel of render_frame with
    // spp = samples[pixel], bit for bit; noise is the standard error of the pixel's mean luminance at its final count.
    struct adaptive_result {
        std::size_t width = 0, height = 0;
        std::vector<std::vector<color<F>>> pixels;
        std::vector<std::uint32_t> samples;
        std::vector<float> noise;
    };
    [[nodiscard]] adaptive_result render_adaptive(const rtk_render_params &params, const rtk_adaptive_params &adaptive,
                                                  rtk_counters *counters = nullptr) const {
        std::size_t n = 0;
        check(rtk_render_output_floats(accel_.get(), &params, &n));
        adaptive_result r;
        r.width = params.width > 0 ? static_cast<std::size_t>(params.width) : scene_ptr->config.image_width;
        r.height = n / 3 / r.width;
        std::vector<float> rgb(n);
        r.samples.resize(n / 3);
        r.noise.resize(n / 3);
        check(rtk_render_adaptive(accel_.get(), &params, &adaptive, rgb.data(), r.samples.data(), r.noise.data(), counters));
        r.pixels.assign(r.height, std::vector<color<F>>(r.width));
        for (std::size_t y = 0; y < r.height; ++y)
            for (std::size_t x = 0; x < r.width; ++x) {
                const float *px = rgb.data() + (y * r.width + x) * 3;
                r.pixels[y][x] = color<F>{px[0], px[1], px[2]};
            }
        return r;
    }

    // config.hpp:6-17 defaults
    [[nodiscard]] static rtk_render_params default_params() noexcept {
        rtk_render_params p{};
        p.spp = 1; p.max_ray_depth = 5; p.diffuse_rays = 0; p.seed = 42; p.fov_degrees = 90.0;
        p.shadow_bias = 1e-4f; p.reflection_bias = 1e-4f; p.refraction_bias = 1e-4f;
        p.trace_mode = RTK_TRACE_AUTO; p.world_size = 1;
        return p;
    }

    // the same defaults for a radiance batch; cull = 1: the batch's rays are traced as render_frame's camera rays are
    [[nodiscard]] static rtk_radiance_params default_radiance_params() noexcept {
        rtk_radiance_params p{};
        p.max_ray_depth = 5; p.diffuse_rays = 0; p.seed = 42; p.sample = 0;
        p.shadow_bias = 1e-4f; p.reflection_bias = 1e-4f; p.refraction_bias = 1e-4f;
        p.cull = 1; p.trace_mode = RTK_TRACE_AUTO;
        return p;
    }

    [[nodiscard]] rtk_accel *handle() const noexcept { return accel_.get(); }

private:
    std::shared_ptr<rtk_accel> accel_;
    std::vector<std::size_t> first_triangle_;     // global triangle index of each mesh's first triangle
    std::size_t n_triangles_ = 0;
    std::vector<std::string> texture_names_;      // the C-ABI's texture indices, in the order the constructor met scene.textures

    // one row of the texture table, as the constructor flattens scene.textures; a bitmap's texels are appended to `texels`
    [[nodiscard]] static rtk_texture to_texture(const texture_variant<F> &tv, std::vector<uint8_t> &texels) {
        rtk_texture out{};
        std::visit([&](const auto &t) {
            using T = std::decay_t<decltype(t)>;
            float *a = out.color_a, *b = out.color_b;
            if constexpr (std::is_same_v<T, albedo_texture<F>>) { out.kind = RTK_TEX_ALBEDO; a[0] = t.albedo.red; a[1] = t.albedo.green; a[2] = t.albedo.blue; }
            else if constexpr (std::is_same_v<T, edge_texture<F>>) {
                out.kind = RTK_TEX_EDGES; out.param = t.edge_width;
                a[0] = t.edge_color.red; a[1] = t.edge_color.green; a[2] = t.edge_color.blue;
                b[0] = t.inner_color.red; b[1] = t.inner_color.green; b[2] = t.inner_color.blue;
            } else if constexpr (std::is_same_v<T, checker_texture<F>>) {
                out.kind = RTK_TEX_CHECKER; out.param = t.square_size;
                a[0] = t.color_a.red; a[1] = t.color_a.green; a[2] = t.color_a.blue;
                b[0] = t.color_b.red; b[1] = t.color_b.green; b[2] = t.color_b.blue;
            } else {                                  // bitmap_texture (scene/texture/bitmap.hpp:40-44)
                out.kind = RTK_TEX_BITMAP;
                to_texels(t.texture, out.width, out.height, texels);
            }
        }, tv);
        return out;
    }

    // image<F> back as the bytes stbi_load gave: a channel is F(byte) * F(1.0 / 255.0) (bitmap.hpp:19-28), inverted exactly
    static void to_texels(const image<F> &im, int32_t &width, int32_t &height, std::vector<uint8_t> &texels) {
        const std::size_t h = im.get_height(), w = im.get_width();
        width = static_cast<int32_t>(w); height = static_cast<int32_t>(h);
        for (std::size_t r = 0; r < h; ++r) for (std::size_t c = 0; c < w; ++c) {
            const auto &px = im.get_pixel(r, c);
            const F ch[3] = {px.red, px.green, px.blue};
            for (F v : ch) texels.push_back(static_cast<uint8_t>(v * F(255) + F(0.5)));
        }
    }

    [[nodiscard]] std::size_t texture_index(const std::string &name, const char *who) const {
        for (std::size_t ti = 0; ti < texture_names_.size(); ++ti) if (texture_names_[ti] == name) return ti;
        throw std::invalid_argument(std::string(who) + ": unknown texture '" + name + "'");
    }

    // one row of the material table, as the constructor flattens scene.materials
    [[nodiscard]] rtk_material to_material(const material_variant<F> &mv) const {
        rtk_material out{};
        out.kind = RTK_MAT_DIFFUSE; out.ior = 1.f; out.texture = -1;
        std::visit([&](const auto &m) {
            using M = std::decay_t<decltype(m)>;
            out.smooth = m.smooth_shading ? 1 : 0;
            if constexpr (std::is_same_v<M, diffuse_material<F>>) out.kind = RTK_MAT_DIFFUSE;
            else if constexpr (std::is_same_v<M, reflective_material<F>>) out.kind = RTK_MAT_REFLECTIVE;
            else if constexpr (std::is_same_v<M, refractive_material<F>>) { out.kind = RTK_MAT_REFRACTIVE; out.ior = m.ior; }
            else if constexpr (std::is_same_v<M, constant_material<F>>) out.kind = RTK_MAT_CONSTANT;
            else {
                out.kind = RTK_MAT_TEXTURE;
                for (std::size_t ti = 0; ti < texture_names_.size(); ++ti) if (texture_names_[ti] == m.texture) out.texture = static_cast<int32_t>(ti);
                if (out.texture < 0) throw std::invalid_argument("hip_accel: material uses unknown texture '" + m.texture + "'");
            }
            if constexpr (requires { m.albedo; }) { out.albedo[0] = m.albedo.red; out.albedo[1] = m.albedo.green; out.albedo[2] = m.albedo.blue; }
        }, mv);
        return out;
    }

    static rtk_view to_view(const camera<F> &c) noexcept {
        rtk_view v{};
        v.position[0] = c.position.x; v.position[1] = c.position.y; v.position[2] = c.position.z;
        for (std::size_t i = 0; i < 9; ++i) v.matrix[i] = c.matrix.m[i];
        return v;
    }

    // render_tile's std::size_t corners as rtk_rect's int32 ones; a corner that does not fit becomes one the library refuses
    template <typename Tile>
    static std::vector<rtk_rect> to_rects(std::span<const Tile> tiles) {
        const auto corner = [](auto v) -> int32_t {
            if constexpr (std::is_unsigned_v<decltype(v)>) {
                return static_cast<unsigned long long>(v) > 0x7FFFFFFFull ? int32_t(0x7FFFFFFF) : static_cast<int32_t>(v);
            } else {
                const long long s = static_cast<long long>(v);
                return s > 0x7FFFFFFFll ? int32_t(0x7FFFFFFF) : (s < -0x7FFFFFFFll ? int32_t(-0x7FFFFFFF) : static_cast<int32_t>(s));
            }
        };
        std::vector<rtk_rect> out(tiles.size());
        for (std::size_t i = 0; i < tiles.size(); ++i) out[i] = rtk_rect{corner(tiles[i].x0), corner(tiles[i].y0), corner(tiles[i].x1), corner(tiles[i].y1)};
        return out;
    }

    // the calls that return finished images take no partial pass of a progressive frame (see render_frame)
    static void whole_samples(const rtk_render_params &params, const char *who) {
        if (params.sample_begin != 0 || (params.sample_count != 0 && params.sample_count != params.spp))
            throw std::invalid_argument(std::string(who) + " renders finished pixels (sample_begin = 0, all spp samples)");
    }

    static void check(int rc) {
        if (rc != RTK_OK) throw std::runtime_error(std::string("rtk: ") + rtk_last_error());
    }

    // rebuilds hit<F> (render/hit.hpp:9-21) from the compact record, as kd_tree_simd.hpp:252-263 fills it
    [[nodiscard]] std::optional<hit<F>> to_hit(const ray3<F> &ray, const rtk_hit &h) const noexcept {
        if (h.tri == 0xFFFFFFFFu) return std::nullopt;
        const auto &mesh = scene_ptr->meshes[h.mesh];
        const auto &tri = mesh.triangles[h.tri - first_triangle_[h.mesh]];
        return hit<F>{
            ray,
            ray.origin + (h.t * ray.direction),
            vec3<F>{h.normal[0], h.normal[1], h.normal[2]},
            tri.normal,
            tri.uvs,
            h.t,
            h.u,
            h.v,
            static_cast<F>(1.) - h.u - h.v,
            static_cast<std::size_t>(h.mesh)
        };
    }
};
