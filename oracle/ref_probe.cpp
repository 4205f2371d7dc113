// ref_probe — a stand-alone program over the reference's own headers (found through -I, nothing of them is copied here).
//
// It reads a flat binary dump of an oracle.FlatScene (oracle/__init__.py: write_scene_dump), builds scene<float> through the
// reference's constructors and answers one command, binary in and binary out:
//
//   ref_probe [--scalar] SCENE tree      -      OUT   node boxes, links, leaf references (ora.Accel.dump() layout), packets
//   ref_probe [--scalar] SCENE intersect RAYS   OUT   intersect<false> and intersect<true>: every field of hit<F> per ray
//   ref_probe [--scalar] SCENE occluded  QUERY  OUT   is_occluded, one byte per query
//   ref_probe [--scalar] SCENE radiance  RAYS   OUT   intersect<true> then color_hit(.., 0), background on a miss
//   ref_probe [--scalar] SCENE frame     -      OUT   render_frame(BUCKET_TILES), the float image
//
// RAYS = float32 [n][6] (origin, direction); QUERY = RAYS followed by float32 max_t [n] (n = file size / 28).
// Every command prints one line "calls=<intersect invocations> hits=<of which hit> width=<packet width>" on stdout.
// Tree shape, eps and packet width are template arguments of the reference, max_ray_depth a constant: one binary per variant
// (oracle/ref.mk).  TEST INFRASTRUCTURE ONLY, like the rest of oracle/.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <stb_image.h>
#include <raytracer/config.hpp>
#include <raytracer/render/hit.hpp>
#ifdef RTK_REF_SCALAR
#include "ref_shim/optional_transform.hpp"
#include <raytracer/render/accel/kd_tree.hpp>
#else
#include <raytracer/render/accel/kd_tree_simd.hpp>
#endif
#include <raytracer/render/render.hpp>

#ifndef RTK_REF_TREE_DEPTH
#define RTK_REF_TREE_DEPTH 8
#endif
#ifndef RTK_REF_TREE_LEAF
#define RTK_REF_TREE_LEAF 64
#endif

using F = float;
#ifdef RTK_REF_SCALAR
using accel_t = kd_tree_accel<F, static_cast<F>(epsilon), RTK_REF_TREE_DEPTH, RTK_REF_TREE_LEAF>;
constexpr std::size_t packet_width = 1;
#else
using accel_t = kd_tree_simd_accel<F, static_cast<F>(epsilon), RTK_REF_TREE_DEPTH, RTK_REF_TREE_LEAF>;   // W = native_simd
constexpr std::size_t packet_width = stdx::native_simd<F>::size();
#endif
static_assert(samples_per_pixel == 1 && diffuse_reflection_ray_count == 0, "the reference's RNG is a data race: GI is not probed");

// ---------------------------------------------------------------- files

static std::vector<unsigned char> read_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> b(static_cast<std::size_t>(n));
    if (n && std::fread(b.data(), 1, b.size(), f) != b.size()) throw std::runtime_error(std::string("short read ") + path);
    std::fclose(f);
    return b;
}

static void write_file(const char* path, const std::vector<unsigned char>& b) {
    FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error(std::string("cannot write ") + path);
    if (!b.empty() && std::fwrite(b.data(), 1, b.size(), f) != b.size()) throw std::runtime_error(std::string("short write ") + path);
    std::fclose(f);
}

template <class T>
static void put(std::vector<unsigned char>& b, const T& v) {
    const auto* p = reinterpret_cast<const unsigned char*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}

struct reader {
    const std::vector<unsigned char>& b;
    std::size_t at = 0;
    template <class T>
    std::vector<T> take(std::size_t n) {
        if (at + n * sizeof(T) > b.size()) throw std::runtime_error("scene dump too short");
        std::vector<T> v(n);
        if (n) std::memcpy(v.data(), b.data() + at, n * sizeof(T));
        at += (n * sizeof(T) + 3) / 4 * 4;
        return v;
    }
};

// ---------------------------------------------------------------- bitmap pixels for the reference's load_bitmap

struct bitmap { int w, h; std::vector<unsigned char> rgb; };
static std::vector<bitmap> g_bitmaps;

extern "C" unsigned char* stbi_load(char const* filename, int* x, int* y, int* channels_in_file, int) {
    const bitmap& bm = g_bitmaps.at(static_cast<std::size_t>(std::atoi(filename)));   // the "file name" is the texture's index
    *x = bm.w; *y = bm.h; *channels_in_file = 3;
    auto* p = static_cast<unsigned char*>(std::malloc(bm.rgb.size() ? bm.rgb.size() : 1));
    std::memcpy(p, bm.rgb.data(), bm.rgb.size());
    return p;
}
extern "C" void stbi_image_free(void* p) { std::free(p); }
extern "C" const char* stbi_failure_reason(void) { return "no decoder in the probe"; }

// ---------------------------------------------------------------- scene dump -> scene<float>

static std::string texture_name(std::int32_t i) { return "texture" + std::to_string(i); }

static scene<F> load_scene(const char* path) {
    const auto bytes = read_file(path);
    reader r{bytes};
    const auto head = r.take<std::int32_t>(13);
    if (head[0] != 0x534B5452 || head[1] != 1) throw std::runtime_error("not a scene dump");       // "RTKS", version 1
    const std::size_t n_meshes = head[2], n_materials = head[3], n_textures = head[4], n_lights = head[5];
    const std::size_t n_verts = head[9], n_tris = head[10], n_uvs = head[11], n_texbytes = head[12];
    const auto mesh_material = r.take<std::int32_t>(n_meshes), mesh_nverts = r.take<std::int32_t>(n_meshes);
    const auto mesh_ntris = r.take<std::int32_t>(n_meshes), mesh_has_uvs = r.take<std::int32_t>(n_meshes);
    const auto vertices = r.take<float>(n_verts * 3);
    const auto indices = r.take<std::uint32_t>(n_tris * 3);
    const auto uvs = r.take<float>(n_uvs * 2);
    const auto mat_kind = r.take<std::int32_t>(n_materials);
    const auto mat_albedo = r.take<float>(n_materials * 3);
    const auto mat_ior = r.take<float>(n_materials);
    const auto mat_smooth = r.take<std::int32_t>(n_materials), mat_texture = r.take<std::int32_t>(n_materials);
    const auto tex_kind = r.take<std::int32_t>(n_textures);
    const auto tex_a = r.take<float>(n_textures * 3), tex_b = r.take<float>(n_textures * 3), tex_param = r.take<float>(n_textures);
    const auto tex_bitmap = r.take<std::int32_t>(n_textures * 3);
    const auto tex_pixels = r.take<unsigned char>(n_texbytes);
    const auto light_pos = r.take<float>(n_lights * 3), light_intensity = r.take<float>(n_lights);
    const auto cam_pos = r.take<float>(3), cam_mat = r.take<float>(9), background = r.take<float>(3);

    scene<F> sc{};
    sc.config = settings<F>{color<F>{background[0], background[1], background[2]}, static_cast<std::size_t>(head[7]),
                            static_cast<std::size_t>(head[6]), static_cast<std::size_t>(head[8])};   // height, width, bucket
    sc.viewpoint = camera<F>{vec3<F>{cam_pos[0], cam_pos[1], cam_pos[2]},
                             mat3<F>{{cam_mat[0], cam_mat[1], cam_mat[2], cam_mat[3], cam_mat[4], cam_mat[5], cam_mat[6], cam_mat[7], cam_mat[8]}}};
    for (std::size_t i = 0; i < n_lights; ++i)
        sc.lights.push_back(light<F>{vec3<F>{light_pos[i * 3], light_pos[i * 3 + 1], light_pos[i * 3 + 2]}, light_intensity[i]});

    g_bitmaps.assign(n_textures, bitmap{0, 0, {}});
    for (std::size_t i = 0; i < n_textures; ++i) {
        const color<F> a{tex_a[i * 3], tex_a[i * 3 + 1], tex_a[i * 3 + 2]}, b{tex_b[i * 3], tex_b[i * 3 + 1], tex_b[i * 3 + 2]};
        const std::string name = texture_name(static_cast<std::int32_t>(i));
        switch (tex_kind[i]) {
            case 0: sc.textures.emplace(name, albedo_texture<F>{a}); break;
            case 1: sc.textures.emplace(name, edge_texture<F>{a, b, tex_param[i]}); break;
            case 2: sc.textures.emplace(name, checker_texture<F>{a, b, tex_param[i]}); break;
            case 3: {
                const std::int32_t* bm = &tex_bitmap[i * 3];
                g_bitmaps[i] = bitmap{bm[1], bm[2], {tex_pixels.begin() + bm[0], tex_pixels.begin() + bm[0] + std::size_t(bm[1]) * bm[2] * 3}};
                sc.textures.emplace(name, bitmap_texture<F>{std::to_string(i)});
                break;
            }
            default: throw std::runtime_error("texture kind");
        }
    }
    for (std::size_t i = 0; i < n_materials; ++i) {
        const color<F> albedo{mat_albedo[i * 3], mat_albedo[i * 3 + 1], mat_albedo[i * 3 + 2]};
        const bool smooth = mat_smooth[i] != 0;
        switch (mat_kind[i]) {
            case 0: sc.materials.emplace_back(diffuse_material<F>{albedo, smooth}); break;
            case 1: sc.materials.emplace_back(reflective_material<F>{albedo, smooth}); break;
            case 2: sc.materials.emplace_back(refractive_material<F>{mat_ior[i], smooth}); break;
            case 3: sc.materials.emplace_back(constant_material<F>{albedo, smooth}); break;
            case 4: sc.materials.emplace_back(texture_material<F>{texture_name(mat_texture[i]), smooth}); break;
            default: throw std::runtime_error("material kind");
        }
    }
    std::size_t voff = 0, toff = 0, uvoff = 0;
    for (std::size_t m = 0; m < n_meshes; ++m) {
        const std::size_t nv = mesh_nverts[m], nt = mesh_ntris[m];
        std::vector<vec3<F>> verts;
        for (std::size_t i = 0; i < nv; ++i)
            verts.push_back(vec3<F>{vertices[(voff + i) * 3], vertices[(voff + i) * 3 + 1], vertices[(voff + i) * 3 + 2]});
        std::vector<vec2<F>> mesh_uvs;
        if (mesh_has_uvs[m])
            for (std::size_t i = 0; i < nv; ++i) mesh_uvs.push_back(vec2<F>{uvs[(uvoff + i) * 2], uvs[(uvoff + i) * 2 + 1]});
        std::vector<triangle<F>> tris;
        for (std::size_t i = 0; i < nt; ++i) {
            const std::size_t a = indices[(toff + i) * 3], b = indices[(toff + i) * 3 + 1], c = indices[(toff + i) * 3 + 2];
            vec3<vec2<F>> tuv{};
            if (!mesh_uvs.empty()) tuv = vec3<vec2<F>>{mesh_uvs[a], mesh_uvs[b], mesh_uvs[c]};
            tris.push_back(triangle<F>{verts[a], verts[b], verts[c], {a, b, c}, m, tuv});
        }
        sc.meshes.emplace_back(mesh_object<F>{static_cast<std::size_t>(mesh_material[m]), verts, mesh_uvs, tris});
        voff += nv; toff += nt;
        if (mesh_has_uvs[m]) uvoff += nv;
    }
    return sc;
}

// ---------------------------------------------------------------- an accelerator that counts the calls it forwards

struct counting_accel {
    const accel_t& inner;
    std::shared_ptr<const scene<F>> scene_ptr;
    mutable std::atomic<std::uint64_t> calls{0}, hits{0};

    template <bool backface_culling>
    std::optional<hit<F>> intersect(const ray3<F>& ray) const {
        auto h = inner.template intersect<backface_culling>(ray);
        calls.fetch_add(1, std::memory_order_relaxed);
        if (h.has_value()) hits.fetch_add(1, std::memory_order_relaxed);
        return h;
    }
};

// ---------------------------------------------------------------- commands

static void cmd_tree(const accel_t& a, std::vector<unsigned char>& out) {
    constexpr std::size_t EMPTY = accel_t::EMPTY;
    std::vector<std::int32_t> link, refs;
    std::vector<float> box;
    std::int64_t packets = 0;
    for (const auto& n : a.tree) {
        for (float v : {n.box.min.x, n.box.min.y, n.box.min.z, n.box.max.x, n.box.max.y, n.box.max.z}) box.push_back(v);
        link.push_back(n.child0 == EMPTY ? -1 : static_cast<std::int32_t>(n.child0));
        link.push_back(n.child1 == EMPTY ? -1 : static_cast<std::int32_t>(n.child1));
        if (n.start_idx == EMPTY) { link.push_back(-1); link.push_back(0); continue; }
        link.push_back(static_cast<std::int32_t>(refs.size()));
        const std::size_t before = refs.size();
#ifdef RTK_REF_SCALAR
        for (std::size_t k = n.start_idx; k < n.start_idx + n.count; ++k) refs.push_back(static_cast<std::int32_t>(a.leaf_indices[k]));
#else
        packets += static_cast<std::int64_t>(n.pack_count);
        // a leaf lists each triangle once and pads its last packet with the last triangle: the padding is the trailing repeats
        for (std::size_t p = n.start_idx; p < n.start_idx + n.pack_count; ++p)
            for (std::size_t lane = 0; lane < packet_width; ++lane) {
                const auto t = static_cast<std::int32_t>(a.triangle_packs[p].triangle_indices[lane]);
                if (refs.size() > before && refs.back() == t) continue;
                refs.push_back(t);
            }
#endif
        link.push_back(static_cast<std::int32_t>(refs.size() - before));
    }
    put(out, static_cast<std::int32_t>(a.tree.size()));
    put(out, static_cast<std::int32_t>(refs.size()));
    put(out, static_cast<std::int32_t>(packets));
    put(out, static_cast<std::int32_t>(packet_width));
    for (float v : box) put(out, v);
    for (auto v : link) put(out, v);
    for (auto v : refs) put(out, v);
}

static std::vector<ray3<F>> rays_of(const std::vector<unsigned char>& in, std::size_t n) {
    std::vector<ray3<F>> rays;
    const auto* f = reinterpret_cast<const float*>(in.data());
    for (std::size_t i = 0; i < n; ++i)
        rays.emplace_back(vec3<F>{f[i * 6], f[i * 6 + 1], f[i * 6 + 2]}, vec3<F>{f[i * 6 + 3], f[i * 6 + 4], f[i * 6 + 5]});
    return rays;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// Which triangle a hit lies on: hit<F> does not say.  The triangles of its mesh whose Moeller-Trumbore (t, u, v), computed
// here in the reference's operation order, equal the hit's bit for bit: the first one and how many.
static void owner_of(const accel_t& a, const ray3<F>& ray, const hit<F>& h, std::uint32_t& first, std::uint32_t& count) {
    first = 0xFFFFFFFFu; count = 0;
    const vec3<F> d = ray.direction, o = ray.origin;
    for (std::size_t k = 0; k < a.triangles.size(); ++k) {
        const auto& tr = a.triangles[k];
        if (tr.mesh_idx != h.mesh_idx) continue;
        const F px = d.y * tr.e2.z - d.z * tr.e2.y, py = d.z * tr.e2.x - d.x * tr.e2.z, pz = d.x * tr.e2.y - d.y * tr.e2.x;
        const F inv_det = F(1) / (tr.e1.x * px + tr.e1.y * py + tr.e1.z * pz);
        const F tx = o.x - tr.v0.x, ty = o.y - tr.v0.y, tz = o.z - tr.v0.z;
        const F u = (tx * px + ty * py + tz * pz) * inv_det;
        if (!same_bits(u, h.u)) continue;
        const F qx = ty * tr.e1.z - tz * tr.e1.y, qy = tz * tr.e1.x - tx * tr.e1.z, qz = tx * tr.e1.y - ty * tr.e1.x;
        const F v = (d.x * qx + d.y * qy + d.z * qz) * inv_det;
        const F t = (tr.e2.x * qx + tr.e2.y * qy + tr.e2.z * qz) * inv_det;
        if (!same_bits(v, h.v) || !same_bits(t, h.distance)) continue;
        if (count++ == 0) first = static_cast<std::uint32_t>(k);
    }
}

// per ray and cull mode 24 words: hit, mesh, tri, owners | t u v w | position | hit_normal | face_normal | uvs[6] | 0
static void cmd_intersect(const accel_t& a, const counting_accel& ca, const std::vector<ray3<F>>& rays, std::vector<unsigned char>& out) {
    for (int cull = 0; cull < 2; ++cull)
        for (const auto& ray : rays) {
            const auto h = cull ? ca.intersect<true>(ray) : ca.intersect<false>(ray);
            std::uint32_t w[4] = {0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0};
            float f[20] = {};
            if (h.has_value()) {
                w[0] = 1; w[1] = static_cast<std::uint32_t>(h->mesh_idx);
                owner_of(a, ray, *h, w[2], w[3]);
                const float v[19] = {h->distance, h->u, h->v, h->w, h->position.x, h->position.y, h->position.z,
                                     h->hit_normal.x, h->hit_normal.y, h->hit_normal.z, h->face_normal.x, h->face_normal.y, h->face_normal.z,
                                     h->uvs.x.x, h->uvs.x.y, h->uvs.y.x, h->uvs.y.y, h->uvs.z.x, h->uvs.z.y};
                std::memcpy(f, v, sizeof(v));
            }
            for (auto x : w) put(out, x);
            for (auto x : f) put(out, x);
        }
}

int main(int argc, char** argv) try {
    int at = 1;
    bool scalar = false;
    if (at < argc && std::strcmp(argv[at], "--scalar") == 0) { scalar = true; ++at; }
#ifdef RTK_REF_SCALAR
    if (!scalar) throw std::runtime_error("this binary holds kd_tree_accel: pass --scalar");
#else
    if (scalar) throw std::runtime_error("this binary holds kd_tree_simd_accel: --scalar needs the scalar build");
#endif
    if (argc - at != 4) {
        std::fprintf(stderr, "usage: ref_probe [--scalar] SCENE tree|intersect|occluded|radiance|frame IN|- OUT\n");
        return 2;
    }
    const std::string cmd = argv[at + 1];
    const auto sc = std::make_shared<const scene<F>>(load_scene(argv[at]));
    const accel_t accel(sc);
    const counting_accel ca{accel, sc};
    std::vector<unsigned char> in, out;
    if (std::strcmp(argv[at + 2], "-") != 0) in = read_file(argv[at + 2]);

    if (cmd == "tree") {
        cmd_tree(accel, out);
    } else if (cmd == "intersect") {
        cmd_intersect(accel, ca, rays_of(in, in.size() / 24), out);
    } else if (cmd == "occluded") {
        const std::size_t n = in.size() / 28;
        const auto rays = rays_of(in, n);
        const auto* max_t = reinterpret_cast<const float*>(in.data() + n * 24);
        for (std::size_t i = 0; i < n; ++i) out.push_back(is_occluded<counting_accel, F>(ca, rays[i], max_t[i]) ? 1 : 0);
    } else if (cmd == "radiance") {
        const color<F> background = sc->config.background_color;
        for (const auto& ray : rays_of(in, in.size() / 24)) {
            const auto h = ca.intersect<true>(ray);
            const color<F> c = h.has_value() ? color_hit<counting_accel, F>(ca, h.value(), 0uz) : background;
            put(out, c.red); put(out, c.green); put(out, c.blue);
        }
    } else if (cmd == "frame") {
        const auto img = render_frame<counting_accel, F>(ca, scheduling_type::BUCKET_TILES);
        for (std::size_t y = 0; y < img.get_height(); ++y)
            for (std::size_t x = 0; x < img.get_width(); ++x) {
                const auto& c = img.get_pixel(y, x);
                put(out, c.red); put(out, c.green); put(out, c.blue);
            }
    } else {
        throw std::runtime_error("unknown command " + cmd);
    }
    write_file(argv[at + 3], out);
    std::printf("calls=%llu hits=%llu width=%zu\n", static_cast<unsigned long long>(ca.calls.load()),
                static_cast<unsigned long long>(ca.hits.load()), packet_width);
    return 0;
} catch (const std::exception& e) {
    std::fprintf(stderr, "ref_probe: %s\n", e.what());
    return 1;
}
