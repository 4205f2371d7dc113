// Textures and uvs of a live accel on accels that were NEVER resident: everything here is host work and needs no device.
// argv[1] = a scene with textures, uvs and a bitmap (hw12/scene4.crtscene), argv[2] = one without either (hw09/scene5.crtscene).
// The C-ABI first (include/rtk.h), then hip_accel::set_textures / textures_now / set_texture_pixels / set_uvs / uvs_now
// (simd-raytracer_amd/hip_accel.hpp) on a quad.  Prints one line per failed check and "textures_check: N checks, F failed";
// the exit status is 1 when something failed.  tests/test_cpp_textures.py also builds it with the address and
// undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <memory>
#include <string>
#include <variant>
#include <vector>

#include "hip_accel.hpp"

using F = float;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

struct Table {
    std::vector<rtk_texture> rows;
    std::vector<std::vector<uint8_t>> texels;
    std::vector<const uint8_t *> ptrs() const {
        std::vector<const uint8_t *> p;
        for (const auto &t : texels) p.push_back(t.empty() ? nullptr : t.data());
        p.push_back(nullptr);
        return p;
    }
    bool operator==(const Table &o) const {
        if (rows.size() != o.rows.size()) return false;
        for (std::size_t i = 0; i < rows.size(); ++i)
            if (std::memcmp(&rows[i], &o.rows[i], sizeof(rtk_texture)) != 0 || texels[i] != o.texels[i]) return false;
        return true;
    }
};

static Table table_of(const rtk_accel *a) {
    Table t;
    int32_t n = -1;
    CHECK(rtk_accel_get_textures(a, nullptr, 0, &n) == RTK_OK && n >= 0);
    t.rows.resize(static_cast<std::size_t>(n) + 1);
    CHECK(rtk_accel_get_textures(a, t.rows.data(), n, &n) == RTK_OK);
    t.rows.resize(static_cast<std::size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
        std::size_t bytes = 12345;
        CHECK(rtk_accel_get_texture_pixels(a, i, nullptr, 0, &bytes) == RTK_OK);
        CHECK(bytes == static_cast<std::size_t>(t.rows[i].width) * static_cast<std::size_t>(t.rows[i].height) * 3);
        std::vector<uint8_t> px(bytes);
        if (bytes > 0) CHECK(rtk_accel_get_texture_pixels(a, i, px.data(), px.size(), &bytes) == RTK_OK);
        t.texels.push_back(std::move(px));
    }
    return t;
}

static std::vector<rtk_material> materials_of(const rtk_accel *a, const rtk_scene *s) {
    rtk_scene_info info{};
    CHECK(rtk_scene_get_info(s, &info) == RTK_OK);
    std::vector<rtk_material> m(static_cast<std::size_t>(info.n_materials) + 1);
    CHECK(rtk_accel_get_materials(a, m.data()) == RTK_OK);
    m.resize(static_cast<std::size_t>(info.n_materials));
    return m;
}

static std::vector<float> uvs_of(const rtk_accel *a, int32_t n_vertices) {
    std::vector<float> uv(static_cast<std::size_t>(n_vertices) * 2 + 2, 7.0f);
    CHECK(rtk_accel_get_uvs(a, uv.data()) == RTK_OK);
    uv.resize(static_cast<std::size_t>(n_vertices) * 2);
    return uv;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

static std::vector<uint8_t> noise(std::size_t n, uint32_t seed) {
    std::vector<uint8_t> out(n);
    for (auto &b : out) { seed = seed * 1664525u + 1013904223u; b = static_cast<uint8_t>(seed >> 24); }
    return out;
}

struct Loaded {
    rtk_scene *scene = nullptr;
    rtk_accel *accel = nullptr;
    rtk_scene_info info{};
    explicit Loaded(const char *path) {
        CHECK(rtk_scene_load_crtscene(path, &scene) == RTK_OK);
        if (!scene) { std::printf("cannot load %s: %s\n", path, rtk_last_error()); return; }
        CHECK(rtk_scene_get_info(scene, &info) == RTK_OK);
        CHECK(rtk_accel_build(scene, nullptr, &accel) == RTK_OK);
    }
    ~Loaded() { rtk_accel_destroy(accel); rtk_scene_destroy(scene); }
};

// ---------------------------------------------------------------- the textured scene

static void textured(const char *path) {
    Loaded L(path);
    if (!L.accel) return;
    rtk_accel *a = L.accel;
    const Table own = table_of(a);
    int bitmap = -1, checker = -1;
    for (std::size_t i = 0; i < own.rows.size(); ++i) {
        if (own.rows[i].kind == RTK_TEX_BITMAP) bitmap = static_cast<int>(i);
        if (own.rows[i].kind == RTK_TEX_CHECKER) checker = static_cast<int>(i);
    }
    CHECK(own.rows.size() == static_cast<std::size_t>(L.info.n_textures) && bitmap >= 0 && checker >= 0);
    if (bitmap < 0 || checker < 0) return;
    CHECK(own.texels[static_cast<std::size_t>(bitmap)].size() == static_cast<std::size_t>(L.info.n_bitmap_bytes));
    // a partial fetch: the count is the table's, the rows the first `cap`
    {
        std::vector<rtk_texture> part(2);
        int32_t n = 0;
        CHECK(rtk_accel_get_textures(a, part.data(), 1, &n) == RTK_OK && n == L.info.n_textures);
        CHECK(std::memcmp(&part[0], &own.rows[0], sizeof(rtk_texture)) == 0 && part[1].kind == 0 && part[1].width == 0);
    }
    // get -> set -> get
    CHECK(rtk_accel_set_textures(a, own.rows.data(), static_cast<int32_t>(own.rows.size()), own.ptrs().data()) == RTK_OK);
    CHECK(table_of(a) == own);
    // what a bitmap's colours and another kind's size hold is dropped
    {
        Table odd = own;
        odd.rows[static_cast<std::size_t>(bitmap)].color_a[1] = 0.5f; odd.rows[static_cast<std::size_t>(bitmap)].param = 3.f;
        odd.rows[static_cast<std::size_t>(checker)].width = 9; odd.rows[static_cast<std::size_t>(checker)].height = 4;
        CHECK(rtk_accel_set_textures(a, odd.rows.data(), static_cast<int32_t>(odd.rows.size()), odd.ptrs().data()) == RTK_OK);
        CHECK(table_of(a) == own);
    }
    // colours and parameters as they are: -0.0, a NaN, an infinity, a zero square size
    {
        Table odd = own;
        rtk_texture &c = odd.rows[static_cast<std::size_t>(checker)];
        c.color_a[0] = -0.0f; c.color_a[1] = std::numeric_limits<float>::quiet_NaN(); c.color_b[2] = std::numeric_limits<float>::infinity(); c.param = 0.0f;
        CHECK(rtk_accel_set_textures(a, odd.rows.data(), static_cast<int32_t>(odd.rows.size()), odd.ptrs().data()) == RTK_OK);
        CHECK(table_of(a) == odd);
        CHECK(rtk_accel_set_textures(a, own.rows.data(), static_cast<int32_t>(own.rows.size()), own.ptrs().data()) == RTK_OK);
    }
    const std::vector<rtk_material> mats = materials_of(a, L.scene);
    const std::vector<float> uv0 = uvs_of(a, L.info.n_vertices);

    // ---- every refusal: RTK_ERR_INVALID, never RTK_ERR_NO_DEVICE, and the getters as before
    const int32_t n_own = static_cast<int32_t>(own.rows.size());
    const auto p_own = own.ptrs();
    std::size_t bytes = 0;
    int32_t n = 0;
    std::vector<uint8_t> some = noise(64, 1);
    std::vector<float> somef(64, 0.5f);
    CHECK(rtk_accel_get_textures(nullptr, nullptr, 0, &n) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_textures(a, nullptr, 0, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_texture_pixels(nullptr, 0, nullptr, 0, &bytes) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_texture_pixels(a, 0, nullptr, 0, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_texture_pixels(a, -1, nullptr, 0, &bytes) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_texture_pixels(a, n_own, nullptr, 0, &bytes) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_textures(nullptr, own.rows.data(), n_own, p_own.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_textures(a, own.rows.data(), -1, p_own.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_textures(a, nullptr, n_own, p_own.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_textures(a, own.rows.data(), n_own, nullptr) == RTK_ERR_INVALID);          // a bitmap without the pointer array
    {
        auto p = p_own;
        p[static_cast<std::size_t>(bitmap)] = nullptr;
        CHECK(rtk_accel_set_textures(a, own.rows.data(), n_own, p.data()) == RTK_ERR_INVALID);      // ... and without its own pointer
    }
    for (int32_t kind : {-1, 4, 99}) {
        Table bad = own;
        bad.rows.back().kind = kind;                                                             // the LAST row: everything before it was valid
        CHECK(rtk_accel_set_textures(a, bad.rows.data(), n_own, bad.ptrs().data()) == RTK_ERR_INVALID);
    }
    const int32_t sizes[][2] = {{0, 4}, {4, 0}, {-1, 4}, {4, -3}, {16385, 16384}, {1 << 30, 1 << 30}};
    for (const auto &wh : sizes) {
        Table bad = own;
        bad.rows[static_cast<std::size_t>(bitmap)].width = wh[0]; bad.rows[static_cast<std::size_t>(bitmap)].height = wh[1];
        CHECK(rtk_accel_set_textures(a, bad.rows.data(), n_own, p_own.data()) == RTK_ERR_INVALID);  // (refused before a texel is read)
        CHECK(rtk_accel_set_texture_pixels(a, bitmap, wh[0], wh[1], some.data()) == RTK_ERR_INVALID);
        CHECK(rtk_accel_set_texture_pixels_device(a, bitmap, wh[0], wh[1], some.data(), nullptr) == RTK_ERR_INVALID);
        CHECK(rtk_accel_set_texture_frame_device(a, bitmap, wh[0], wh[1], somef.data(), nullptr) == RTK_ERR_INVALID);
    }
    {
        // three bitmaps of 2^28 texels: each is legal, together their 3 * 805,306,368 bytes pass an int32 offset
        std::vector<rtk_texture> big(3);
        for (auto &t : big) { t.kind = RTK_TEX_BITMAP; t.width = 16384; t.height = 16384; }
        const uint8_t *p[3] = {some.data(), some.data(), some.data()};
        CHECK(rtk_accel_set_textures(a, big.data(), 3, p) == RTK_ERR_INVALID);                    // (refused before a texel is read)
    }
    CHECK(rtk_accel_set_textures(a, own.rows.data(), 0, nullptr) == RTK_ERR_INVALID);             // texture materials exist
    CHECK(rtk_accel_set_textures(a, own.rows.data(), n_own - 1, p_own.data()) == RTK_ERR_INVALID);   // (hw12/scene4 uses every texture)
    CHECK(rtk_accel_set_texture_pixels(nullptr, bitmap, 2, 2, some.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels(a, bitmap, 2, 2, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels(a, -1, 2, 2, some.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels(a, n_own, 2, 2, some.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels(a, checker, 2, 2, some.data()) == RTK_ERR_INVALID);          // not a bitmap
    CHECK(rtk_accel_set_texture_pixels_device(nullptr, bitmap, 2, 2, some.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels_device(a, bitmap, 2, 2, nullptr, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels_device(a, n_own, 2, 2, some.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels_device(a, checker, 2, 2, some.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_frame_device(nullptr, bitmap, 2, 2, somef.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_frame_device(a, bitmap, 2, 2, nullptr, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_frame_device(a, -1, 2, 2, somef.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_frame_device(a, checker, 2, 2, somef.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_uvs(nullptr, somef.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_uvs(a, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_uvs(nullptr, somef.data()) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_uvs(a, nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_uvs_device(nullptr, somef.data(), nullptr) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_uvs_device(a, nullptr, nullptr) == RTK_ERR_INVALID);
    CHECK(table_of(a) == own);
    CHECK(same_bits(uvs_of(a, L.info.n_vertices), uv0));
    {
        const std::vector<rtk_material> now = materials_of(a, L.scene);
        CHECK(now.size() == mats.size() && std::memcmp(now.data(), mats.data(), mats.size() * sizeof(rtk_material)) == 0);
    }

    // ---- n = 0 once no material uses a texture; then a texture material is refused
    std::vector<rtk_material> diffuse = mats;
    for (auto &m : diffuse) m.kind = RTK_MAT_DIFFUSE;
    CHECK(rtk_accel_set_materials(a, diffuse.data(), static_cast<int32_t>(diffuse.size())) == RTK_OK);
    CHECK(rtk_accel_set_textures(a, nullptr, 0, nullptr) == RTK_OK);
    CHECK(table_of(a).rows.empty());
    CHECK(rtk_accel_set_materials(a, mats.data(), static_cast<int32_t>(mats.size())) == RTK_ERR_INVALID);
    CHECK(rtk_accel_get_texture_pixels(a, 0, nullptr, 0, &bytes) == RTK_ERR_INVALID);
    CHECK(rtk_accel_set_texture_pixels(a, 0, 2, 2, some.data()) == RTK_ERR_INVALID);
    // ... and back: the table, then the materials
    CHECK(rtk_accel_set_textures(a, own.rows.data(), n_own, p_own.data()) == RTK_OK);
    CHECK(rtk_accel_set_materials(a, mats.data(), static_cast<int32_t>(mats.size())) == RTK_OK);
    CHECK(table_of(a) == own);

    // ---- bitmaps of awkward sizes: a 1 x 1, then a 3 x 5 at dense byte offset 3, then the scene's own
    Table awkward;
    awkward.rows.resize(3);
    awkward.texels = {noise(3, 2), noise(45, 3), own.texels[static_cast<std::size_t>(bitmap)]};
    awkward.rows[0].kind = awkward.rows[1].kind = awkward.rows[2].kind = RTK_TEX_BITMAP;
    awkward.rows[0].width = 1; awkward.rows[0].height = 1;
    awkward.rows[1].width = 3; awkward.rows[1].height = 5;
    awkward.rows[2].width = own.rows[static_cast<std::size_t>(bitmap)].width; awkward.rows[2].height = own.rows[static_cast<std::size_t>(bitmap)].height;
    std::vector<rtk_material> three = mats;
    for (auto &m : three) if (m.kind == RTK_MAT_TEXTURE) m.texture = m.texture % 3;
    CHECK(rtk_accel_set_materials(a, three.data(), static_cast<int32_t>(three.size())) == RTK_OK);
    CHECK(rtk_accel_set_textures(a, awkward.rows.data(), 3, awkward.ptrs().data()) == RTK_OK);
    CHECK(table_of(a) == awkward);
    // the middle one grows, shrinks and becomes a single texel: its neighbours keep their bytes
    const int32_t steps[][2] = {{7, 2}, {64, 64}, {1, 1}, {3, 5}, {3, 5}};
    for (const auto &wh : steps) {
        awkward.rows[1].width = wh[0]; awkward.rows[1].height = wh[1];
        awkward.texels[1] = noise(static_cast<std::size_t>(wh[0]) * static_cast<std::size_t>(wh[1]) * 3, static_cast<uint32_t>(wh[0] * 131 + wh[1]));
        CHECK(rtk_accel_set_texture_pixels(a, 1, wh[0], wh[1], awkward.texels[1].data()) == RTK_OK);
        CHECK(table_of(a) == awkward);
    }
    // a short fetch takes the first `cap` bytes
    {
        std::vector<uint8_t> part(8, 0xEE);
        CHECK(rtk_accel_get_texture_pixels(a, 1, part.data(), 5, &bytes) == RTK_OK && bytes == 45);
        CHECK(std::memcmp(part.data(), awkward.texels[1].data(), 5) == 0 && part[5] == 0xEE);
    }

    // ---- uvs: their bits, a -0.0 and a NaN among them
    std::vector<float> uv = uv0;
    CHECK(uv.size() >= 8);
    for (std::size_t i = 0; i < uv.size(); ++i) uv[i] = uv0[i] * 0.75f - 0.125f;
    uv[0] = -0.0f; uv[3] = std::numeric_limits<float>::quiet_NaN(); uv[5] = -2.5f; uv[6] = 1e30f;
    CHECK(rtk_accel_set_uvs(a, uv.data()) == RTK_OK);
    CHECK(same_bits(uvs_of(a, L.info.n_vertices), uv) && std::signbit(uvs_of(a, L.info.n_vertices)[0]));
    CHECK(rtk_accel_set_uvs(a, uv0.data()) == RTK_OK);
    CHECK(same_bits(uvs_of(a, L.info.n_vertices), uv0));
}

// ---------------------------------------------------------------- the scene without textures and without uvs

static void plain(const char *path) {
    Loaded L(path);
    if (!L.accel) return;
    rtk_accel *a = L.accel;
    CHECK(L.info.n_textures == 0 && L.info.n_uv_vertices == 0);
    CHECK(table_of(a).rows.empty());
    const std::vector<float> zeros = uvs_of(a, L.info.n_vertices);
    bool all_zero = !zeros.empty();
    for (float f : zeros) all_zero = all_zero && f == 0.0f && !std::signbit(f);
    CHECK(all_zero);                                                                               // a mesh without uvs has zeros
    std::vector<rtk_material> mats = materials_of(a, L.scene);
    std::vector<rtk_material> tex = mats;
    tex.back().kind = RTK_MAT_TEXTURE; tex.back().texture = 0;
    CHECK(rtk_accel_set_materials(a, tex.data(), static_cast<int32_t>(tex.size())) == RTK_ERR_INVALID);   // no texture yet
    // uvs on an accel without textures: stored
    std::vector<float> uv(zeros.size());
    for (std::size_t i = 0; i < uv.size(); ++i) uv[i] = static_cast<float>(i % 17) / 16.0f - 0.25f;
    CHECK(rtk_accel_set_uvs(a, uv.data()) == RTK_OK);
    CHECK(same_bits(uvs_of(a, L.info.n_vertices), uv));
    // ... gains an albedo texture, and set_materials then accepts RTK_MAT_TEXTURE
    rtk_texture albedo{};
    albedo.kind = RTK_TEX_ALBEDO; albedo.color_a[0] = 0.25f; albedo.color_a[1] = 0.5f; albedo.color_a[2] = 0.75f;
    CHECK(rtk_accel_set_textures(a, &albedo, 1, nullptr) == RTK_OK);
    Table got = table_of(a);
    CHECK(got.rows.size() == 1 && std::memcmp(&got.rows[0], &albedo, sizeof(albedo)) == 0);
    CHECK(rtk_accel_set_materials(a, tex.data(), static_cast<int32_t>(tex.size())) == RTK_OK);
    CHECK(materials_of(a, L.scene).back().texture == 0);
    tex.back().texture = 1;
    CHECK(rtk_accel_set_materials(a, tex.data(), static_cast<int32_t>(tex.size())) == RTK_ERR_INVALID);   // the live count is 1
    CHECK(rtk_accel_set_textures(a, nullptr, 0, nullptr) == RTK_ERR_INVALID);                      // in use now
    // a checker and a 4 x 4 bitmap in its place
    rtk_texture two[2] = {};
    two[0].kind = RTK_TEX_CHECKER; two[0].color_a[0] = 1.f; two[0].color_b[2] = 1.f; two[0].param = 0.125f;
    two[1].kind = RTK_TEX_BITMAP; two[1].width = 4; two[1].height = 4;
    const std::vector<uint8_t> px = noise(48, 9);
    const uint8_t *ptrs[2] = {nullptr, px.data()};
    CHECK(rtk_accel_set_textures(a, two, 2, ptrs) == RTK_OK);
    got = table_of(a);
    CHECK(got.rows.size() == 2 && got.texels[1] == px && got.texels[0].empty());
    CHECK(rtk_accel_set_materials(a, mats.data(), static_cast<int32_t>(mats.size())) == RTK_OK);
    CHECK(rtk_accel_set_textures(a, nullptr, 0, nullptr) == RTK_OK);
    CHECK(same_bits(uvs_of(a, L.info.n_vertices), uv));                                            // the uvs outlive the textures
}

// ---------------------------------------------------------------- the adapter

static void adapter() {
    using A = hip_accel<F, 1e-6f>;
    scene<F> sc{};
    sc.config = {{0.25f, 0.5f, 0.75f}, 16, 16, 64};
    sc.viewpoint = {{0.f, 0.f, 0.f}, {{1, 0, 0, 0, 1, 0, 0, 0, 1}}};
    sc.lights.push_back({{0.f, 3.f, -2.f}, 150.f});
    sc.materials.push_back(diffuse_material<F>{{0.9f, 0.6f, 0.3f}, false});
    mesh_object<F> m{};
    m.material_idx = 0;
    m.vertices = {{-1.f, -1.f, -4.f}, {1.f, -1.f, -4.f}, {1.f, 1.f, -4.f}, {-1.f, 1.f, -4.f}};
    const std::size_t idx[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (const auto &i : idx) {
        triangle<F> t{};
        t.v0 = m.vertices[i[0]]; t.v1 = m.vertices[i[1]]; t.v2 = m.vertices[i[2]];
        t.normal = {0.f, 0.f, 1.f};
        t.vertex_indices = {i[0], i[1], i[2]};
        t.mesh_idx = 0;
        m.triangles.push_back(t);
    }
    sc.meshes.push_back(m);
    try {
        A accel(std::make_shared<const scene<F>>(sc));
        CHECK(accel.textures_now().empty());
        const auto uv0 = accel.uvs_now();
        CHECK(uv0.size() == 4 && uv0[2].x == 0.f && uv0[2].y == 0.f);
        const std::vector<vec2<F>> uv = {{0.f, 0.f}, {1.f, -0.0f}, {1.f, 1.f}, {-0.5f, 1.5f}};
        accel.set_uvs(uv);
        const auto uv1 = accel.uvs_now();
        CHECK(uv1.size() == 4 && uv1[3].x == -0.5f && uv1[3].y == 1.5f && std::signbit(uv1[1].y));
        image<F> im(2, 3, std::vector<std::vector<color<F>>>(2, std::vector<color<F>>(3, color<F>{F(51) * F(1.0 / 255.0), 0.f, 1.f})));
        const std::vector<A::named_texture> table = {{"squares", checker_texture<F>{{1.f, 0.f, 0.f}, {0.f, 0.f, 1.f}, 0.25f}},
                                                     {"screen", bitmap_texture<F>{im}}};
        accel.set_textures(table);
        auto now = accel.textures_now();
        CHECK(now.size() == 2 && now[0].first == "squares" && now[1].first == "screen");
        CHECK(std::holds_alternative<checker_texture<F>>(now[0].second) && std::get<checker_texture<F>>(now[0].second).square_size == 0.25f);
        CHECK(std::holds_alternative<image<F>>(now[1].second));
        const image<F> &back = std::get<image<F>>(now[1].second);
        CHECK(back.get_height() == 2 && back.get_width() == 3 && back.get_pixel(1, 2).red == F(51) * F(1.0 / 255.0) && back.get_pixel(0, 0).blue == 1.f);
        accel.set_materials(std::vector<material_variant<F>>{texture_material<F>{"screen", false}});
        CHECK(std::holds_alternative<texture_material<F>>(accel.materials_now()[0]) && std::get<texture_material<F>>(accel.materials_now()[0]).texture == "screen");
        image<F> one(1, 1, std::vector<std::vector<color<F>>>(1, std::vector<color<F>>(1, color<F>{1.f, 1.f, 0.f})));
        accel.set_texture_pixels("screen", one);
        now = accel.textures_now();
        CHECK(std::get<image<F>>(now[1].second).get_width() == 1 && std::get<image<F>>(now[1].second).get_pixel(0, 0).green == 1.f);
        bool refused = false;
        try { accel.set_texture_pixels("squares", one); } catch (const std::exception &) { refused = true; }
        CHECK(refused);
        refused = false;
        try { accel.set_textures(std::span<const A::named_texture>(table.data(), 1)); } catch (const std::exception &) { refused = true; }
        CHECK(refused);                                                                            // "screen" is in use
        refused = false;
        try { accel.set_uvs(std::span<const vec2<F>>(uv.data(), 3)); } catch (const std::exception &) { refused = true; }
        CHECK(refused);
    } catch (const std::exception &e) {
        std::printf("exception %s\n", e.what());
        ++g_failed;
    }
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: textures_check TEXTURED.crtscene PLAIN.crtscene\n"); return 2; }
    textured(argv[1]);
    plain(argv[2]);
    adapter();
    std::printf("textures_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
