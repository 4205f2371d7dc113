// C-ABI, the rest of scene<F> on a live accel: rtk_accel_{get,set}_lights, _materials and _background (rtk.h).  The launch paths
// read a->scene and the device tables when they run (api_frame.hip scene_args), so most of this is bookkeeping; the device work
// that a changed set of refractive materials asks for is remake_occluders (api_update.hip, occluders.hip).
// Then the textures and uvs (rtk.h, "textures and uvs of a live accel"): the table, the texels of one bitmap -- every bitmap of a
// resident accel has a slot in d_tex_pixels -- and the per-vertex uvs, from which k_tri_uv (topology.hip) makes the per-triangle ones.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "accel.hpp"

using namespace rtk;

namespace {

// Room for n lights in d_lights, of a resident accel whose device is idle.  A larger table is made before the old one goes, so a
// failure leaves the accel as it was.
int reserve_lights(rtk_accel *a, size_t n) {
    if (n <= a->d_lights.capacity()) return RTK_OK;
    DevBuf<DevLight> larger;
    RTK_MEM(larger.reserve(n, grow_lights()));
    a->d_lights.swap(larger);                            // (the old table goes with `larger`)
    return RTK_OK;
}

// every block's cost scales with the number of lights; their positions leave the silhouettes where they are (rtk.h), but move the
// shadow edges and with them the costs of the blocks they cross: the orders stay in use, and their schedules start over, so that
// the list in use is re-sorted and judged again within RTK_COST_RESORT_EVERY frames of its last sort (behind the next frame if it is
// older already) and not up to RTK_COST_RESORT_MAX later -- however often the call comes, it never puts a sort off
void lights_changed(rtk_accel *a, size_t n_before) {
    if (a->scene.lights.size() == n_before) { restart_order_schedules(a); return; }
    forget_orders(a, kKeepTrial);
}

// ---- textures and uvs

constexpr size_t kTexelLimit = 0x7FFFFFFFull;              // DevTexture::bmp[2] is an int32 byte offset
constexpr size_t kSlotAlign = 16;

inline size_t slot_round(size_t bytes) { return (bytes + kSlotAlign - 1) & ~(kSlotAlign - 1); }
inline bool is_bitmap(const DevTexture &t) { return t.kind == RTK_TEX_BITMAP; }
inline size_t texel_bytes(const DevTexture &t) { return is_bitmap(t) ? size_t(t.bmp[0]) * size_t(t.bmp[1]) * 3 : 0; }

// scene_from_desc's judgement of a bitmap's size (scene.cpp)
inline bool bitmap_size_ok(int32_t w, int32_t h) { return w >= 1 && h >= 1 && int64_t(w) * int64_t(h) <= (int64_t{1} << 28); }

// per-triangle uvs on the host, for an accel that has never been updated (its triangles are still here): kdtree.cpp build_tree
void host_tri_uv(const rtk_accel *a, const std::vector<float> &vert_uv, std::vector<DevTriUv> &out) {
    std::vector<size_t> first(a->mesh_nverts.size() + 1, 0);
    for (size_t mi = 0; mi < a->mesh_nverts.size(); ++mi) first[mi + 1] = first[mi] + size_t(a->mesh_nverts[mi]);
    out.resize(a->tree.triangles.size());
    for (size_t i = 0; i < out.size(); ++i) {
        const HostTriangle &tr = a->tree.triangles[i];
        for (int k = 0; k < 3; ++k) {
            const size_t g = first[tr.mesh] + tr.vi[k];
            out[i].uv[k * 2] = vert_uv[g * 2]; out[i].uv[k * 2 + 1] = vert_uv[g * 2 + 1];
        }
    }
}

// DevTriUv of the live topology from topo_vert_uv, on `s`, into the spare table; the caller swaps it in once nothing can fail
int make_tri_uv(rtk_accel *a, hipStream_t s) {
    RTK_TRY(ensure_update_static(a));
    const size_t nt = size_t(a->scene.n_triangles);
    RTK_MEM(a->topo_spare.tri_uv.reserve(std::max<size_t>(1, nt), grow_bytes()));
    RTK_HIP_AS(launch_tri_uv(a->topo.index.get(), a->topo_vert_uv.get(), uint32_t(nt), uint32_t(a->scene.n_vertices), a->topo_spare.tri_uv.get(), s),
               "launch k_tri_uv");
    return RTK_OK;
}

// the device's row of texture i: the host's, with the offset of its slot
DevTexture device_row(const DevTexture &host, const rtk_accel::TexSlot &slot) {
    DevTexture t = host;
    if (is_bitmap(t)) t.bmp[2] = slot.off;
    return t;
}

// rows [first, first + n) of `rows` to the same rows of `table`, on `s`, through the pinned stage: the host does not wait
int send_rows(rtk_accel *a, const std::vector<DevTexture> &rows, DevTexture *table, size_t first, size_t n, hipStream_t s) {
    if (n == 0) return RTK_OK;
    RTK_MEM(a->up_stage.reserve(n * sizeof(DevTexture), grow_bytes()));
    std::memcpy(a->up_stage.get(), rows.data() + first, n * sizeof(DevTexture));
    RTK_HIP(hipMemcpyAsync(table + first, a->up_stage.get(), n * sizeof(DevTexture), hipMemcpyHostToDevice, s));
    return RTK_OK;
}

// What one texel setter is about to do to a RESIDENT accel whose device is idle: where the texels of `texture` go.
struct TexelPlan {
    uint8_t *dst = nullptr;                     // where the caller writes width * height * 3 bytes, on `s`
    std::vector<rtk_accel::TexSlot> slots;      // the slots afterwards
    size_t used = 0;
    bool moved = false;                         // the other bitmaps were copied into tx_pixels and the table written to tx_textures
};

// Room for `need` bytes of texture `texture`, whose new row is `row` (host offsets; the device's is written here).  Within the
// slot: in place.  Else a new slot with head room at the end of the buffer, or -- when that is full -- a larger buffer.
int place_texels(rtk_accel *a, size_t texture, const DevTexture &row, size_t need, hipStream_t s, TexelPlan &P) {
    const std::vector<DevTexture> &tex = a->scene.textures;
    P.slots = a->tx_slots; P.used = a->tx_used;
    rtk_accel::TexSlot &mine = P.slots[texture];
    const bool same_shape = tex[texture].bmp[0] == row.bmp[0] && tex[texture].bmp[1] == row.bmp[1];
    if (need <= mine.cap) {
        P.dst = a->d_tex_pixels.get() + mine.off;
        if (same_shape) return RTK_OK;                                       // (the steady case: the row stays as it is)
    } else {
        size_t room = slot_round(need + need / 2);
        size_t off = slot_round(P.used);
        if (off + room > kTexelLimit) room = slot_round(need);
        if (off + room <= a->d_tex_pixels.capacity() && off + room <= kTexelLimit && a->d_tex_pixels.get()) {
            mine.off = int32_t(off); mine.cap = room; P.used = off + room;
            P.dst = a->d_tex_pixels.get() + off;
        } else {
            // every bitmap into the spare buffer, packed again
            size_t at = 0;
            std::vector<rtk_accel::TexSlot> packed = P.slots;
            for (size_t i = 0; i < tex.size(); ++i) {
                if (!is_bitmap(tex[i])) continue;
                const size_t live = i == texture ? need : texel_bytes(tex[i]);
                packed[i].off = int32_t(at); packed[i].cap = slot_round(i == texture ? need + need / 2 : live);
                if (at + packed[i].cap > kTexelLimit) packed[i].cap = slot_round(live);
                at += packed[i].cap;
                if (at > kTexelLimit) return fail(RTK_ERR_INVALID, "the texel bytes of all bitmaps must fit an int32 offset");
            }
            RTK_MEM(a->tx_pixels.reserve(at, grow_bytes()));
            for (size_t i = 0; i < tex.size(); ++i)
                if (is_bitmap(tex[i]) && i != texture)
                    RTK_HIP(hipMemcpyAsync(a->tx_pixels.get() + packed[i].off, a->d_tex_pixels.get() + P.slots[i].off, texel_bytes(tex[i]),
                                           hipMemcpyDeviceToDevice, s));
            P.slots.swap(packed); P.used = at; P.moved = true;
            P.dst = a->tx_pixels.get() + P.slots[texture].off;
            std::vector<DevTexture> rows(tex.size());
            for (size_t i = 0; i < tex.size(); ++i) rows[i] = device_row(i == texture ? row : tex[i], P.slots[i]);
            RTK_MEM(a->tx_textures.reserve(rows.size()));
            return send_rows(a, rows, a->tx_textures.get(), 0, rows.size(), s);
        }
    }
    std::vector<DevTexture> rows(tex.size());
    rows[texture] = device_row(row, P.slots[texture]);
    return send_rows(a, rows, a->d_textures.get(), texture, 1, s);
}

// The host's dense texel bytes with texture `texture` resized to `row` (bytes from `rgb`, or left as they fall when the
// texels live on the device), and the table with the offsets that follow.  Same size: nothing is made, `same` says so.
struct HostTexels {
    bool same = false;
    std::vector<DevTexture> table;
    std::vector<uint8_t> pixels;
};
int host_texels(const rtk_accel *a, size_t texture, int32_t w, int32_t h, const uint8_t *rgb, HostTexels &H) {
    const std::vector<DevTexture> &tex = a->scene.textures;
    const size_t was = texel_bytes(tex[texture]), need = size_t(w) * size_t(h) * 3, at = size_t(tex[texture].bmp[2]);
    const std::vector<uint8_t> &old = a->scene.tex_pixels;
    if (old.size() - was + need > kTexelLimit) return fail(RTK_ERR_INVALID, "the texel bytes of all bitmaps must fit an int32 offset");
    H.same = tex[texture].bmp[0] == w && tex[texture].bmp[1] == h;
    if (H.same) return RTK_OK;
    H.table = tex;
    H.table[texture].bmp[0] = w; H.table[texture].bmp[1] = h;
    for (size_t i = 0; i < tex.size(); ++i)
        if (is_bitmap(tex[i]) && size_t(tex[i].bmp[2]) > at) H.table[i].bmp[2] = int32_t(size_t(tex[i].bmp[2]) - was + need);
    H.pixels.resize(old.size() - was + need);
    std::memcpy(H.pixels.data(), old.data(), at);
    if (rgb) std::memcpy(H.pixels.data() + at, rgb, need);
    std::memcpy(H.pixels.data() + at + need, old.data() + at + was, old.size() - at - was);
    return RTK_OK;
}

// the checks every texel setter makes before it looks at a device
int check_texel_call(const rtk_accel *a, int32_t texture, int32_t w, int32_t h) {
    if (texture < 0 || size_t(texture) >= a->scene.textures.size()) return fail(RTK_ERR_INVALID, "texture index out of range");
    if (!bitmap_size_ok(w, h)) return fail(RTK_ERR_INVALID, "bad bitmap texture size");
    if (!is_bitmap(a->scene.textures[size_t(texture)])) return fail(RTK_ERR_INVALID, "the texture is not a bitmap");
    return RTK_OK;
}

// nothing here fails: the host's picture after a texel setter
void adopt_texels(rtk_accel *a, size_t texture, HostTexels &H, const uint8_t *rgb, TexelPlan *P, bool on_device) {
    if (H.same) { if (rgb) std::memcpy(a->scene.tex_pixels.data() + a->scene.textures[texture].bmp[2], rgb, texel_bytes(a->scene.textures[texture])); }
    else { a->scene.textures.swap(H.table); a->scene.tex_pixels.swap(H.pixels); }
    if (!P) return;
    if (P->moved) { a->d_tex_pixels.swap(a->tx_pixels); a->d_textures.swap(a->tx_textures); }
    a->tx_slots.swap(P->slots); a->tx_used = P->used;
    a->tx_slots[texture].on_device = on_device;
}

// the two device variants: `write` puts the texels at the address it is given, on the stream
template <typename Write>
int set_texels_device(rtk_accel *a, int32_t texture, int32_t w, int32_t h, const void *d_src, hipStream_t s, Write write) {
    if (!a || !d_src) return fail(RTK_ERR_INVALID, "null accel or texels");
    std::lock_guard<std::mutex> lock(a->mu);
    RTK_TRY(check_texel_call(a, texture, w, h));
    HostTexels H;
    RTK_TRY(host_texels(a, size_t(texture), w, h, nullptr, H));
    RTK_TRY(ensure_device(a));
    RTK_HIP(a->geom_fence.quiesce());
    DevTexture row = a->scene.textures[size_t(texture)];
    row.bmp[0] = w; row.bmp[1] = h;
    TexelPlan P;
    RTK_TRY(place_texels(a, size_t(texture), row, size_t(w) * size_t(h) * 3, s, P));
    RTK_TRY(write(P.dst, s));
    RTK_HIP(a->geom_fence.publish(s));
    adopt_texels(a, size_t(texture), H, nullptr, &P, true);
    return RTK_OK;
}

}  // namespace

void rtk::dense_texture_slots(rtk_accel *a) {
    const std::vector<DevTexture> &tex = a->scene.textures;
    a->tx_slots.assign(tex.size(), rtk_accel::TexSlot{});
    for (size_t i = 0; i < tex.size(); ++i)
        if (is_bitmap(tex[i])) { a->tx_slots[i].off = tex[i].bmp[2]; a->tx_slots[i].cap = texel_bytes(tex[i]); }
    a->tx_used = a->scene.tex_pixels.size();
}

const std::vector<float> &rtk::host_vert_uv(rtk_accel *a) {
    if (a->vert_uv_made) return a->vert_uv;
    std::vector<float> uv(size_t(a->scene.n_vertices) * 2, 0.0f);          // kdtree.cpp:283-: a mesh without uvs has zeros
    size_t voff = 0;
    for (size_t mi = 0; mi < a->mesh_nverts.size(); ++mi) {
        const std::vector<float> &mu = a->scene.meshes[mi].uvs;
        const size_t n = std::min(mu.size(), size_t(a->mesh_nverts[mi]) * 2);
        if (n > 0) std::memcpy(uv.data() + voff * 2, mu.data(), n * sizeof(float));
        voff += size_t(a->mesh_nverts[mi]);
    }
    a->vert_uv.swap(uv);
    a->vert_uv_made = true;
    return a->vert_uv;
}

int rtk::ensure_vert_uv_dev(rtk_accel *a) {
    if (a->vert_uv_dev) return RTK_OK;
    const std::vector<float> &uv = host_vert_uv(a);
    RTK_MEM(a->topo_vert_uv.reserve(std::max<size_t>(2, uv.size())));
    if (!uv.empty()) RTK_HIP(hipMemcpy(a->topo_vert_uv.get(), uv.data(), uv.size() * sizeof(float), hipMemcpyHostToDevice));
    a->vert_uv_dev = true;
    return RTK_OK;
}

extern "C" {

int rtk_accel_get_lights(const rtk_accel *a, rtk_light *out, int32_t cap, int32_t *n) {
    return abi_guard([&]() -> int {
        if (!a || !n) return fail(RTK_ERR_INVALID, "null accel or count");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        const size_t have = a->scene.lights.size();
        *n = int32_t(have);
        const size_t take = (out && cap > 0) ? std::min(have, size_t(cap)) : 0;
        if (take == 0) return RTK_OK;
        if (a->lights_on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(hipDeviceSynchronize());
            RTK_HIP(hipMemcpy(out, a->d_lights.get(), take * sizeof(rtk_light), hipMemcpyDeviceToHost));
        } else std::memcpy(out, a->scene.lights.data(), take * sizeof(rtk_light));
        return RTK_OK;
    });
}

int rtk_accel_set_lights(rtk_accel *a, const rtk_light *lights, int32_t n) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        if (n < 0 || (n > 0 && !lights)) return fail(RTK_ERR_INVALID, "negative light count or null lights");
        std::lock_guard<std::mutex> lock(a->mu);
        std::vector<DevLight> table(static_cast<size_t>(n));
        if (n > 0) std::memcpy(table.data(), lights, size_t(n) * sizeof(DevLight));
        if (a->on_device) {
            RTK_HIP(hipSetDevice(a->device));
            // entry: nothing issued earlier on this accel, on whatever stream, may still read the table
            RTK_HIP(a->geom_fence.quiesce());
            RTK_TRY(reserve_lights(a, size_t(n)));
            if (n > 0) RTK_HIP(hipMemcpy(a->d_lights.get(), table.data(), size_t(n) * sizeof(DevLight), hipMemcpyHostToDevice));
        }
        const size_t before = a->scene.lights.size();
        a->scene.lights.swap(table);
        a->lights_on_device = false;
        lights_changed(a, before);
        return RTK_OK;
    });
}

int rtk_accel_set_lights_device(rtk_accel *a, const rtk_light *d_lights, int32_t n, void *hip_stream) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        if (n < 0 || (n > 0 && !d_lights)) return fail(RTK_ERR_INVALID, "negative light count or null lights");
        std::lock_guard<std::mutex> lock(a->mu);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        RTK_TRY(ensure_device(a));
        RTK_HIP(a->geom_fence.quiesce());
        RTK_TRY(reserve_lights(a, size_t(n)));
        std::vector<DevLight> count_only(static_cast<size_t>(n), DevLight{{0.f, 0.f, 0.f}, 0.f});
        if (n > 0) RTK_HIP(hipMemcpyAsync(a->d_lights.get(), d_lights, size_t(n) * sizeof(DevLight), hipMemcpyDeviceToDevice, s));
        RTK_HIP(a->geom_fence.publish(s));
        const size_t before = a->scene.lights.size();
        a->scene.lights.swap(count_only);              // the COUNT every launch path reads; the values live in d_lights
        a->lights_on_device = true;
        lights_changed(a, before);
        return RTK_OK;
    });
}

int rtk_accel_get_materials(const rtk_accel *a, rtk_material *out) {
    return abi_guard([&]() -> int {
        if (!a || !out) return fail(RTK_ERR_INVALID, "null accel or materials");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        if (!a->scene.materials.empty()) std::memcpy(out, a->scene.materials.data(), a->scene.materials.size() * sizeof(rtk_material));
        return RTK_OK;
    });
}

int rtk_accel_set_materials(rtk_accel *a, const rtk_material *materials, int32_t n) {
    return abi_guard([&]() -> int {
        if (!a || !materials) return fail(RTK_ERR_INVALID, "null accel or materials");
        std::lock_guard<std::mutex> lock(a->mu);
        if (n < 0 || size_t(n) != a->scene.materials.size()) return fail(RTK_ERR_INVALID, "the number of materials is fixed when the scene is made");
        // scene.cpp, scene_from_desc
        std::vector<DevMaterial> table(static_cast<size_t>(n));
        for (size_t i = 0; i < table.size(); ++i) {
            DevMaterial &m = table[i];
            std::memcpy(&m, &materials[i], sizeof(m));
            if (m.kind < RTK_MAT_DIFFUSE || m.kind > RTK_MAT_TEXTURE) return fail(RTK_ERR_INVALID, "material type unknown");
            if (m.kind == RTK_MAT_TEXTURE) {
                if (m.texture < 0 || size_t(m.texture) >= a->scene.textures.size()) return fail(RTK_ERR_INVALID, "texture material refers to a texture that does not exist");
            } else m.texture = -1;
            m.pad = 0u;
        }
        if (a->on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(a->geom_fence.quiesce());
            // the new table goes into the spare one, what follows from it is built beside what is active, and both are swapped in at the end
            RTK_MEM(a->st_materials.reserve(table.size()));             // (once: the number of materials is fixed)
            if (!table.empty()) RTK_HIP(hipMemcpy(a->st_materials.get(), table.data(), table.size() * sizeof(DevMaterial), hipMemcpyHostToDevice));
            RTK_TRY(remake_occluders(a, table, a->st_materials.get(), nullptr));
            a->d_materials.swap(a->st_materials);
        }
        a->scene.materials.swap(table);
        a->has_refractive = any_refractive(a->scene.materials);
        // a scene that starts or stops forking runs other kernels over other block costs, and needs a new verdict
        forget_orders(a);
        return RTK_OK;
    });
}

int rtk_accel_get_background(const rtk_accel *a, float rgb[3]) {
    return abi_guard([&]() -> int {
        if (!a || !rgb) return fail(RTK_ERR_INVALID, "null accel or colour");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        std::memcpy(rgb, a->scene.background, sizeof(a->scene.background));
        return RTK_OK;
    });
}

int rtk_accel_set_background(rtk_accel *a, const float rgb[3]) {
    return abi_guard([&]() -> int {
        if (!a || !rgb) return fail(RTK_ERR_INVALID, "null accel or colour");
        std::lock_guard<std::mutex> lock(a->mu);
        std::memcpy(a->scene.background, rgb, sizeof(a->scene.background));
        return RTK_OK;
    });
}

// ---------------------------------------------------------------- textures and uvs of a live accel

int rtk_accel_get_textures(const rtk_accel *a, rtk_texture *out, int32_t cap, int32_t *n) {
    return abi_guard([&]() -> int {
        if (!a || !n) return fail(RTK_ERR_INVALID, "null accel or count");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        const std::vector<DevTexture> &tex = a->scene.textures;
        *n = int32_t(tex.size());
        const size_t take = (out && cap > 0) ? std::min(tex.size(), size_t(cap)) : 0;
        for (size_t i = 0; i < take; ++i) {
            rtk_texture t{};
            t.kind = tex[i].kind;
            if (is_bitmap(tex[i])) { t.width = tex[i].bmp[0]; t.height = tex[i].bmp[1]; }
            else { std::memcpy(t.color_a, tex[i].a, sizeof(t.color_a)); std::memcpy(t.color_b, tex[i].b, sizeof(t.color_b)); t.param = tex[i].param; }
            out[i] = t;
        }
        return RTK_OK;
    });
}

int rtk_accel_get_texture_pixels(const rtk_accel *a, int32_t texture, uint8_t *out, size_t cap, size_t *n_bytes) {
    return abi_guard([&]() -> int {
        if (!a || !n_bytes) return fail(RTK_ERR_INVALID, "null accel or size");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        if (texture < 0 || size_t(texture) >= a->scene.textures.size()) return fail(RTK_ERR_INVALID, "texture index out of range");
        const DevTexture &t = a->scene.textures[size_t(texture)];
        *n_bytes = texel_bytes(t);
        const size_t take = out ? std::min(*n_bytes, cap) : 0;
        if (take == 0) return RTK_OK;
        if (a->on_device && a->tx_slots[size_t(texture)].on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(hipDeviceSynchronize());
            RTK_HIP(hipMemcpy(out, a->d_tex_pixels.get() + a->tx_slots[size_t(texture)].off, take, hipMemcpyDeviceToHost));
        } else std::memcpy(out, a->scene.tex_pixels.data() + t.bmp[2], take);
        return RTK_OK;
    });
}

int rtk_accel_set_textures(rtk_accel *a, const rtk_texture *textures, int32_t n, const uint8_t *const *pixels) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        if (n < 0 || (n > 0 && !textures)) return fail(RTK_ERR_INVALID, "negative texture count or null textures");
        std::lock_guard<std::mutex> lock(a->mu);
        // scene.cpp, scene_from_desc: the dense table and texel bytes of the host
        std::vector<DevTexture> table(static_cast<size_t>(n));
        size_t total = 0;
        for (size_t i = 0; i < table.size(); ++i) {
            DevTexture &t = table[i];
            std::memset(&t, 0, sizeof(t));
            t.kind = textures[i].kind;
            if (t.kind < RTK_TEX_ALBEDO || t.kind > RTK_TEX_BITMAP) return fail(RTK_ERR_INVALID, "texture type unknown");
            if (is_bitmap(t)) {
                if (!bitmap_size_ok(textures[i].width, textures[i].height)) return fail(RTK_ERR_INVALID, "bad bitmap texture size");
                if (!pixels || !pixels[i]) return fail(RTK_ERR_INVALID, "bitmap texture without pixels");
                t.bmp[0] = textures[i].width; t.bmp[1] = textures[i].height; t.bmp[2] = int32_t(total);
                total += texel_bytes(t);
                if (total > kTexelLimit) return fail(RTK_ERR_INVALID, "the texel bytes of all bitmaps must fit an int32 offset");
                continue;
            }
            std::memcpy(t.a, textures[i].color_a, sizeof(t.a)); std::memcpy(t.b, textures[i].color_b, sizeof(t.b));
            t.param = textures[i].param;
        }
        for (const DevMaterial &m : a->scene.materials)
            if (m.kind == RTK_MAT_TEXTURE && (m.texture < 0 || size_t(m.texture) >= table.size()))
                return fail(RTK_ERR_INVALID, "a texture material refers to a texture the new table does not have: change the materials first");
        std::vector<uint8_t> texels(total);
        for (size_t i = 0; i < table.size(); ++i)
            if (is_bitmap(table[i])) std::memcpy(texels.data() + table[i].bmp[2], pixels[i], texel_bytes(table[i]));
        const bool first = a->scene.textures.empty() && !table.empty();     // from none to some: the per-triangle uvs do not exist yet
        std::vector<DevTriUv> tri_uv;
        std::vector<rtk_accel::TexSlot> slots(table.size());
        size_t used = 0;
        if (a->on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(a->geom_fence.quiesce());
            // table and texels go into the spare buffers, every bitmap into an aligned slot, and are swapped in at the end
            std::vector<DevTexture> rows(table.size());
            for (size_t i = 0; i < table.size(); ++i) {
                if (is_bitmap(table[i])) { slots[i].off = int32_t(used); slots[i].cap = slot_round(texel_bytes(table[i])); used += slots[i].cap; }
                if (used > kTexelLimit) return fail(RTK_ERR_INVALID, "the texel bytes of all bitmaps must fit an int32 offset");
                rows[i] = device_row(table[i], slots[i]);
            }
            RTK_MEM(a->tx_textures.reserve(std::max<size_t>(1, rows.size())));
            if (!rows.empty()) RTK_HIP(hipMemcpy(a->tx_textures.get(), rows.data(), rows.size() * sizeof(DevTexture), hipMemcpyHostToDevice));
            if (used > 0) RTK_MEM(a->tx_pixels.reserve(used, grow_bytes()));
            for (size_t i = 0; i < table.size(); ++i)
                if (is_bitmap(table[i])) RTK_HIP(hipMemcpy(a->tx_pixels.get() + slots[i].off, pixels[i], texel_bytes(table[i]), hipMemcpyHostToDevice));
            if (first) {
                RTK_TRY(ensure_vert_uv_dev(a));
                RTK_TRY(make_tri_uv(a, nullptr));
                RTK_HIP(a->geom_fence.publish(nullptr));
            }
        } else if (first) host_tri_uv(a, host_vert_uv(a), tri_uv);
        // ---- nothing below fails
        if (a->on_device) {
            a->d_textures.swap(a->tx_textures);
            if (used > 0) a->d_tex_pixels.swap(a->tx_pixels);
            if (first) a->topo.tri_uv.swap(a->topo_spare.tri_uv);
            a->tx_slots.swap(slots); a->tx_used = used;
        } else if (first) a->tree.dev_tri_uv.swap(tri_uv);
        a->scene.textures.swap(table);
        a->scene.tex_pixels.swap(texels);
        return RTK_OK;
    });
}

int rtk_accel_set_texture_pixels(rtk_accel *a, int32_t texture, int32_t width, int32_t height, const uint8_t *rgb) {
    return abi_guard([&]() -> int {
        if (!a || !rgb) return fail(RTK_ERR_INVALID, "null accel or texels");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(check_texel_call(a, texture, width, height));
        HostTexels H;
        RTK_TRY(host_texels(a, size_t(texture), width, height, rgb, H));
        if (!a->on_device) { adopt_texels(a, size_t(texture), H, rgb, nullptr, false); return RTK_OK; }
        RTK_HIP(hipSetDevice(a->device));
        RTK_HIP(a->geom_fence.quiesce());
        DevTexture row = a->scene.textures[size_t(texture)];
        row.bmp[0] = width; row.bmp[1] = height;
        const size_t need = size_t(width) * size_t(height) * 3;
        TexelPlan P;
        RTK_TRY(place_texels(a, size_t(texture), row, need, nullptr, P));
        RTK_HIP(hipMemcpy(P.dst, rgb, need, hipMemcpyHostToDevice));
        RTK_HIP(hipStreamSynchronize(nullptr));                             // (the table row left through the pinned stage)
        adopt_texels(a, size_t(texture), H, rgb, &P, false);
        return RTK_OK;
    });
}

int rtk_accel_set_texture_pixels_device(rtk_accel *a, int32_t texture, int32_t width, int32_t height, const uint8_t *d_rgb, void *hip_stream) {
    return abi_guard([&]() -> int {
        const size_t need = size_t(width) * size_t(height) * 3;             // (used once the size has been judged)
        return set_texels_device(a, texture, width, height, d_rgb, static_cast<hipStream_t>(hip_stream), [&](uint8_t *dst, hipStream_t s) -> int {
            RTK_HIP(hipMemcpyAsync(dst, d_rgb, need, hipMemcpyDeviceToDevice, s));
            return RTK_OK;
        });
    });
}

int rtk_accel_set_texture_frame_device(rtk_accel *a, int32_t texture, int32_t width, int32_t height, const float *d_rgb, void *hip_stream) {
    return abi_guard([&]() -> int {
        const size_t need = size_t(width) * size_t(height) * 3;
        return set_texels_device(a, texture, width, height, d_rgb, static_cast<hipStream_t>(hip_stream), [&](uint8_t *dst, hipStream_t s) -> int {
            RTK_HIP_AS(launch_frame_to_texels(d_rgb, need, dst, s), "launch k_frame_to_texels");
            return RTK_OK;
        });
    });
}

int rtk_accel_get_uvs(const rtk_accel *a, float *uvs) {
    return abi_guard([&]() -> int {
        if (!a || !uvs) return fail(RTK_ERR_INVALID, "null accel or uvs");
        rtk_accel *w = const_cast<rtk_accel *>(a);                          // (the dense array is made on first use)
        std::lock_guard<std::mutex> lock(w->mu);
        const size_t n = size_t(a->scene.n_vertices) * 2;
        if (n == 0) return RTK_OK;
        if (a->uvs_on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(hipDeviceSynchronize());
            RTK_HIP(hipMemcpy(uvs, a->topo_vert_uv.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        } else std::memcpy(uvs, host_vert_uv(w).data(), n * sizeof(float));
        return RTK_OK;
    });
}

int rtk_accel_set_uvs(rtk_accel *a, const float *uvs) {
    return abi_guard([&]() -> int {
        if (!a || !uvs) return fail(RTK_ERR_INVALID, "null accel or uvs");
        std::lock_guard<std::mutex> lock(a->mu);
        const size_t n = size_t(a->scene.n_vertices) * 2;
        std::vector<float> uv(uvs, uvs + n);
        const bool textured = !a->scene.textures.empty();
        std::vector<DevTriUv> tri_uv;
        if (a->on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(a->geom_fence.quiesce());
            RTK_MEM(a->topo_vert_uv.reserve(std::max<size_t>(2, n)));       // (once: the vertex count never changes)
            a->vert_uv_dev = false;
            if (n > 0) RTK_HIP(hipMemcpy(a->topo_vert_uv.get(), uv.data(), n * sizeof(float), hipMemcpyHostToDevice));
            if (textured) {
                RTK_TRY(make_tri_uv(a, nullptr));
                RTK_HIP(a->geom_fence.publish(nullptr));
                a->topo.tri_uv.swap(a->topo_spare.tri_uv);
            }
            a->vert_uv_dev = true;
        } else if (textured) host_tri_uv(a, uv, tri_uv);
        if (!a->on_device && textured) a->tree.dev_tri_uv.swap(tri_uv);
        a->vert_uv.swap(uv);
        a->vert_uv_made = true;
        a->uvs_on_device = false;
        return RTK_OK;
    });
}

int rtk_accel_set_uvs_device(rtk_accel *a, const float *d_uvs, void *hip_stream) {
    return abi_guard([&]() -> int {
        if (!a || !d_uvs) return fail(RTK_ERR_INVALID, "null accel or uvs");
        std::lock_guard<std::mutex> lock(a->mu);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        RTK_TRY(ensure_device(a));
        RTK_HIP(a->geom_fence.quiesce());
        const size_t n = size_t(a->scene.n_vertices) * 2;
        const bool textured = !a->scene.textures.empty();
        RTK_MEM(a->topo_vert_uv.reserve(std::max<size_t>(2, n)));
        if (textured) RTK_TRY(ensure_update_static(a));                     // (the one blocking step, on an accel no update has touched)
        a->vert_uv_dev = false;
        if (n > 0) RTK_HIP(hipMemcpyAsync(a->topo_vert_uv.get(), d_uvs, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (textured) RTK_TRY(make_tri_uv(a, s));
        RTK_HIP(a->geom_fence.publish(s));
        if (textured) a->topo.tri_uv.swap(a->topo_spare.tri_uv);
        a->vert_uv_dev = true;
        a->uvs_on_device = true;                                            // (the host's copy is stale: the getter fetches)
        return RTK_OK;
    });
}

}  // extern "C"
