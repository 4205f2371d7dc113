// C-ABI of the rtk engine (include/rtk.h).  Owns device buffers, validates operands against what the
// kernels and their grids assume, and never lets an exception cross the boundary: every entry point of api*.hip that returns a
// status runs its body through abi_guard (abi_guard.hpp).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

#include "accel.hpp"

namespace rtk {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

int ensure_device(rtk_accel *a, hipStream_t s) {
    if (a->on_device) {
        RTK_HIP(hipSetDevice(a->device));
        RTK_HIP(a->geom_fence.wait(s));
        return RTK_OK;
    }
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(RTK_ERR_NO_DEVICE, "no usable HIP device (this engine has no CPU path)");
    int dev = a->params.device;
    if (dev < 0) RTK_HIP(hipGetDevice(&dev));
    if (dev >= count) return fail(RTK_ERR_INVALID, "device ordinal out of range");
    RTK_HIP(hipSetDevice(dev));
    a->device = dev;
    // (a retry after a failure part-way finds what the first attempt uploaded in its buffers, and uploads into them again)
    GeomBufs &G = a->geom;
    RTK_TRY(upload(a->tree.dev_nodes, G.nodes));
    RTK_TRY(upload(a->tree.dev_leaves, G.leaves));
    if (a->fast_traversal) RTK_TRY(upload(a->tree.dev_leaves_fast, G.leaves_fast));
    RTK_TRY(upload(a->tree.dev_tris, G.tris));
    RTK_TRY(upload(a->tree.dev_tri_ids, G.tri_ids));
    RTK_TRY(upload(a->tree.dev_shade, G.shade));
    if (a->fast_traversal && a->has_refractive && a->knobs.fast_occluders) {
        HostOccluders o;                                                    // the second tree of RTK_TRAVERSAL_FAST (update_plan.hpp)
        if (const char *why = host_occluders(a->tree, a->scene.materials, o)) return fail(RTK_ERR_INVALID, why);
        RTK_TRY(upload(o.tree.nodes, G.occl_nodes));
        RTK_TRY(upload(o.tree.leaves, G.occl_leaves));
        RTK_TRY(upload(o.tris, G.occl_tris));
        RTK_TRY(upload(o.ids, G.occl_ids));
        a->occl_n_leaves = uint32_t(o.tree.leaves.size());
        a->occl_on = true;
    }
    RTK_TRY(upload(a->scene.materials, a->d_materials));
    RTK_TRY(upload(a->scene.lights, a->d_lights));
    if (!a->scene.textures.empty()) {
        RTK_TRY(upload(a->scene.textures, a->d_textures));
        RTK_TRY(upload(a->tree.dev_tri_uv, a->topo.tri_uv));
        if (!a->scene.tex_pixels.empty()) RTK_TRY(upload(a->scene.tex_pixels, a->d_tex_pixels));
    }
    dense_texture_slots(a);
    RTK_MEM(a->d_counters.reserve(2 * kCounterAllocWords));                 // (two blocks of the counters and their tail: counters.hpp, accel.hpp)
    RTK_HIP(hipMemset(a->d_counters.get(), 0, 2 * kCounterAllocWords * sizeof(unsigned long long)));
    a->cnt = CounterState{};
    a->on_device = true;
    return RTK_OK;
}

dev::TreeView tree_view(const rtk_accel *a) {
    dev::TreeView t;
    const GeomBufs &G = a->geom;
    t.nodes = G.nodes.get(); t.tris = G.tris.get(); t.tri_ids = G.tri_ids.get(); t.shade = G.shade.get();
    t.leaves = G.leaves.get(); t.n_leaves = static_cast<uint32_t>(a->tree.dev_leaves.size());
    t.leaves_fast = a->fast_traversal ? G.leaves_fast.get() : nullptr;
    t.n_nodes = static_cast<uint32_t>(a->tree.dev_nodes.size());
    t.eps = a->params.eps;
    t.normalize = a->params.normalize_hit_normal;
    t.bundle_cull = (a->knobs.bundle_cull && a->coords_small) ? 1 : 0;
    t.scalar_surv = 0;
    return t;
}

}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_abi_version(void) { return RTK_ABI_VERSION; }

const char *rtk_last_error(void) { return g_last_error.c_str(); }

int rtk_device_count(int *count) {
    return abi_guard([&]() -> int {
        if (!count) return fail(RTK_ERR_INVALID, "null count");
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        *count = n;
        return RTK_OK;
    });
}

// ---------------------------------------------------------------- scene

int rtk_scene_create(const rtk_scene_desc *desc, rtk_scene **out) {
    return abi_guard([&]() -> int {
        if (!desc || !out) return fail(RTK_ERR_INVALID, "null desc or out");
        *out = nullptr;
        rtk_scene *s = new rtk_scene();
        std::string err;
        const int rc = scene_from_desc(*desc, *s, err);
        if (rc != RTK_OK) { delete s; return fail(rc, err); }
        *out = s;
        return RTK_OK;
    });
}

int rtk_scene_load_crtscene(const char *path, rtk_scene **out) {
    return abi_guard([&]() -> int {
        if (!path || !out) return fail(RTK_ERR_INVALID, "null path or out");
        *out = nullptr;
        rtk_scene *s = new rtk_scene();
        std::string err;
        const int rc = scene_from_crtscene(path, *s, err);
        if (rc != RTK_OK) { delete s; return fail(rc, err); }
        *out = s;
        return RTK_OK;
    });
}

int rtk_scene_get_info(const rtk_scene *s, rtk_scene_info *info) {
    return abi_guard([&]() -> int {
        if (!s || !info) return fail(RTK_ERR_INVALID, "null scene or info");
        info->n_meshes = int32_t(s->meshes.size());
        info->n_materials = int32_t(s->materials.size());
        info->n_lights = int32_t(s->lights.size());
        info->n_vertices = s->n_vertices;
        info->n_triangles = s->n_triangles;
        info->width = s->width; info->height = s->height; info->bucket_size = s->bucket_size;
        info->n_textures = int32_t(s->textures.size());
        info->n_uv_vertices = 0;
        for (const HostMesh &m : s->meshes) info->n_uv_vertices += int32_t(m.uvs.size() / 2);
        info->n_bitmap_bytes = int32_t(s->tex_pixels.size());
        return RTK_OK;
    });
}

int rtk_scene_get_arrays(const rtk_scene *s, int32_t *mesh_material, int32_t *mesh_nverts, int32_t *mesh_ntris,
                         float *vertices, uint32_t *indices, int32_t *mat_kind, float *mat_albedo, float *mat_ior,
                         int32_t *mat_smooth, float *light_pos, float *light_intensity, float *cam_pos, float *cam_mat,
                         float *background) {
    return abi_guard([&]() -> int {
        if (!s) return fail(RTK_ERR_INVALID, "null scene");
        size_t vo = 0, to = 0;
        for (size_t m = 0; m < s->meshes.size(); ++m) {
            const HostMesh &hm = s->meshes[m];
            if (mesh_material) mesh_material[m] = hm.material;
            if (mesh_nverts) mesh_nverts[m] = int32_t(hm.vertices.size());
            if (mesh_ntris) mesh_ntris[m] = int32_t(hm.indices.size() / 3);
            if (vertices) for (size_t i = 0; i < hm.vertices.size(); ++i) {
                vertices[(vo + i) * 3] = hm.vertices[i].x; vertices[(vo + i) * 3 + 1] = hm.vertices[i].y; vertices[(vo + i) * 3 + 2] = hm.vertices[i].z;
            }
            if (indices && !hm.indices.empty()) std::memcpy(indices + to * 3, hm.indices.data(), hm.indices.size() * sizeof(uint32_t));
            vo += hm.vertices.size(); to += hm.indices.size() / 3;
        }
        for (size_t i = 0; i < s->materials.size(); ++i) {
            if (mat_kind) mat_kind[i] = s->materials[i].kind;
            if (mat_albedo) std::memcpy(mat_albedo + i * 3, s->materials[i].albedo, 3 * sizeof(float));
            if (mat_ior) mat_ior[i] = s->materials[i].ior;
            if (mat_smooth) mat_smooth[i] = s->materials[i].smooth;
        }
        for (size_t i = 0; i < s->lights.size(); ++i) {
            if (light_pos) std::memcpy(light_pos + i * 3, s->lights[i].pos, 3 * sizeof(float));
            if (light_intensity) light_intensity[i] = s->lights[i].intensity;
        }
        if (cam_pos) std::memcpy(cam_pos, s->cam_pos, sizeof(s->cam_pos));
        if (cam_mat) std::memcpy(cam_mat, s->cam_mat, sizeof(s->cam_mat));
        if (background) std::memcpy(background, s->background, sizeof(s->background));
        return RTK_OK;
    });
}

int rtk_scene_get_textures(const rtk_scene *s, int32_t *mat_texture, int32_t *mesh_has_uvs, float *uvs, int32_t *tex_kind,
                           float *tex_color_a, float *tex_color_b, float *tex_param) {
    return abi_guard([&]() -> int {
        if (!s) return fail(RTK_ERR_INVALID, "null scene");
        for (size_t i = 0; i < s->materials.size(); ++i) if (mat_texture) mat_texture[i] = s->materials[i].texture;
        size_t uo = 0;
        for (size_t m = 0; m < s->meshes.size(); ++m) {
            const HostMesh &hm = s->meshes[m];
            if (mesh_has_uvs) mesh_has_uvs[m] = hm.uvs.empty() ? 0 : 1;
            if (uvs && !hm.uvs.empty()) std::memcpy(uvs + uo, hm.uvs.data(), hm.uvs.size() * sizeof(float));
            uo += hm.uvs.size();
        }
        for (size_t i = 0; i < s->textures.size(); ++i) {
            if (tex_kind) tex_kind[i] = s->textures[i].kind;
            const bool bmp = s->textures[i].kind == RTK_TEX_BITMAP;
            const float zero[3] = {0.f, 0.f, 0.f};
            if (tex_color_a) std::memcpy(tex_color_a + i * 3, bmp ? zero : s->textures[i].a, 3 * sizeof(float));
            if (tex_color_b) std::memcpy(tex_color_b + i * 3, s->textures[i].b, 3 * sizeof(float));
            if (tex_param) tex_param[i] = s->textures[i].param;
        }
        return RTK_OK;
    });
}

int rtk_scene_get_bitmaps(const rtk_scene *s, int32_t *tex_bitmap, uint8_t *tex_pixels) {
    return abi_guard([&]() -> int {
        if (!s) return fail(RTK_ERR_INVALID, "null scene");
        for (size_t i = 0; i < s->textures.size(); ++i) {
            if (!tex_bitmap) break;
            const DevTexture &t = s->textures[i];
            const bool bmp = t.kind == RTK_TEX_BITMAP;
            tex_bitmap[i * 3] = bmp ? t.bmp[2] : 0; tex_bitmap[i * 3 + 1] = bmp ? t.bmp[0] : 0; tex_bitmap[i * 3 + 2] = bmp ? t.bmp[1] : 0;
        }
        if (tex_pixels && !s->tex_pixels.empty()) std::memcpy(tex_pixels, s->tex_pixels.data(), s->tex_pixels.size());
        return RTK_OK;
    });
}

int rtk_decode_jpeg(const uint8_t *data, size_t size, int32_t *width, int32_t *height, int32_t *channels, uint8_t *pixels, size_t cap) {
    return abi_guard([&]() -> int {
        if (!data || !width || !height || !channels) return fail(RTK_ERR_INVALID, "null argument");
        std::vector<uint8_t> px;
        std::string err;
        int w = 0, h = 0, ch = 0;
        const int rc = decode_jpeg(data, size, w, h, ch, px, err);
        if (rc != RTK_OK) return fail(rc, err);
        *width = w; *height = h; *channels = ch;
        if (pixels) std::memcpy(pixels, px.data(), px.size() < cap ? px.size() : cap);
        return RTK_OK;
    });
}

int rtk_scene_vertex_normals(const rtk_scene *s, int32_t mesh, float *out) {
    return abi_guard([&]() -> int {
        if (!s || !out) return fail(RTK_ERR_INVALID, "null scene or out");
        if (mesh < 0 || size_t(mesh) >= s->meshes.size()) return fail(RTK_ERR_INVALID, "mesh index out of range");
        const HostMesh &hm = s->meshes[size_t(mesh)];
        for (size_t i = 0; i < hm.vertex_normals.size(); ++i) {
            out[i * 3] = hm.vertex_normals[i].x; out[i * 3 + 1] = hm.vertex_normals[i].y; out[i * 3 + 2] = hm.vertex_normals[i].z;
        }
        return RTK_OK;
    });
}

void rtk_scene_destroy(rtk_scene *s) { delete s; }

// ---------------------------------------------------------------- accel

int rtk_accel_build(const rtk_scene *scene, const rtk_accel_params *params, rtk_accel **out) {
    return abi_guard([&]() -> int {
        if (!scene || !out) return fail(RTK_ERR_INVALID, "null scene or out");
        *out = nullptr;
        rtk_accel *a = new rtk_accel();
        a->scene = *scene;
        if (params) a->params = *params;
        else { a->params.max_depth = 8; a->params.max_leaf_size = 64; a->params.eps = 1e-6f; a->params.normalize_hit_normal = 1; a->params.device = -1; a->params.traversal = RTK_TRAVERSAL_REFERENCE; }
        if (a->params.traversal != RTK_TRAVERSAL_REFERENCE && a->params.traversal != RTK_TRAVERSAL_FAST) { delete a; return fail(RTK_ERR_INVALID, "unknown traversal"); }
        std::string err;
        const int rc = build_tree(a->scene, a->params.max_depth, a->params.max_leaf_size, a->tree, err);
        if (rc != RTK_OK) { delete a; return fail(rc, err); }
        if (a->tree.dev_nodes.size() > 0x7FFFFFFFull || a->tree.dev_tris.size() > 0x7FFFFFFFull) {
            delete a; return fail(RTK_ERR_INVALID, "tree too large for 32-bit node/triangle indices");
        }
        // eps: the reciprocal-estimate prefilter of tri_step and the bundle culling both assume that a determinant which
        // passes `eps <= |det|` is a normal float with a finite reciprocal
        if (!(a->params.eps >= 1.17549435e-38f && a->params.eps < 1.0f)) {
            delete a; return fail(RTK_ERR_INVALID, "eps must be in [FLT_MIN, 1)");
        }
        a->has_refractive = any_refractive(a->scene.materials);
        for (const HostMesh &m : a->scene.meshes) { a->mesh_nverts.push_back(int32_t(m.vertices.size())); a->mesh_ntris.push_back(int32_t(m.indices.size() / 3)); }
        a->knobs = rtk_knobs::from_env();
        a->stream_slices_auto = stream_slices_for(a->tree);
        a->fast_traversal = a->params.traversal == RTK_TRAVERSAL_FAST || a->knobs.traversal_fast;
        if (a->fast_traversal) build_fast_leaf_orders(a->tree);
        a->coords_small = true;
        for (const DevTri &t : a->tree.dev_tris)
            for (int k = 0; k < 3; ++k)
                if (!(std::fabs(t.v0[k]) <= dev::kBundleLimit && std::fabs(t.e1[k]) <= dev::kBundleLimit && std::fabs(t.e2[k]) <= dev::kBundleLimit))
                    a->coords_small = false;
        *out = a;
        return RTK_OK;
    });
}

int rtk_accel_tree_info(const rtk_accel *a, rtk_tree_info *info) {
    return abi_guard([&]() -> int {
        if (!a || !info) return fail(RTK_ERR_INVALID, "null accel or info");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        std::memset(info, 0, sizeof(*info));
        info->n_nodes = int32_t(a->tree.nodes.size());
        for (const HostNode &n : a->tree.nodes) {
            if (n.leaf_start >= 0) { info->n_leaves += 1; if (n.leaf_count > info->max_leaf_refs) info->max_leaf_refs = n.leaf_count; }
            else info->n_inner += 1;
        }
        // (after rtk_accel_update_vertices / _update_geometry the per-triangle and per-reference arrays live on the device only, and
        // scene.n_triangles is the count of the last triangle lists)
        info->n_leaf_refs = a->refs_on_device ? a->n_leaf_refs_dev : int32_t(a->tree.leaf_refs.size());
        info->n_triangles = a->refs_on_device ? a->scene.n_triangles : int32_t(a->tree.triangles.size());
        info->tree_depth = a->tree.depth;
        return RTK_OK;
    });
}

int rtk_accel_tree_dump(const rtk_accel *a, float *nodes_box, int32_t *nodes_link, int32_t *leaf_refs) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);      // (an update on another thread swaps the tree)
        for (size_t i = 0; i < a->tree.nodes.size(); ++i) {
            const HostNode &n = a->tree.nodes[i];
            if (nodes_box) {
                float *b = nodes_box + i * 6;
                b[0] = n.box.mn.x; b[1] = n.box.mn.y; b[2] = n.box.mn.z; b[3] = n.box.mx.x; b[4] = n.box.mx.y; b[5] = n.box.mx.z;
            }
            if (nodes_link) {
                int32_t *l = nodes_link + i * 4;
                l[0] = n.child0; l[1] = n.child1; l[2] = n.leaf_start; l[3] = n.leaf_count;
            }
        }
        if (leaf_refs && a->refs_on_device) {
            // the device build wrote them (build.hip, k_build_gather): fetched when someone asks
            if (a->n_leaf_refs_dev > 0) {
                RTK_HIP(hipSetDevice(a->device));
                RTK_HIP(a->geom_fence.sync_host());
                RTK_HIP(hipMemcpy(leaf_refs, a->geom.leaf_refs.get(), size_t(a->n_leaf_refs_dev) * sizeof(int32_t), hipMemcpyDeviceToHost));
            }
        } else if (leaf_refs && !a->tree.leaf_refs.empty())
            std::memcpy(leaf_refs, a->tree.leaf_refs.data(), a->tree.leaf_refs.size() * sizeof(int32_t));
        return RTK_OK;
    });
}

void rtk_accel_destroy(rtk_accel *a) {
    if (!a) return;
    delete a;           // (~rtk_accel selects the device; the members free what they own)
}

// ---------------------------------------------------------------- image out

int rtk_format_ppm(const float *rgb, int32_t width, int32_t height, char *buf, size_t cap, size_t *n) {
    return abi_guard([&]() -> int {
        if (!rgb || !n || width <= 0 || height <= 0) return fail(RTK_ERR_INVALID, "bad image");
        const std::string s = format_ppm(rgb, width, height);
        *n = s.size();
        if (buf) std::memcpy(buf, s.data(), s.size() < cap ? s.size() : cap);
        return RTK_OK;
    });
}

int rtk_frame_to_rgb8_device(const float *d_rgb, size_t n, uint8_t *d_out, void *stream) {
    return abi_guard([&]() -> int {
        if (n > 0 && (!d_rgb || !d_out)) return fail(RTK_ERR_INVALID, "null buffer");
        if (n > (size_t(1) << 38)) return fail(RTK_ERR_INVALID, "too many values for one launch");
        RTK_HIP_AS(launch_to_rgb8(d_rgb, n, d_out, static_cast<hipStream_t>(stream)), "launch k_to_rgb8");
        return RTK_OK;
    });
}

int rtk_format_ppm_rgb8(const uint8_t *rgb8, int32_t width, int32_t height, char *buf, size_t cap, size_t *n) {
    return abi_guard([&]() -> int {
        if (!rgb8 || !n || width <= 0 || height <= 0) return fail(RTK_ERR_INVALID, "bad image");
        const std::string s = format_ppm_rgb8(rgb8, width, height);
        *n = s.size();
        if (buf) std::memcpy(buf, s.data(), s.size() < cap ? s.size() : cap);
        return RTK_OK;
    });
}

int rtk_write_ppm(const float *rgb, int32_t width, int32_t height, const char *path) {
    return abi_guard([&]() -> int {
        if (!rgb || !path || width <= 0 || height <= 0) return fail(RTK_ERR_INVALID, "bad image or path");
        const std::string s = format_ppm(rgb, width, height);
        std::FILE *f = std::fopen(path, "wb");
        if (!f) return fail(RTK_ERR_IO, std::string("cannot open ") + path);
        const size_t w = std::fwrite(s.data(), 1, s.size(), f);
        const int c = std::fclose(f);
        if (w != s.size() || c != 0) return fail(RTK_ERR_IO, std::string("short write to ") + path);
        return RTK_OK;
    });
}

}  // extern "C"
