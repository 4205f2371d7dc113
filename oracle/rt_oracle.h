/*
 * rt_oracle.h — CPU restatement of the reference's kd-tree traversal / leaf-packet
 * Möller–Trumbore / render-loop hot path (SURVEY.md §8a rows a1–a16).
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this library.  The shipped path
 * (simd-raytracer_amd/) never links, imports or calls anything in oracle/.
 *
 * PARITY PIN STATUS: PINNED, bit for bit, by a build of the reference's own headers: oracle/ref_probe.cpp (recipe
 * oracle/ref.mk, stand-ins for the missing C++23 library pieces in oracle/ref_shim/) answers tree, intersect, occluded,
 * radiance and frame queries; tests/test_ref_probe.py compares this restatement with the arrays it recorded
 * (tests/golden/ref_probe/) and, where the build exists, with the probe itself over every loadable scene, generated scenes,
 * tree shapes, eps values, packet widths 4 / 8 / 16 and the scalar kd-tree.  Not covered there: the scene loader, the JPEG
 * decode (tests/golden/jpeg/), GI and multi-sample frames (the reference's RNG is a race).
 * Also pinned by the reference's own committed renders: its outputs (PNG conversions of its image.ppm files, README.md:43-68),
 * decoded into tests/golden/ref_outputs/, are golden frames:
 *   - refractive_dragon.png (hw11/scene8, 1920x1080): this restatement's write_ppm bytes are
 *     equal on all 6,220,800 bytes (tests/test_reference_outputs.py);
 *   - textures.png (hw12/scene4): equal on every byte, incl. the bitmap-textured quad;
 *   - gi_*.png (hw15/scene2, stochastic): statistically (block means vs the 512-spp render).
 * And by the reference-measured counters recorded in SURVEY.md §6/§8 (tree topology,
 * intersect-call counts per frame, per-ray node/packet averages), tests/test_oracle_pins.py.
 *
 * Every function cites the reference file:line it follows (paths relative to
 * the reference's include/raytracer/).
 */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ORA_MAT_DIFFUSE = 0, ORA_MAT_REFLECTIVE = 1, ORA_MAT_REFRACTIVE = 2, ORA_MAT_CONSTANT = 3, ORA_MAT_TEXTURE = 4 };
enum { ORA_TEX_ALBEDO = 0, ORA_TEX_EDGES = 1, ORA_TEX_CHECKER = 2, ORA_TEX_BITMAP = 3 };   /* scene/texture/texture.hpp:13 */
enum { ORA_ACCEL_KD_SIMD = 0, ORA_ACCEL_KD_SCALAR = 1 };

typedef struct ora_scene ora_scene;
typedef struct ora_accel ora_accel;

/* Flattened scene (what io/json/loader.hpp:235-265 produces, as arrays). */
typedef struct {
    int32_t n_meshes;
    const int32_t *mesh_material;  /* [n_meshes] */
    const int32_t *mesh_nverts;    /* [n_meshes] */
    const int32_t *mesh_ntris;     /* [n_meshes] */
    const float *vertices;         /* concatenated [sum nverts][3] */
    const uint32_t *indices;       /* concatenated [sum ntris][3], mesh-local */
    int32_t n_materials;
    const int32_t *mat_kind;       /* [n_materials] ORA_MAT_* */
    const float *mat_albedo;       /* [n_materials][3] */
    const float *mat_ior;          /* [n_materials] */
    const int32_t *mat_smooth;     /* [n_materials] */
    const int32_t *mat_texture;    /* [n_materials] texture index for ORA_MAT_TEXTURE */
    const float *uvs;              /* concatenated [.][2] per-vertex uv of the meshes with mesh_has_uvs */
    const int32_t *mesh_has_uvs;   /* [n_meshes] */
    int32_t n_textures;
    const int32_t *tex_kind;       /* [n_textures] ORA_TEX_* */
    const float *tex_color_a;      /* [n_textures][3] */
    const float *tex_color_b;      /* [n_textures][3] */
    const float *tex_param;        /* [n_textures] edge_width / square_size */
    int32_t n_lights;
    const float *light_pos;        /* [n_lights][3] */
    const float *light_intensity;  /* [n_lights] */
    float cam_pos[3];
    float cam_mat[9];              /* row-major, as in the .crtscene */
    float background[3];
    int32_t width, height, bucket_size;
    /* bitmap textures (scene/texture/bitmap.hpp): the decoded RGB bytes of every ORA_TEX_BITMAP texture, rows top-down as
     * stbi_load returns them, and per texture {byte offset into tex_pixels, width, height}.  May be NULL without bitmaps. */
    const uint8_t *tex_pixels;
    const int32_t *tex_bitmap;     /* [n_textures][3] */
} ora_scene_desc;

/* Runtime form of config.hpp:6-17 (compile-time constants in the reference). */
typedef struct {
    int32_t width, height;         /* 0 = take from scene */
    int32_t spp;                   /* samples_per_pixel */
    int32_t max_depth;             /* max_ray_depth */
    int32_t diffuse_rays;          /* diffuse_reflection_ray_count */
    uint32_t seed;                 /* fixed_rng_seed */
    double fov_degrees;
    float shadow_bias, reflection_bias, refraction_bias;
    int32_t n_threads;             /* 0 = hardware concurrency */
    int32_t count_work;            /* 1 = also tally nodes / boxes / leaves / packets / triangles (slower) */
} ora_render_params;

/* 32-byte hit record, same layout as rtk_hit in include/rtk.h. */
typedef struct {
    float t, u, v;                 /* t < 0 => miss */
    uint32_t tri;                  /* global triangle index, 0xFFFFFFFF on miss */
    uint32_t mesh;
    float normal[3];               /* hit_normal */
} ora_hit;

/* counters[] slots */
enum {
    ORA_C_RAYS = 0,      /* intersect() invocations */
    ORA_C_HITS,          /* invocations that returned a hit */
    ORA_C_NODES,         /* tree nodes popped */
    ORA_C_BOXPASS,       /* nodes whose box test passed (incl. best_t prune) */
    ORA_C_LEAVES,        /* leaves entered */
    ORA_C_PACKETS,       /* W-wide packets tested (kd_simd) */
    ORA_C_TRIS,          /* unpadded triangles tested */
    ORA_C_PRIMARY,       /* camera rays */
    ORA_C_COUNT
};

ora_scene *ora_scene_create(const ora_scene_desc *d);
void ora_scene_destroy(ora_scene *s);

/* kind: ORA_ACCEL_KD_SIMD (kd_tree_simd.hpp) or ORA_ACCEL_KD_SCALAR (kd_tree.hpp).
 * W is the packet width for KD_SIMD (native_simd<float>::size() in the reference). */
ora_accel *ora_accel_build(const ora_scene *s, int kind, float eps, int max_depth, int max_leaf, int W);
void ora_accel_destroy(ora_accel *a);

/* Tree introspection (reference node order = creation order, kd_tree_simd.hpp:146-185). */
int64_t ora_accel_num_nodes(const ora_accel *a);
int64_t ora_accel_num_packets(const ora_accel *a);
int64_t ora_accel_num_leaf_refs(const ora_accel *a);     /* unpadded */
int64_t ora_accel_num_triangles(const ora_accel *a);
/* nodes_box [n][6] (min xyz, max xyz); nodes_link [n][4] = child0, child1, leaf_start (into the
 * unpadded leaf-ref array, -1 for inner), leaf_count (unpadded). */
void ora_accel_dump(const ora_accel *a, float *nodes_box, int32_t *nodes_link, int32_t *leaf_refs);
/* vertex normals of mesh m (mesh.hpp:23-44), [nverts][3] */
void ora_scene_vertex_normals(const ora_scene *s, int mesh, float *out);

/* Batched closest-hit: rays [n][6] = origin xyz, direction xyz. */
void ora_intersect(const ora_accel *a, const float *rays, size_t n, int cull, ora_hit *out,
                   uint64_t *counters /* ORA_C_COUNT, accumulated; may be NULL */);

/* The rest of hit<F> for the same rays: out [n][16] = position xyz, face_normal xyz, uvs[6], w, 0, 0, 0 (zeros on a miss). */
void ora_intersect_rest(const ora_accel *a, const float *rays, size_t n, int cull, float *out);

/* render_frame (render/render.hpp:18-108).  rgb [h][w][3] float. */
int ora_render_frame(const ora_accel *a, const ora_render_params *p, float *rgb,
                     uint64_t *counters /* ORA_C_COUNT, overwritten; may be NULL */);

/* The camera rays render_frame spawns (render/render.hpp:35-62), sample `sample` of every pixel:
 * rays [h][w][6] = origin xyz, direction xyz. */
int ora_camera_rays(const ora_accel *a, const ora_render_params *p, int sample, float *rays);

/* The colour caller-supplied rays see (render/render.hpp:64-69 for one ray each): intersect<cull>, then color_hit(.., 0), the
 * background on a miss.  rays [n][6], rgb [n][3]; the RNG root key of ray i is ora_root_key(p->seed, i, sample).  Of `p` the
 * depth, the GI rays, the seed and the biases are read.  One thread. */
int ora_radiance(const ora_accel *a, const ora_render_params *p, const float *rays, size_t n, int cull, int sample, float *rgb,
                 uint64_t *counters /* ORA_C_COUNT, overwritten; may be NULL */);

/* What the light loop multiplies the light by at every ray's first hit (render/render.hpp:205, :235): sample(texture, hit, uvs)
 * on a texture material (the sample_texture that color_hit calls), the material's albedo on any other, the background on a
 * miss.  rays [n][6], rgb [n][3]. */
void ora_first_hit_albedo(const ora_accel *a, const float *rays, size_t n, int cull, float *rgb);

/* write_ppm (io/image/ppm.hpp:7-25): returns bytes written into buf (or needed if buf==NULL). */
size_t ora_write_ppm(const float *rgb, int width, int height, char *buf, size_t cap);

/* Counter-based RNG shared by the oracle and the HIP path (replaces utils/rand.hpp:5-19): keyed by the position of a
 * ray in its sample's ray tree (see rt_oracle.c). */
uint32_t ora_root_key(uint32_t seed, uint32_t pixel, uint32_t sample);
uint32_t ora_child_key(uint32_t key, uint32_t child);
float ora_urand_key(uint32_t key, uint32_t j);
/* deterministic sin/cos used for GI directions on both sides */
void ora_sincos(float angle, float *s, float *c);

#ifdef __cplusplus
}
#endif
#endif
