/*
 * rtk.h — C-ABI of the MI355X-native kd-tree traversal / ray-triangle intersection engine.
 *
 * This is the drop-in boundary for ONE path of MihailMihov/simd-raytracer: everything a caller
 * reaches through the reference's `accelerator` concept and `render_frame` for
 * `kd_tree_simd_accel`.  Plain pointers and sizes only; no C++/torch types; never throws.
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/include/raytracer/).  The reference-side binding a maintainer would add is
 * in INTEGRATION.md; the header-only C++ adapter modelling the concept is
 * simd-raytracer_amd/hip_accel.hpp.
 *
 * There is NO CPU fallback behind this interface: compute entry points return
 * RTK_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef RTK_H
#define RTK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTK_ABI_VERSION 4

/* status codes (reference: intersect is noexcept, miss = nullopt, kd_tree_simd.hpp:188,231;
 * loader throws std::invalid_argument, io/json/loader.hpp:104,127,145,170,190,224) */
enum {
    RTK_OK = 0,
    RTK_ERR_INVALID = 1,      /* bad argument / malformed description */
    RTK_ERR_NO_DEVICE = 2,    /* no usable HIP device: the product has no CPU path */
    RTK_ERR_HIP = 3,          /* a HIP runtime call failed */
    RTK_ERR_IO = 4,           /* file could not be read / written */
    RTK_ERR_PARSE = 5,        /* .crtscene is not valid JSON or misses a required key */
    RTK_ERR_UNSUPPORTED = 6   /* feature outside the accelerated path (bitmap texture files other than baseline JPEG) */
};

/* material kinds: scene/material/material.hpp:12 */
enum { RTK_MAT_DIFFUSE = 0, RTK_MAT_REFLECTIVE = 1, RTK_MAT_REFRACTIVE = 2, RTK_MAT_CONSTANT = 3, RTK_MAT_TEXTURE = 4 };

/* texture kinds: scene/texture/texture.hpp:13.  RTK_TEX_BITMAP = bitmap_texture (scene/texture/bitmap.hpp): the texels
 * travel as the RGB bytes `stbi_load` returns (tex_pixels); rtk_scene_load_crtscene decodes baseline JPEG files itself
 * (csrc/jpeg.cpp, stb_image's arithmetic) */
enum { RTK_TEX_ALBEDO = 0, RTK_TEX_EDGES = 1, RTK_TEX_CHECKER = 2, RTK_TEX_BITMAP = 3 };

/* traversal strategy of the device kernels; all of them give bit-identical results */
enum {
    RTK_TRACE_AUTO = 0,   /* batched intersect: wave-cooperative while the wave's rays agree, per-lane otherwise; batches of
                             2^18 rays and more are probed first (every 16th wave of 64 rays; one stream synchronisation):
                             coherent as they come -> RTK_TRACE_WAVE, in no useful order -> sorted first (RTK_TRACE_REPACK);
                             frames: the GROUP4 megakernel (GROUP8 when the frame has few pixel blocks); scenes whose ray trees
                             fork (refraction, diffuse GI) are timed through RTK_TRACE_STREAM and the megakernel on their first
                             frames and keep the faster */
    RTK_TRACE_LANE = 1,   /* one ray per lane, independent stackless traversal */
    RTK_TRACE_WAVE = 2,   /* one wave walks the tree once for its 64 rays (scalar node/triangle fetch) */
    RTK_TRACE_GROUP4 = 3, /* frames only: 4 waves share 64 rays and split every large leaf 4 ways (merge through LDS) */
    RTK_TRACE_GROUP8 = 4, /* frames only: same with 8 waves */
    RTK_TRACE_GROUP16 = 5, /* frames only: same with 16 waves (one 1024-thread workgroup per 8x8 pixel block) */
    RTK_TRACE_STREAM = 6, /* frames only: the ray tree level by level — per-depth path / shadow / combine kernels over
                             compacted ray queues (stream.hip) */
    RTK_TRACE_TWOPASS = 7, /* frames only, spp == 1: rendered by the GROUP4 engine; kept so that callers compile (it named a
                             camera-ray pass followed by a cost-sorted shading pass, which GROUP4's cost feedback superseded) */
    RTK_TRACE_REPACK = 8  /* batched intersect only: the rays are first sorted by the cell of their origin and direction
                             (repack.hip: Morton key over the dimensions that vary, rocPRIM radix sort), then traced in that
                             order -- wave-cooperatively when the sort makes tight waves, with the per-lane fallback otherwise;
                             hits land in the caller's order, bit-identical to every other mode.  Needs 16 B of workspace
                             per ray (kept by the accel; a later batch on another stream waits, on the device, for the batch
                             that is still walking it).  Never blocks the host.  RTK_TRACE_AUTO does this by itself for large
                             incoherent batches -- after a probe whose verdict costs one stream synchronisation, so AUTO on
                             2^18 rays and more is not stream-capturable; RTK_REPACK=0 in the environment turns the probe and
                             the sort off */
};

typedef struct rtk_scene rtk_scene;   /* replaces scene<F>, scene/scene.hpp:14-22 */
typedef struct rtk_accel rtk_accel;   /* replaces kd_tree_simd_accel<F,eps,...>, render/accel/kd_tree_simd.hpp:63-98 */

/* Flattened scene<F>: what parse_scene_file (io/json/loader.hpp:235-265) produces. */
typedef struct {
    int32_t n_meshes;
    const int32_t *mesh_material;   /* [n_meshes]  mesh_object::material_idx */
    const int32_t *mesh_nverts;     /* [n_meshes] */
    const int32_t *mesh_ntris;      /* [n_meshes] */
    const float *vertices;          /* concatenated [sum nverts][3] */
    const uint32_t *indices;        /* concatenated [sum ntris][3], mesh-local vertex indices */
    int32_t n_materials;
    const int32_t *mat_kind;        /* [n_materials] RTK_MAT_* */
    const float *mat_albedo;        /* [n_materials][3] */
    const float *mat_ior;           /* [n_materials] */
    const int32_t *mat_smooth;      /* [n_materials] smooth_shading */
    const int32_t *mat_texture;     /* [n_materials] texture index for RTK_MAT_TEXTURE, ignored otherwise; may be NULL */
    const float *uvs;               /* concatenated per-vertex (u, v) of the meshes with mesh_has_uvs != 0, in mesh order
                                       (loader.hpp:173-192 keeps the first two of every three numbers); may be NULL */
    const int32_t *mesh_has_uvs;    /* [n_meshes] 1 = the mesh has nverts uv pairs in `uvs`, 0 = all-zero uvs; may be NULL */
    int32_t n_textures;             /* scene::textures (scene/scene.hpp:18), referenced by index instead of by name */
    const int32_t *tex_kind;        /* [n_textures] RTK_TEX_* */
    const float *tex_color_a;       /* [n_textures][3] albedo / edge_color / color_A */
    const float *tex_color_b;       /* [n_textures][3] (unused) / inner_color / color_B */
    const float *tex_param;         /* [n_textures] (unused) / edge_width / square_size */
    int32_t n_lights;
    const float *light_pos;         /* [n_lights][3] */
    const float *light_intensity;   /* [n_lights] */
    float cam_pos[3];               /* camera::position, scene/camera.hpp:10 */
    float cam_mat[9];               /* camera::matrix row-major, scene/camera.hpp:11 */
    float background[3];            /* settings::background_color */
    int32_t width, height;          /* settings::image_width/height */
    int32_t bucket_size;            /* settings::bucket_size (default 64, loader.hpp:48) */
    /* bitmap_texture::texture (scene/texture/bitmap.hpp:11-44) of every RTK_TEX_BITMAP texture: 3 bytes per texel, rows top-down,
     * as stbi_load returns them (bitmap.hpp turns a byte b into F(b) * F(1.0 / 255.0)); all textures concatenated.
     * tex_bitmap[i] = {byte offset of texture i in tex_pixels, width, height}.  Both may be NULL without bitmap textures. */
    const uint8_t *tex_pixels;
    const int32_t *tex_bitmap;      /* [n_textures][3] */
} rtk_scene_desc;

typedef struct {
    int32_t n_meshes, n_materials, n_lights;
    int32_t n_vertices, n_triangles;
    int32_t width, height, bucket_size;
    int32_t n_textures, n_uv_vertices;   /* n_uv_vertices = vertices of the meshes that carry uvs */
    int32_t n_bitmap_bytes;              /* size of the concatenated texel bytes of all bitmap textures */
} rtk_scene_info;

/* template parameters of kd_tree_simd_accel (kd_tree_simd.hpp:63-67) as runtime values */
typedef struct {
    int32_t max_depth;              /* 8  */
    int32_t max_leaf_size;          /* 64 */
    float eps;                      /* 1e-6f  (config.hpp:8) */
    int32_t normalize_hit_normal;   /* 1 = kd_tree_simd.hpp:250 behaviour, 0 = kd_tree.hpp:140 behaviour */
    int32_t device;                 /* HIP device ordinal; -1 = current device */
    int32_t traversal;              /* RTK_TRAVERSAL_* ; 0 = the reference's order (the parity mode, default) */
} rtk_accel_params;

/* Leaf visiting order of the wave-cooperative walks (kd_tree_simd.hpp:207-214 pushes child0 then child1 for every ray: child1
 * is always visited first, there is no near/far ordering; README.md:118-124 lists better traversal as the author's to-do).
 *   RTK_TRAVERSAL_REFERENCE  that order: every result bit-identical to the reference (hit-record ties included).
 *   RTK_TRAVERSAL_FAST       front to back: at every split plane the child on the side the rays come from is visited first
 *                            (chosen per wave from the majority sign of the direction on each axis), so a hit found early
 *                            prunes what lies behind it (`best_t < box.t_min`, :203-205).  The closest distance t of every
 *                            ray is unchanged; which of several triangles with EXACTLY that t wins (shared edges and vertices,
 *                            duplicated references) may differ, and with it u, v, the triangle index and the normal of such hits.
 *                            Occlusion queries give the same answers -- except that on scenes with transmissive materials the
 *                            streaming pipeline answers one with a SINGLE any-hit query against the triangles that are not
 *                            transmissive, on the straight segment to the light, instead of is_occluded's loop of closest hits
 *                            that steps through every transmissive surface (render.hpp:110-131; the README's "any-hit shadow
 *                            rays").  The answers differ where an occluder lies within shadow_bias behind a transmissive surface
 *                            (the loop steps over it), beyond the light by less than the biases the loop has accumulated (the loop
 *                            does not take them off max_t), or where a ray grazes an occluder's edge within rounding; measured on
 *                            hw11/scene8 at 1920x1080: 0 pixels.  RTK_FAST_OCCLUDERS=0 keeps the loop.
 *                            Not the parity mode: off unless asked for here, or by RTK_TRAVERSAL_FAST=1 in the environment when
 *                            the accel is built. */
enum { RTK_TRAVERSAL_REFERENCE = 0, RTK_TRAVERSAL_FAST = 1 };

typedef struct {
    int32_t n_nodes, n_inner, n_leaves;
    int32_t n_leaf_refs;            /* unpadded triangle references over all leaves */
    int32_t max_leaf_refs;
    int32_t n_triangles;
    int32_t tree_depth;
    int32_t reserved;
} rtk_tree_info;

/* ray3<F> without the derived inv_direction (core/math/ray3.hpp:5-15); 24 bytes */
typedef struct { float origin[3]; float direction[3]; } rtk_ray;

/* compact hit<F> (render/hit.hpp:9-21); 32 bytes.  Miss: t = -1, tri = mesh = 0xFFFFFFFF.
 * position = origin + t*direction, w = 1-u-v, face_normal/uvs = triangles[tri] — all derivable by the caller. */
typedef struct {
    float t, u, v;
    uint32_t tri;                   /* global triangle index (position in the concatenated mesh order, kd_tree_simd.hpp:103-111) */
    uint32_t mesh;                  /* hit<F>::mesh_idx */
    float normal[3];                /* hit<F>::hit_normal */
} rtk_hit;

/* config.hpp:6-17 as runtime parameters + multi-GPU tile sharding */
typedef struct {
    int32_t width, height;          /* 0 = take from the scene */
    int32_t spp;                    /* samples_per_pixel */
    int32_t max_ray_depth;          /* max_ray_depth */
    int32_t diffuse_rays;           /* diffuse_reflection_ray_count */
    uint32_t seed;                  /* fixed_rng_seed */
    double fov_degrees;             /* fov_degrees */
    float shadow_bias, reflection_bias, refraction_bias;
    int32_t trace_mode;             /* RTK_TRACE_* */
    int32_t rank, world_size;       /* world_size <= 1: whole frame.  Else this rank's share of the scene's buckets
                                     * (render/tile/bucket.hpp:7-21, row-major): bucket i belongs to rank i % world_size -- or,
                                     * when a row of buckets is a whole number of rounds (tiles_x % world_size == 0, which would give
                                     * every rank the same columns), bucket (bx, by) to rank (bx + by) % world_size */
    int32_t collect_stats;          /* 1 = also count nodes/leaves/triangles per ray, as the reference algorithm visits them
                                     * (slower kernel variant); 2 = count what the production path visits (its occlusion
                                     * queries stop at the first answering hit when no material is transmissive, and those
                                     * whose light contribution is +-0 in every channel are counted in `rays` but not traced:
                                     * RTK_SKIP_UNLIT_SHADOW; same frame, same `rays`) */
    /* Progressive accumulation (the spp loop of render/render.hpp:34-72 cut into passes): render samples
     * [sample_begin, sample_begin + sample_count) of every pixel.  sample_count == 0: all `spp` samples in one call.
     * A pass with sample_begin > 0 continues the running per-pixel sum the previous pass left in the output buffer (the
     * sum stays in sample order, so N passes give the bits of one call); the pass that ends at `spp` divides by spp
     * (render.hpp:72) and leaves the finished frame.  Until then the buffer holds sums, not colours. */
    int32_t sample_begin, sample_count;
} rtk_render_params;

typedef struct {
    uint64_t rays;                  /* the reference's intersect() invocations (primary + shadow segments + reflection + refraction
                                     * + GI), whether or not the production path had to traverse the tree to answer them */
    uint64_t primary;               /* camera rays */
    uint64_t hits;                  /* valid only with collect_stats */
    uint64_t nodes;                 /* tree nodes popped, per ray, summed           (collect_stats) */
    uint64_t boxpass;               /* nodes whose slab test passed                 (collect_stats) */
    uint64_t leaves;                /* leaves entered                               (collect_stats) */
    uint64_t tris;                  /* unpadded triangles tested                    (collect_stats) */
    uint64_t packets16;             /* = sum ceil(leaf_count/16): W=16 packets the reference would test (collect_stats) */
} rtk_counters;

/* ---- library ---- */
int rtk_abi_version(void);
const char *rtk_last_error(void);               /* thread-local message for the last non-OK status */
int rtk_device_count(int *count);               /* number of usable HIP devices (0 is not an error) */

/* ---- scene: replaces parse_scene_file + scene<F> ---- */
int rtk_scene_create(const rtk_scene_desc *desc, rtk_scene **out);      /* copies everything it needs */
int rtk_scene_load_crtscene(const char *path, rtk_scene **out);         /* io/json/loader.hpp:235-265 */
int rtk_scene_get_info(const rtk_scene *scene, rtk_scene_info *info);
/* copies the flattened arrays back out (sizes from rtk_scene_get_info); any pointer may be NULL */
int rtk_scene_get_arrays(const rtk_scene *scene, int32_t *mesh_material, int32_t *mesh_nverts, int32_t *mesh_ntris,
                         float *vertices, uint32_t *indices, int32_t *mat_kind, float *mat_albedo, float *mat_ior,
                         int32_t *mat_smooth, float *light_pos, float *light_intensity, float *cam_pos,
                         float *cam_mat, float *background);
/* texture side of the scene: [n_materials], [n_meshes], [n_uv_vertices][2], [n_textures], [n_textures][3] x2, [n_textures] */
int rtk_scene_get_textures(const rtk_scene *scene, int32_t *mat_texture, int32_t *mesh_has_uvs, float *uvs,
                           int32_t *tex_kind, float *tex_color_a, float *tex_color_b, float *tex_param);
/* bitmap textures: tex_bitmap [n_textures][3] = {byte offset, width, height}, tex_pixels [n_bitmap_bytes]; either may be NULL */
int rtk_scene_get_bitmaps(const rtk_scene *scene, int32_t *tex_bitmap, uint8_t *tex_pixels);
/* The decoder behind bitmap textures: what `stbi_load(path, &w, &h, &channels, 0)` (scene/texture/bitmap.hpp:15) returns for a
 * baseline JPEG held in memory.  *channels = 1 or 3; writes at most cap bytes (pixels may be NULL to query the size). */
int rtk_decode_jpeg(const uint8_t *data, size_t size, int32_t *width, int32_t *height, int32_t *channels,
                    uint8_t *pixels, size_t cap);
/* mesh_object::vertex_normals (scene/object/mesh.hpp:25-43), [nverts of that mesh][3] */
int rtk_scene_vertex_normals(const rtk_scene *scene, int32_t mesh, float *out);
void rtk_scene_destroy(rtk_scene *scene);

/* ---- accel: replaces kd_tree_simd_accel ctor + build_tree (kd_tree_simd.hpp:100-185) ---- */
int rtk_accel_build(const rtk_scene *scene, const rtk_accel_params *params, rtk_accel **out);
int rtk_accel_tree_info(const rtk_accel *accel, rtk_tree_info *info);
/* Tree in the REFERENCE's node order (creation order).  nodes_box [n][6] = min xyz, max xyz;
 * nodes_link [n][4] = child0, child1, leaf_start (index into leaf_refs, -1 for inner), leaf_count;
 * leaf_refs [n_leaf_refs] global triangle indices in leaf order (the unpadded packet contents). */
int rtk_accel_tree_dump(const rtk_accel *accel, float *nodes_box, int32_t *nodes_link, int32_t *leaf_refs);
void rtk_accel_destroy(rtk_accel *accel);

/* ---- batched closest hit: replaces accel.template intersect<cull>(ray) (render/accel/accel.hpp:8-12,
 *      kd_tree_simd.hpp:187-264); one ray per lane ---- */
int rtk_accel_intersect(rtk_accel *accel, const rtk_ray *rays, size_t n, int cull, int trace_mode,
                        rtk_hit *out);                                   /* host buffers, synchronous */
int rtk_accel_intersect_device(rtk_accel *accel, const rtk_ray *d_rays, size_t n, int cull, int trace_mode,
                               rtk_hit *d_out, void *hip_stream);        /* device buffers, stream-ordered */
/* same launch with per-ray work counters accumulated into *counters (device side, synchronous) */
int rtk_accel_intersect_stats(rtk_accel *accel, const rtk_ray *d_rays, size_t n, int cull, int trace_mode,
                              rtk_hit *d_out, rtk_counters *counters);

/* ---- batched occlusion: replaces is_occluded(accel, ray, max_t) (render/render.hpp:110-131) ---- */
/* Per query i, the reference's loop in float, in its operation order:
 *     while (0.0f < max_t) {                      // false for NaN, <= 0, -0: RTK_OCC_CLEAR, nothing traced
 *         h = intersect<cull = false>(ray)        // closest hit, as rtk_accel_intersect(cull = 0)
 *         if (miss || max_t < h.t) -> RTK_OCC_CLEAR                                          (:117)
 *         if (material of h.mesh is not RTK_MAT_REFRACTIVE) -> RTK_OCC_OCCLUDED              (material/queries.hpp:28-30)
 *         ray.origin = (ray.origin + h.t * ray.direction) + shadow_bias * ray.direction      (:126-127)
 *         max_t -= h.t
 *     }
 *     -> RTK_OCC_CLEAR
 * max_t is in units of the ray parameter t (the reference's callers pass unit directions and the distance to the light;
 * nothing here needs unit directions); max_t = +inf is a plain any-hit query.
 * The reference's loop has no bound; a kernel needs one.  A query that has made RTK_OCCLUDED_MAX_STEPS closest-hit queries
 * and would make another is answered RTK_OCC_STEP_LIMIT: "the reference would still be stepping" -- the only departure, and
 * visible in the answer.  (With the reference's bias of 1e-4 the longest loop on the fixture scenes is 15; a negative bias
 * re-hits the surface it just left and runs into the limit.)
 * trace_mode: RTK_TRACE_AUTO, RTK_TRACE_LANE or RTK_TRACE_WAVE, identical bytes from all three; the frame-only modes and
 * RTK_TRACE_REPACK are RTK_ERR_INVALID.  shadow_bias must be finite.  n == 0 is RTK_OK and touches nothing.  out / d_out
 * holds one byte per query (no alignment demand; d_max_t: 4 bytes).
 * An accel built with RTK_TRAVERSAL_FAST runs the same loop over its own front-to-back tree -- NOT the opaque-only shortcut
 * tree of the streaming pipeline.  The closest t is the same in both orders, so on scenes without transmissive materials the
 * answers are those of the parity mode; with them, a transmissive and an opaque triangle at EXACTLY the same t may resolve
 * either way (the tie caveat of RTK_TRAVERSAL_FAST above), and with it that query's answer.
 * n_intersections (host variant, may be NULL): the closest-hit queries the batch made, summed over its queries -- what the
 * reference's intersect() call counter would have gone up by. */
#define RTK_OCCLUDED_MAX_STEPS 1024
enum { RTK_OCC_CLEAR = 0, RTK_OCC_OCCLUDED = 1, RTK_OCC_STEP_LIMIT = 2 };

int rtk_accel_occluded(rtk_accel *accel, const rtk_ray *rays, const float *max_t, size_t n,
                       float shadow_bias, int trace_mode, uint8_t *out,
                       uint64_t *n_intersections /* may be NULL */);     /* host buffers, synchronous */
/* launch only: no host synchronisation and no allocation (stream-capturable once the accel is on the device, i.e. after
 * any compute call on it) */
int rtk_accel_occluded_device(rtk_accel *accel, const rtk_ray *d_rays, const float *d_max_t, size_t n,
                              float shadow_bias, int trace_mode, uint8_t *d_out,
                              void *hip_stream);                          /* device buffers, stream-ordered */

/* ---- batched radiance: replaces `intersect<cull>(ray)` followed by color_hit(accel, hit, 0) (render/render.hpp:64-69, 133-308) ---- */
typedef struct {
    int32_t max_ray_depth;          /* config.hpp max_ray_depth; 0..16 as for frames */
    int32_t diffuse_rays;           /* diffuse_reflection_ray_count */
    uint32_t seed;                  /* fixed_rng_seed */
    int32_t sample;                 /* which sample of `seed`'s sequence these rays are (see ids) */
    float shadow_bias, reflection_bias, refraction_bias;
    int32_t cull;                   /* the <cull> of the batch's own rays: 1 = as render_frame's camera rays (:64), 0 = as a secondary ray */
    int32_t trace_mode;             /* RTK_TRACE_AUTO or RTK_TRACE_STREAM; everything else RTK_ERR_INVALID */
} rtk_radiance_params;
/* Per ray i, in float, in the reference's operation order:
 *     h = intersect<cull>(rays[i])
 *     c = h ? color_hit(accel, *h, 0) : background_color
 *     rgb[i] = color{} += c                       // what render_frame leaves in a pixel at samples_per_pixel == 1
 *                                                 // (render.hpp:33,66-72: a channel that is -0 comes out +0, "/ 1" changes nothing)
 * One colour per ray, written in the caller's order; nothing accumulates across calls.  Rays need not share an origin and
 * need not be normalised (the reference's own secondary rays are not always).  The scene's camera plays no part.
 * Random numbers (diffuse GI only): a draw is keyed by a ray's position in its sample's ray tree, root key =
 * f(seed, pixel index, sample).  Ray i gets the root key of pixel index `ids ? ids[i] : (uint32_t)i` at sample `p->sample`.  So the
 * rays of rtk_camera_rays(.., sample s) with ids == NULL, cull = 1, sample = s give exactly sample s of rtk_render_frame with the
 * same parameters, diffuse GI included; a caller's sum over s in order, divided by float(spp) (render.hpp:66-72), gives the
 * frame.  Without diffuse rays ids, seed and sample cannot change a result.
 * counters (host variant, may be NULL) as for a frame: rays = the reference's intersect() invocations the batch stands for,
 * its own n level-0 rays included; primary = n; the collect_stats fields are 0.  The counters of the most recent frame
 * (rtk_render_last_counters) are left alone.
 * Occlusion queries inside the recursion are answered as in frames, with the same switches (they stop at the first
 * answering hit when no material is transmissive; RTK_SKIP_UNLIT_SHADOW): same colours, same `rays`.  On an accel built with
 * RTK_TRAVERSAL_FAST the call has the caveats frames have there (ties at exactly equal t, occlusion through transmissive
 * surfaces answered from the opaque triangles); parity with the reference is claimed for RTK_TRAVERSAL_REFERENCE only.
 * The batch runs through the streaming pipeline (RTK_TRACE_STREAM's; RTK_TRACE_AUTO means the same here) in chunks.  A chunk
 * whose ray tree outgrows its queues is redone on the device by a per-ray kernel: slower, the same bits.
 * Errors: a NULL accel or p, another trace_mode, max_ray_depth outside [0, 16], diffuse_rays < 0, sample < 0, a non-finite bias,
 * n > 0 with NULL rays / rgb, ids == NULL with n > 2^32 -> RTK_ERR_INVALID, and the accel stays usable.  Then n == 0 -> RTK_OK,
 * nothing touched, device or not.  Then no device -> RTK_ERR_NO_DEVICE.
 * The host variant is synchronous.  The device variant is stream-ordered and never synchronises the host; it allocates
 * (and then synchronises the device once) when a batch needs more queue space than any call before it on this accel -- more
 * rays, or more lights than before (the queues hold one contribution per light: rtk_accel_set_lights).  It is
 * NOT stream-capturable: the pipeline forks onto streams of its own.
 * The queues belong to the accel and are shared with RTK_TRACE_STREAM frames.  A radiance batch (or such a frame) issued on
 * another stream than the previous user of the queues waits for that user ON THE DEVICE (an event) before it touches them:
 * calls on different streams are safe and take turns.  d_rays: 4-byte aligned, 24 bytes per ray; d_rgb: 4-byte aligned. */
int rtk_accel_radiance(rtk_accel *accel, const rtk_ray *rays, const uint32_t *ids /* may be NULL */, size_t n,
                       const rtk_radiance_params *p, float *rgb /* host [n][3] */, rtk_counters *counters /* may be NULL */);
int rtk_accel_radiance_device(rtk_accel *accel, const rtk_ray *d_rays, const uint32_t *d_ids /* may be NULL */, size_t n,
                              const rtk_radiance_params *p, float *d_rgb /* device [n][3] */, void *hip_stream);

/* ---- dynamic geometry: the accel after scene<F>'s vertex positions changed (what re-running the kd_tree_simd_accel ctor,
 *      kd_tree_simd.hpp:100-185, on the moved scene would hold) ----
 * `vertices` has the layout of rtk_scene_desc.vertices: all meshes concatenated, rtk_scene_info.n_vertices rows.  Topology, uvs,
 * materials, textures, lights, camera and rtk_accel_params stay as they were at rtk_accel_build.
 * After RTK_OK everything observable through the accel is, bit for bit, what rtk_accel_build gives for a scene that differs from
 * the accel's only in `vertices` (same params, same environment knobs): rtk_accel_tree_info / _tree_dump, every rtk_accel_intersect*,
 * rtk_accel_occluded* and rtk_accel_radiance* result, every frame through every RTK_TRACE_* engine and its counters' `rays`.
 * RTK_TRAVERSAL_FAST accels included (their leaf orders and, with transmissive materials, the opaque-only occlusion tree are rebuilt).
 * The tree is REBUILT, not refitted, and on the device: triangles, smooth vertex normals, boxes, the level-by-level split and the
 * leaves' packets (csrc/build.hip); the host numbers the few hundred nodes.  The handle, its streams and its grown workspaces
 * survive; the cost-feedback launch order and RTK_TRACE_AUTO's engine trial start over, as on a new accel.
 * Ordering: the call SYNCHRONISES THE DEVICE AT ENTRY (nothing issued earlier, on any stream, can still be reading what it
 * replaces), then works on `hip_stream` (the host variant: the null stream).  It blocks the host once more, to read back the node
 * table and the flags; a further time only when a buffer has to grow (the first call on an accel, a tree larger than any before).  A build
 * that outgrows its node or reference capacity is noticed on the device and repeated with more room; the flag tells what the level
 * that did not fit needed, so a much deeper tree than any before can take several such repeats (at most 16), each a rebuild and a
 * host block.  Capacities are kept, so the calls after it pay nothing.
 * Work issued on the accel afterwards, on any stream, sees the new geometry: it waits on the device for an event recorded
 * behind the update's last kernel.  NOT stream-capturable.
 * Errors, in this order: NULL accel or pointer -> RTK_ERR_INVALID; no usable device -> RTK_ERR_NO_DEVICE (there is no CPU path; an
 * accel that has not been on the device yet goes there first); a non-finite coordinate -> RTK_ERR_INVALID (the host variant looks
 * before it touches the device, the device variant learns it from a flag its first kernel raises).  After any error the accel is
 * exactly as before the call and stays usable: the new geometry is built into buffers of its own and swapped in at the end. */
int rtk_accel_update_vertices(rtk_accel *accel, const float *vertices /* host [n_vertices][3] */);
int rtk_accel_update_vertices_device(rtk_accel *accel, const float *d_vertices /* device [n_vertices][3] */, void *hip_stream);

/* ---- dynamic geometry, new triangle lists: the accel after scene<F>'s meshes got other triangles as well (an isosurface
 *      extracted again, another level of detail, a tear) ----
 * `vertices` as above.  `indices` has the layout of rtk_scene_desc.indices: the meshes' triangle lists one behind the other,
 * three indices per triangle, each LOCAL to its mesh's vertices; `mesh_ntris` says how many triangles each mesh has now and
 * is read on the host in both variants.  `indices` may be NULL when every count is 0.
 * After RTK_OK everything observable through the accel is, bit for bit, what rtk_accel_build gives for a scene that differs from
 * the accel's only in `vertices`, `indices` and `mesh_ntris` (same params, same environment knobs): rtk_accel_tree_info (with
 * n_triangles) / _tree_dump, every rtk_accel_intersect*, rtk_accel_occluded* and rtk_accel_radiance* result, every frame through
 * every RTK_TRACE_* engine and its counters' `rays`.  RTK_TRAVERSAL_FAST accels included, with their leaf orders and the
 * opaque-only occlusion tree.  rtk_hit.tri is the global index in the new concatenated order.  A later
 * rtk_accel_update_vertices moves the vertices of the new topology.
 * Fixed by the call: the number of meshes, every mesh's vertex count, every mesh's material, materials, textures, lights, camera and
 * rtk_accel_params (the per-triangle uvs are gathered from the per-vertex uvs as they are NOW: rtk_accel_set_uvs, "textures and
 * uvs of a live accel" below).  Every mesh's triangle count is free: 0, smaller, or larger than anything
 * before.  Vertices no triangle uses are legal and cost a few bytes each: a caller whose vertex count varies builds the scene
 * with a POOL of vertices per mesh, as large as it will ever need, and indexes into what it uses of it.
 * The topology tables -- vertex ids, the vertex -> (triangle, corner) lists the smooth normals are summed in, mesh / material and
 * uvs per triangle, which triangles are opaque -- are made on the device from `indices` (csrc/topology.hip); from there the
 * call is rtk_accel_update_vertices: one code path, the same tree build, the same host numbering.
 * Ordering and memory are those of rtk_accel_update_vertices: the device is synchronised at entry, the work goes to `hip_stream`
 * (the host variant: the null stream), the host blocks once for the node table and the flags, later work on any stream waits
 * for the update's event; NOT stream-capturable.  Buffers grow with head room when a count outgrows them and never shrink.  The
 * node / reference retry is the same.  The cost-feedback launch order and RTK_TRACE_AUTO's engine trial start over.
 * Errors, in this order: a NULL accel, vertices or mesh_ntris, or NULL indices with a positive count -> RTK_ERR_INVALID; no usable
 * device -> RTK_ERR_NO_DEVICE; then RTK_ERR_INVALID for a negative count, triangles on a mesh without vertices, more than
 * 0xFFFFFFF0 / 3 triangles, a non-finite coordinate, an index that is not below its OWN mesh's vertex count.  The host variant
 * finds the last two before it touches the device; the device variant learns them from flags in the header it reads back anyway.
 * A bad index never becomes a bad address: the kernel that validates puts an index that is in range in its place before anything
 * dereferences it, and nothing else reads the vertex array through the caller's indices.  After any error the accel is exactly
 * as before the call and stays usable: topology and geometry are built into buffers of their own and swapped in at the end. */
int rtk_accel_update_geometry(rtk_accel *accel, const float *vertices /* host [n_vertices][3] */,
                              const uint32_t *indices /* host, concatenated [sum mesh_ntris][3], mesh-local */,
                              const int32_t *mesh_ntris /* host [n_meshes] */);
int rtk_accel_update_geometry_device(rtk_accel *accel, const float *d_vertices, const uint32_t *d_indices,
                                     const int32_t *mesh_ntris /* HOST [n_meshes] */, void *hip_stream);

/* ---- frame: replaces render_frame<A,F> (render/render.hpp:18-108) with color_hit/is_occluded device-side ---- */
/* number of floats the (rank-local) output of rtk_render_frame_device holds */
int rtk_render_output_floats(const rtk_accel *accel, const rtk_render_params *p, size_t *n_floats);
/* host variant: a pass with sample_begin > 0 uploads `rgb` (the running sums of the passes before it) first */
int rtk_render_frame(rtk_accel *accel, const rtk_render_params *p, float *rgb /* host [h][w][3] */,
                     rtk_counters *counters /* may be NULL */);
/* world_size <= 1: d_out is the frame [h][w][3].  world_size > 1: d_out is this rank's compact bucket
 * buffer [buckets_per_rank][bucket][bucket][3] (equal length on every rank, ready for an all-gather). */
/* Frames of one accel are meant for one stream at a time.  A frame on another stream than the accel's previous frame zeroes its
 * counters itself; a frame on the same stream may find them zeroed by the frame before it.  Streams are told apart by their
 * handle: before a stream on which an accel has rendered is destroyed, synchronise it, so that a stream created later at the same
 * address starts behind that accel's last frame. */
int rtk_render_frame_device(rtk_accel *accel, const rtk_render_params *p, float *d_out, void *hip_stream);
/* counters of the most recent rtk_render_frame_device on this accel; synchronises the stream it ran on */
int rtk_render_last_counters(rtk_accel *accel, rtk_counters *counters);
/* The longest 8x8 pixel block of the most recent megakernel frame on this accel, in milliseconds (device real-time clock):
 * the frame's critical path -- no number of compute units or GPUs makes the frame shorter than this.  0 for frames that
 * went through the streaming pipeline or whose blocks all took less than 10 microseconds.  Synchronises the stream the frame ran on. */
int rtk_render_last_critical_path(rtk_accel *accel, double *ms);
/* Diagnostic, not part of the rendering contract: how many times frames, views and regions calls of this accel have zeroed its
 * counters with a fill of their own since it was built.  A steady megakernel frame issues none.  Needs no device. */
int rtk_debug_counter_fills(rtk_accel *accel, uint64_t *fills);
/* Diagnostics, not part of the rendering contract, of the launch order of this accel's FRAMES (rtk_render_frame*; not views or
 * regions calls).  The order is re-sorted from the blocks' measured costs every few frames; a new order (the challenger) is judged
 * behind its first frame against the one before it (the champion) by the device time of one frame under each, and the slower
 * one is dropped.  No pixel depends on any of this.  Both calls synchronise the stream of the most recent frame.
 * rtk_debug_order_judge: of one table -- the frames' (RTK_ORDER_TABLE_FRAMES, index 0), or that of launch `index` of a views call or
 * of a regions call (a call is one launch unless it is cut) -- the sorts and judges enqueued since the accel was built, the verdicts given on the device (`taken`: the
 * challenger became the champion; `rejected`: the champion's lists were copied back), and the two stored scores in ticks of the
 * device's 100 MHz clock (0: none).  An accel that has rendered no megakernel frame reports zeros.
 * RTK_COST_JUDGE_FORCE (read when the accel is built): 1 every challenger is taken, 2 none is. */
typedef struct rtk_order_judge_stats {
    uint64_t sorts, judges;
    uint64_t taken, rejected;
    uint32_t champion_ticks, challenger_ticks;
    uint32_t units;                     /* units (8x8 pixel blocks) of the lists of the most recent frame */
    int32_t read_set;                   /* which of the two sets of lists the next frame reads: 0 or 1 */
} rtk_order_judge_stats;
enum { RTK_ORDER_TABLE_FRAMES = 0, RTK_ORDER_TABLE_VIEWS = 1, RTK_ORDER_TABLE_REGIONS = 2 };
int rtk_debug_order_judge(rtk_accel *accel, int32_t table, int32_t index, rtk_order_judge_stats *stats);
/* One set of lists as the device holds it: order [units], header [4] = {workgroups, units, -, -}, workgroup list [units] (its first
 * header[0] words are in use: a unit, or 0x80000000 | index into order of the first of four packed units).  `set`: 0 or 1.
 * *n_words = 2 * units + 4; `words` is filled when it is non-null and `capacity` (in words) suffices, else RTK_ERR_INVALID. */
int rtk_debug_order_lists(rtk_accel *accel, int32_t set, uint32_t *words, size_t capacity, size_t *n_words);
/* after the all-gather: d_gathered = [world][buckets_per_rank][bucket][bucket][3] -> d_rgb [h][w][3] */
int rtk_tiles_assemble_device(const rtk_accel *accel, const rtk_render_params *p, const float *d_gathered,
                              float *d_rgb, void *hip_stream);

/* The camera rays render_frame spawns (render/render.hpp:35-62), sample `sample` of every pixel, [h][w] in row-major order:
 * what `ray3<F> ray(camera.position, direction)` at :62 holds.  (Also the generator of the fixed synthetic workload.) */
int rtk_camera_rays(rtk_accel *accel, const rtk_render_params *p, int32_t sample, rtk_ray *rays /* host [h*w] */);
int rtk_camera_rays_device(rtk_accel *accel, const rtk_render_params *p, int32_t sample, rtk_ray *d_rays, void *hip_stream);

/* ---- the camera of a live accel, and many cameras in one call ----
 * camera<F> (scene/camera.hpp:9-11): position and matrix, row-major -- the layout of rtk_scene_desc.cam_pos / cam_mat; 48 bytes.
 * The reference keeps the camera a plain mutable member and reads it when a frame starts (render/render.hpp:25); so does the
 * accel: it is 12 floats of every launch's arguments.  The camera moves of camera.hpp:13-70 are not mirrored: callers compute poses. */
typedef struct { float position[3]; float matrix[9]; } rtk_view;

int rtk_accel_get_camera(const rtk_accel *accel, rtk_view *out);
/* After RTK_OK everything that reads the camera -- rtk_render_frame* in every RTK_TRACE_* engine, sharded frames,
 * rtk_camera_rays*, the counters -- is, bit for bit, what a fresh rtk_accel_build gives for a scene that differs only in cam_pos /
 * cam_mat.  The tree, the batched intersect / occluded / radiance results and rtk_accel_tree_dump do not depend on it.
 * The values are taken as they are (as rtk_scene_create takes the scene's).  The call touches no device memory, synchronises
 * nothing, needs no GPU and works on an accel that has never been on one; frames already enqueued keep the camera they were
 * launched with.  The camera survives rtk_accel_update_vertices / _geometry.
 * Neither the cost-feedback launch order nor RTK_TRACE_AUTO's engine verdict changes a result.  The launch order of megakernel
 * frames STARTS OVER (first-frame prior, then the new camera's costs), as after an update of the geometry, and does so even
 * when the new camera equals the old one.  Measured at 1920x1080 after a 5 degree step: on the first frame neither
 * choice wins every run (medians 0.33 ms kept, 0.35 ms reset); the third frame takes 0.20 ms after a reset and 0.30 ms under the
 * old camera's order, which a kept order serves until its next re-sort.  RTK_CAMERA_KEEPS_ORDER=1 keeps it.
 * The engine verdict is KEPT: started over at every move, the trial of a camera in motion would never end.
 * NULL accel or view -> RTK_ERR_INVALID; never RTK_ERR_NO_DEVICE. */
int rtk_accel_set_camera(rtk_accel *accel, const rtk_view *view);

/* n_views frames of the same rtk_render_params, one per camera: out is [n_views][h][w][3].  View v is, bit for bit and with the
 * same `rays`, what rtk_accel_set_camera(views[v]) + rtk_render_frame[_device] with *p gives; the accel's own camera is not
 * changed.  Random numbers are keyed by the pixel index INSIDE the view, sample and seed, as for a frame: equal cameras give
 * equal views.  sample_begin / sample_count work as for a frame, the running sums of all views live in the output buffer (the
 * host variant uploads them for a pass with sample_begin > 0).  Counters are summed over the views (primary = n_views * w * h *
 * samples); rtk_render_last_counters gives the call's totals, rtk_render_last_critical_path its longest block.
 * What runs: under RTK_TRACE_GROUP4 / 8 / 16, and RTK_TRACE_AUTO on scenes whose ray trees do not fork, with collect_stats == 0,
 * the pixel blocks of ALL views are the units of one megakernel launch, ordered by cost and packed together (RTK_TRACE_AUTO
 * chooses its workgroup size by the total).  A call of more than 131,072 blocks is cut into launches of whole views.  Every
 * other case (LANE / WAVE / STREAM / TWOPASS, forking scenes under AUTO, collect_stats != 0) renders view after view through
 * the existing engines with the view's camera in the launch arguments: same bits, same counts.
 * Errors, in this order: what rtk_render_frame refuses for *p; n_views < 0, world_size > 1 (views are not sharded: a multi-GPU
 * caller deals whole views to ranks), NULL views / output with n_views > 0 -> RTK_ERR_INVALID; then n_views == 0 -> RTK_OK with
 * nothing touched, device or not; then RTK_ERR_NO_DEVICE.
 * The device variant (d_views in DEVICE memory, 4-byte aligned) is stream-ordered.  On the one-launch path it never blocks the
 * host, except that it may allocate, and then synchronise once, when a call needs larger order / cost tables than any call
 * before it.  On the view-after-view path it copies the views back to the host first (their cameras go into launch
 * arguments), which waits for `hip_stream` once.  NOT stream-capturable. */
int rtk_render_views(rtk_accel *accel, const rtk_render_params *p, const rtk_view *views /* host */, int32_t n_views,
                     float *rgb /* host */, rtk_counters *counters /* may be NULL: totals over the views */);
int rtk_render_views_device(rtk_accel *accel, const rtk_render_params *p, const rtk_view *d_views /* DEVICE, 4-byte aligned */,
                            int32_t n_views, float *d_out /* device */, void *hip_stream);

/* ---- rectangles of a frame in one call ----
 * render_tile {x0, y0, x1, y1} (render/tile/tile.hpp), the unit of work tile_worker consumes (render/render.hpp:30-77): pixels
 * [x0, x1) x [y0, y1) of the frame *p describes.  The reference's single / region / bucket schedulers differ only in which
 * rectangles they hand out; here the caller hands them out.
 * Contract: every pixel inside a rectangle ends up, bit for bit, as rtk_render_frame with *p leaves it: the accel's camera, the
 * frame's RNG keys (pixel index py * width + px, sample, seed), the same sample_begin / sample_count semantics (a pass with
 * sample_begin > 0 continues the running sums in the output; the pass that ends at spp divides).  On an RTK_TRAVERSAL_FAST accel
 * "the same" means equal to that accel's own frame (that order is chosen per wave of 64 pixels: a rectangle made of whole 8x8
 * blocks of the frame's grid runs the frame's own waves; for any other rectangle the winner of an EXACT tie of t may differ from
 * the frame's as it may between two engines, the tie caveat of RTK_TRAVERSAL_FAST).  counters.primary = sum of the areas x samples of the pass; counters.rays =
 * the reference's intersect() invocations for exactly those pixels, so the `rays` of rectangles that tile the frame add up to
 * the frame's.  rtk_render_last_counters / rtk_render_last_critical_path report the call.  The accel's camera, the cost tables
 * of plain frames and RTK_TRACE_AUTO's engine verdict are left alone.
 * Layouts:
 *   RTK_REGIONS_IN_FRAME  the output is the whole frame [h][w][3].  Only pixels inside a rectangle are read (sample_begin > 0) or
 *                         written; every other float keeps its bits.  The rectangles must be pairwise disjoint.
 *   RTK_REGIONS_PACKED    rectangle r is a dense [y1-y0][x1-x0][3] array at float offset 3 * (sum of the areas of the rectangles
 *                         before it).  Overlaps are legal: each rectangle gets its own copy.  The running sums of a progressive
 *                         render live in this packed buffer.
 * `rects` is in HOST memory in both variants (the host sizes the launch from it), at most 65,536 of them; empty rectangles
 * (x0 == x1 or y0 == y1) are legal and cost nothing.
 * What runs: under RTK_TRACE_GROUP4 / 8 / 16, and RTK_TRACE_AUTO on scenes whose ray trees do not fork, the 8x8 pixel blocks of ALL
 * rectangles -- anchored at each rectangle's own corner -- are the units of ONE megakernel launch with one cost order and one
 * packed list of cheap blocks.  A call of more than 131,072 units (RTK_VIEWS_LAUNCH_UNITS) is cut into launches of whole
 * rectangles.  The measured launch order is reused only by a call whose rectangle list, layout and parameters equal the previous
 * call's; any other list starts in the natural order.  RTK_TRACE_STREAM, and RTK_TRACE_AUTO on forking scenes (refraction,
 * diffuse GI), run sample by sample: the rectangles' camera rays and frame pixel indices, the streaming pipeline of
 * rtk_accel_radiance over them, and a kernel that adds the colours into the output in sample order (bit-equal: radiance
 * returns +0 + c, and a running sum that starts at +0 never holds -0).  Its workspace belongs to the accel, grows with head
 * room and is walked in chunks of 2^20 pixels.
 * Errors, in this order, all RTK_ERR_INVALID: a NULL accel or p, then what rtk_render_frame refuses for *p; RTK_TRACE_LANE /
 * _WAVE / _TWOPASS, collect_stats != 0, world_size > 1 (the caller deals rectangles to ranks), n_rects < 0 or > 65,536, another
 * layout; NULL rects or output with n_rects > 0; a rectangle with x0 < 0, y0 < 0, x1 < x0, y1 < y0, x1 > width or y1 > height;
 * overlapping rectangles under RTK_REGIONS_IN_FRAME.  Then n_rects == 0 or zero total area -> RTK_OK with nothing touched, device
 * or not.  Then RTK_ERR_NO_DEVICE.  A refused call leaves the accel usable and unchanged.
 * The host variant moves what the layout needs: the packed buffer, or the whole frame up and down (so the caller's pixels outside
 * the rectangles come back as they went).  The device variant is stream-ordered; it copies the small rectangle table from a
 * buffer of its own (it waits for the previous call's table to be consumed first) and may allocate, and then synchronise once,
 * when a call needs larger tables than any before.  NOT stream-capturable. */
typedef struct { int32_t x0, y0, x1, y1; } rtk_rect;
enum { RTK_REGIONS_IN_FRAME = 0, RTK_REGIONS_PACKED = 1 };

int rtk_render_regions(rtk_accel *accel, const rtk_render_params *p, const rtk_rect *rects /* host */, int32_t n_rects,
                       int layout, float *rgb /* host */, rtk_counters *counters /* may be NULL: totals */);
int rtk_render_regions_device(rtk_accel *accel, const rtk_render_params *p, const rtk_rect *rects /* HOST */, int32_t n_rects,
                              int layout, float *d_out /* device */, void *hip_stream);

/* ---- what the camera rays hit: first-hit depth, position, normal, albedo, barycentrics and ids as planes ----
 * hit<F> (render/hit.hpp:9-21) of `accel.template intersect<true>(ray)` for the camera ray of every pixel (render/render.hpp:35-64),
 * written field by field into separate arrays, for n_views cameras in one launch: what a depth map, a denoiser's feature
 * buffers or an id mask need, without the detour over 24 B of ray and 32 B of rtk_hit per pixel.
 * Contract, per pixel (px, py) of view v: r = the ray rtk_camera_rays(.., sample) gives for that pixel after
 * rtk_accel_set_camera(views[v]) -- pixel centres at spp == 1, otherwise the jitter of root key (seed, py * width + px inside the
 * view, sample) -- and h = intersect<cull = true>(r).  Every plane but `albedo` holds, bit for bit, the corresponding field of
 * rtk_accel_intersect(cull = 1) on those rays (`position` = r.origin + (h.t * r.direction) in float, kd_tree_simd.hpp:254; `material`
 * = the material index of h.mesh), and on a miss what rtk_accel_intersect writes there.  `albedo` on a hit: for a material of kind
 * RTK_MAT_TEXTURE sample(texture, hit, uvs), the very value color_hit multiplies the light into (render.hpp:234-235); for every
 * other kind the material's `albedo` as rtk_accel_get_materials returns it.
 * First hit only and ONE sample per call: the caller averages or picks.  Nothing behind the first hit (no reflection, no
 * refraction), no rectangles inside the call, one size for all views, no sharding (world_size > 1 is refused: deal whole views to
 * ranks), no counters.
 * The call reads the live state -- camera, geometry after rtk_accel_update_*, materials, textures, texels, uvs, background -- and
 * changes none of: the accel's camera, the cost-feedback launch orders, RTK_TRACE_AUTO's verdict, the frame counters
 * (rtk_render_last_counters, rtk_debug_counter_fills and the counter block a steady frame relies on).
 * On an RTK_TRAVERSAL_FAST accel `depth` and the hit / miss pattern are those of the parity mode; the other planes carry the tie
 * caveat of RTK_TRAVERSAL_FAST above (the leaf order is chosen per wave, and a wave here is an 8x8 pixel block of a view).
 * What runs: one kernel (csrc/gbuffer.hip), one wave per 8x8 pixel block of a view, the blocks anchored at the view's corner; a
 * wave none of whose rays enters the tree's root box writes its miss values and ends.  Only the planes asked for are written.  A
 * call of more than 2^30 blocks is cut into launches of whole views.
 * trace_mode, max_ray_depth, diffuse_rays, the biases, sample_begin and sample_count of *p are validated as a frame validates them
 * and otherwise not consulted.
 * Errors, in this order: a NULL accel, p or out; what rtk_render_frame refuses for *p; sample outside [0, spp); world_size > 1,
 * collect_stats != 0, n_views < 0; NULL views with n_views != 1; all eight planes NULL; more than 2^56 pixels -> RTK_ERR_INVALID.
 * Then n_views == 0 -> RTK_OK, nothing touched, device or not.  Then (device variant) a plane pointer or view table that is not 4-byte
 * aligned -> RTK_ERR_INVALID.  Then RTK_ERR_NO_DEVICE.
 * The device variant is stream-ordered, waits (on the device) for the geometry of the last update like every other entry point,
 * allocates nothing and never blocks the host once the accel is resident.  Stream capture is neither claimed nor tested.  The
 * host variant stages views and planes in buffers the accel owns (they grow with head room and never shrink) and is synchronous. */
typedef struct {            /* any pointer may be NULL = plane not wanted; at least one must be set.  [n_views][h][w] each */
    float    *depth;        /* hit<F>::t of the camera ray (ray parameter; the camera rays are unit length); miss: -1 */
    float    *position;     /* [..][3] ray.origin + (t * ray.direction), kd_tree_simd.hpp:254; miss: 0 0 0 */
    float    *normal;       /* [..][3] hit<F>::hit_normal exactly as rtk_hit.normal (normalize_hit_normal honoured); miss: 0 0 0 */
    float    *albedo;       /* [..][3] see above; miss: the accel's background */
    float    *bary;         /* [..][2] u, v; miss: 0 0 */
    uint32_t *tri, *mesh, *material;   /* rtk_hit.tri / .mesh, and the mesh's material index; miss: 0xFFFFFFFF */
} rtk_gbuffer;              /* 64 bytes */

int rtk_render_gbuffer(rtk_accel *accel, const rtk_render_params *p, int32_t sample,
                       const rtk_view *views /* host; NULL = the accel's camera, n_views must be 1 */, int32_t n_views,
                       const rtk_gbuffer *out /* host planes */);
int rtk_render_gbuffer_device(rtk_accel *accel, const rtk_render_params *p, int32_t sample,
                              const rtk_view *d_views /* DEVICE, 4-byte aligned; NULL as above */, int32_t n_views,
                              const rtk_gbuffer *out /* struct on the HOST, DEVICE plane pointers, 4-byte aligned */, void *hip_stream);

/* ---- guides seen through mirrors and glass: the planes of the first surface that is actually SHADED ----
 * rtk_render_gbuffer describes a mirror or glass pixel by the mirror's own surface; color_hit (render/render.hpp:239-301) shades
 * what the mirror shows.  This call follows the specular chain of every camera ray -- the reflection ray off a reflective
 * material (render.hpp:239-250), the refraction ray through a refractive one (:252-292; its weight 1 - fresnel is never below
 * 1/2, :300-301) or its reflection ray under total internal reflection (:266-271) -- to the first surface of any other kind, and
 * writes that surface's planes, placed in the "virtual" world in which it lies on a straight line behind the mirror.
 * Contract, per pixel (px, py) of view v; all arithmetic is float, in the order written, without contraction:
 *   ray = the pixel's camera ray (as rtk_render_gbuffer);  L = 0.0f;  M = identity (3x3);  k = 0;  mirrored = false
 *   h = intersect<cull = true>(ray)
 *   loop:
 *     h is a miss                      -> end NO SURFACE
 *     k == max_ray_depth               -> end NO SURFACE   (color_hit returns the background there, render.hpp:138-139)
 *     L = L + h.t;  P = ray.o + (h.t * ray.d)
 *     material kind of h.mesh:
 *       RTK_MAT_REFLECTIVE: next = reflection of ray.d off hit_normal at P with reflection_bias (render.hpp:240-242);
 *                           m = hit_normal;  fold(m)
 *       RTK_MAT_REFRACTIVE: R = the refraction at P (render.hpp:252-292: i = normalized(ray.d), n = normalized(smooth_shading ?
 *                           hit_normal : face_normal), the biases of *p)
 *                           total internal reflection: next = R's reflection ray;  m = n;  fold(m)
 *                           otherwise                : next = R's refraction ray;  M unchanged
 *       anything else      -> end SURFACE
 *     k = k + 1;  ray = next;  h = intersect<cull = false>(ray)
 *   fold(m):  w_i = (M_i0 * m.x + M_i1 * m.y) + M_i2 * m.z;   M_ij = M_ij - ((2.0f * w_i) * m_j);   mirrored = true
 * On SURFACE: depth = L;  position = o0 + (L * d0) over the CAMERA ray's origin and direction;  normal = the end hit's hit_normal,
 * bit for bit, when `mirrored` is false, otherwise vn_i = (M_i0 * n.x + M_i1 * n.y) + M_i2 * n.z of it;  every other plane holds
 * the end hit's fields exactly as rtk_render_gbuffer defines them for a first hit, over the chain's last ray (surface_position =
 * ray.o + (h.t * ray.d)).  On NO SURFACE the planes take the miss values below.  bounces = k and last_ray are written either way
 * (with max_ray_depth == 0 every pixel that hits anything is NO SURFACE, as color_hit shades it).
 * What follows: for planar mirrors `position` and `normal` are exactly the mirror image of the shaded point, seen along a straight
 * line -- a fixed world point whatever the camera does -- so rtk_temporal_accumulate[_clamped] and rtk_denoise_frame take depth,
 * position, normal and mesh of this call in place of rtk_gbuffer's without any change; and a pixel with k == 0 holds
 * rtk_render_gbuffer's bits in every shared plane.  For curved mirrors and for refraction it is the usual straight-line
 * approximation: the virtual point moves with the camera, and the temporal step's mesh, normal and plane tests still guard it.
 * last_ray with cull = (bounces == 0) reproduces the end hit through rtk_accel_intersect.
 * Out of scope: moving geometry seen in a mirror (rtk_render_motion over the end hit's tri / bary gives a real, not a virtual,
 * previous position), the reflection branch of a refracting surface and the Fresnel weight, more than one sample per call,
 * sharding, rectangles.
 * Views, sizes, `sample`, the cut into launches of whole views, the live state that is read and the state that is left alone, the
 * stream order, the host variant's staging: rtk_render_gbuffer's, word for word.  The RTK_TRAVERSAL_FAST tie caveat compounds
 * along the chain: only k == 0 pixels keep the parity mode's depth.  *p is validated as rtk_render_gbuffer validates it; beyond
 * that max_ray_depth, reflection_bias and refraction_bias are CONSULTED (non-finite biases are not refused: they flow into the rays).
 * What runs: one kernel (csrc/gbuffer_specular.hip), one wave per 8x8 pixel block of a view; a loop of at most max_ray_depth + 1
 * wave-cooperative closest-hit queries, in which lanes whose chain has ended take no part.
 * Errors, in this order: a NULL accel, p or out; what rtk_render_frame refuses for *p; sample outside [0, spp); world_size > 1,
 * collect_stats != 0, n_views < 0; NULL views with n_views != 1; all twelve planes NULL; more than 2^56 pixels -> RTK_ERR_INVALID.
 * Then n_views == 0 -> RTK_OK, nothing touched, device or not.  Then (device variant) a plane pointer or view table that is not 4-byte
 * aligned -> RTK_ERR_INVALID.  Then RTK_ERR_NO_DEVICE. */
typedef struct {               /* any pointer may be NULL = plane not wanted; at least one set.  [n_views][h][w] each */
    float    *depth;           /* L, the path length (above); no surface: -1 */
    float    *position;        /* [..][3] virtual position; no surface: 0 0 0 */
    float    *normal;          /* [..][3] virtual normal; no surface: 0 0 0 */
    float    *surface_position;/* [..][3] the end hit's real position; no surface: 0 0 0 */
    float    *surface_normal;  /* [..][3] the end hit's hit_normal, as rtk_hit.normal; no surface: 0 0 0 */
    float    *albedo;          /* [..][3] as rtk_gbuffer.albedo, of the end hit; no surface: the accel's background */
    float    *bary;            /* [..][2] of the end hit; no surface: 0 0 */
    uint32_t *tri, *mesh, *material;   /* of the end hit; no surface: 0xFFFFFFFF */
    uint32_t *bounces;         /* k: secondary rays traced for this pixel, 0..max_ray_depth */
    float    *last_ray;        /* [..][6] origin, direction of the chain's last ray (the camera ray when k == 0) */
} rtk_gbuffer_specular;        /* 96 bytes */

int rtk_render_gbuffer_specular(rtk_accel *accel, const rtk_render_params *p, int32_t sample,
                                const rtk_view *views /* host; NULL = the accel's camera, n_views must be 1 */, int32_t n_views,
                                const rtk_gbuffer_specular *out /* host planes */);
int rtk_render_gbuffer_specular_device(rtk_accel *accel, const rtk_render_params *p, int32_t sample,
                                       const rtk_view *d_views /* DEVICE, 4-byte aligned; NULL as above */, int32_t n_views,
                                       const rtk_gbuffer_specular *out /* struct on the HOST, DEVICE plane pointers, 4-byte aligned */,
                                       void *hip_stream);

/* ---- a frame whose pixel blocks stop sampling once they have converged ----
 * The sample loop of tile_worker (render/render.hpp:30-77: for every pixel, for sample in [0, samples_per_pixel): camera ray,
 * intersect, color_hit, pixel_sum += colour; then pixel_sum / samples_per_pixel) cut short per 8x8 pixel block of the frame's own
 * grid (edge blocks are partial).  p->spp is the ceiling.  Blocks are judged at the checkpoints min_samples, min_samples + step,
 * ..., and spp itself as the last one (the last round may be shorter than step).
 * Contract:
 *  1. samples[px] is one of the checkpoints and equal over a block.  rgb[px] is, bit for bit, the pixel rtk_render_frame leaves
 *     with the same parameters and spp = samples[px] (a sample's jitter and RNG keys depend on the seed, the pixel index and the
 *     sample, not on spp, for spp >= 2; the sum is kept in sample order and divided by float(samples[px])).  This holds against
 *     any engine and is claimed for RTK_TRAVERSAL_REFERENCE accels; RTK_TRAVERSAL_FAST accels carry the tie caveat that
 *     rtk_accel_radiance states.
 *  2. counters.rays is the sum, over the checkpoints n, of what rtk_render_regions(spp = n, RTK_TRACE_STREAM) reports for the
 *     blocks that ended at n; counters.primary is the sum of samples[px].  rtk_render_last_counters reports the call (the call
 *     fills the accel's counter block as a regions call does; rtk_render_last_critical_path reports 0 for it).
 *  3. The statistic.  Per sample colour c: y = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b in float, without contraction.  Per
 *     pixel, in double and in sample order: S1 += (double)y, S2 += (double)y * (double)y.  At a checkpoint n, for every valid pixel
 *     i of block B in row-major order, all in double: m_i = S1 / n, v_i = max(0, (S2 - S1 * S1 / n) / (n - 1)) / n, e_i = sqrt(v_i),
 *     and E_B = (sum e_i / |B|) / max(sum m_i / |B|, (double)floor).  The block stops iff E_B <= (double)threshold evaluates true; a
 *     NaN keeps sampling to the ceiling (both max() pass a NaN on).  noise[px] = (float)e_i at the pixel's final count.
 *  4. The call reads the live state -- camera, updated geometry, lights, materials, textures, background -- and leaves alone the
 *     accel's camera, the cost tables of frames, views and regions, the regions table and RTK_TRACE_AUTO's verdict.
 * What runs (csrc/adaptive.hip): round by round, the active pixels in chunks of at most 2^20 (RTK_ADAPTIVE_CHUNK_PIXELS), per
 * chunk and sample the camera rays, the streaming pipeline of rtk_accel_radiance and a kernel that adds the colours into the sums
 * and the statistic; at the checkpoint one wave per active block decides.  The order of the blocks in a later round's list is not
 * deterministic; no result depends on it.  The workspace (24 B per pixel) belongs to the accel and grows with head room.
 * Errors, in this order, all RTK_ERR_INVALID: a NULL accel, p, ap or rgb; what rtk_render_frame refuses for *p; trace_mode other
 * than RTK_TRACE_AUTO or RTK_TRACE_STREAM; spp < 2; sample_begin or sample_count not 0; collect_stats != 0; world_size > 1;
 * min_samples < 2 or > spp; step < 1; a threshold that is non-finite or negative; a floor that is non-finite or not positive; a
 * frame of more than 2^31 pixels.  Then RTK_ERR_NO_DEVICE.  A refused call leaves the accel unchanged and usable.
 * The device variant is stream-ordered: everything is enqueued on hip_stream.  It BLOCKS THE HOST once per round but the last, to
 * read back one 64-bit word (the pixels and blocks still active), and may block again, once, to grow the workspace.  It is NOT
 * stream-capturable.  d_samples and d_noise may be NULL.  Resuming an earlier adaptive render with a higher ceiling is not offered. */
typedef struct {
    int32_t min_samples;   /* >= 2: every pixel gets at least this many */
    int32_t step;          /* >= 1: samples per round after the first */
    float   threshold;     /* finite, >= 0: a block stops once E_B <= threshold */
    float   floor;         /* finite, > 0: lower bound of the block mean in E_B's denominator */
} rtk_adaptive_params;     /* 16 bytes */

int rtk_render_adaptive(rtk_accel *accel, const rtk_render_params *p, const rtk_adaptive_params *ap,
                        float *rgb /* host [h][w][3] */, uint32_t *samples /* host [h][w], may be NULL */,
                        float *noise /* host [h][w], may be NULL */, rtk_counters *counters /* may be NULL */);
int rtk_render_adaptive_device(rtk_accel *accel, const rtk_render_params *p, const rtk_adaptive_params *ap,
                               float *d_rgb, uint32_t *d_samples, float *d_noise, void *hip_stream);

/* ---- a frame of a fixed sample count, with its noise plane ----
 * What rtk_denoise_frame wants beside the frame: the `noise` plane of rtk_render_adaptive, for a caller who wants every pixel to
 * take all p->spp samples, at the speed of a frame.  An adaptive render with min_samples = spp gives the same two planes, one
 * sample of one chunk at a time; this call renders a streamed frame and takes the statistic where the samples already lie.
 * Contract:
 *  1. rgb is, bit for bit, what rtk_render_frame leaves with the same *p, through any engine; counters.rays and counters.primary
 *     are the frame's.  rtk_render_last_counters reports the call, rtk_render_last_critical_path reports 0 for it.  This is claimed
 *     for RTK_TRAVERSAL_REFERENCE accels; RTK_TRAVERSAL_FAST accels carry the tie caveat that rtk_accel_radiance states.
 *  2. noise[px] = (float)e_i of item 3 of rtk_render_adaptive's contract at n = spp: per sample colour c, as radiance returns it
 *     (+0 + c), y = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b in float, without contraction; S1 += (double)y and
 *     S2 += (double)y * (double)y in double, in sample order; then v = max(0, (S2 - S1 * S1 / n) / (n - 1)) / n and e = sqrt(v) in
 *     double (max passes a NaN on).  noise is therefore, bit for bit, the noise plane of rtk_render_adaptive with the same *p and
 *     min_samples = spp: both are built without contraction from the same double expressions and the same square root.
 *  3. The call reads the live state -- camera, updated geometry, lights, materials, textures, background -- and leaves alone the
 *     accel's camera, the cost tables of frames, views and regions, the regions table and RTK_TRACE_AUTO's trial and verdict: it
 *     neither takes part in the trial nor abandons it, beyond what growing the queues it shares with the frames already does.  On
 *     the accel's counter block (rtk_debug_counter_fills, the block a steady frame relies on) it has the effect of an
 *     RTK_TRACE_STREAM frame in its place.
 *  4. The call always runs through the streaming engine: RTK_TRACE_AUTO means RTK_TRACE_STREAM here, as for rtk_accel_radiance.
 * What runs (csrc/frame_noise.hip): the batches of an RTK_TRACE_STREAM frame, and behind every batch's last kernel one more, a
 * thread per pixel, that adds the batch's sample luminances to the pixel's two sums, or, in the batch that ends at spp, writes the
 * noise.  The sums (16 B per pixel) are the workspace of rtk_render_adaptive, which belongs to the accel and grows with head room.
 * Overflow.  A streamed frame whose queues overflow is normally redone by the megakernel, which has no statistic.  This call reads
 * the overflow flag back and, if it is set, redoes itself as rtk_render_adaptive with min_samples = spp, step = 1, threshold = 0 and
 * floor = 1: by items 1 and 2 the same rgb, noise, rays and primary; only the time differs (and the counter block is filled a
 * second time).  rtk_debug_noise_fallbacks counts such calls.
 * Errors, in this order, all RTK_ERR_INVALID: a NULL accel, p, rgb or noise (a caller without use for the noise has
 * rtk_render_frame); what rtk_render_frame refuses for *p; trace_mode other than RTK_TRACE_AUTO or RTK_TRACE_STREAM; spp < 2;
 * sample_begin or sample_count not 0 (the statistic of a progressive frame would need a second running buffer in the caller's
 * hands: not offered); collect_stats != 0; world_size > 1; a frame of more than 2^31 pixels.  Then RTK_ERR_NO_DEVICE.  A refused
 * call leaves the accel unchanged and usable.
 * The device variant is stream-ordered on hip_stream.  It may block the host to grow a workspace, and it BLOCKS THE HOST ONCE AT
 * ITS END to read back one 32-bit word, whether any queue overflowed.  It is NOT stream-capturable.  The host variant stages rgb
 * and noise in a buffer the accel owns and is synchronous. */
int rtk_render_frame_noise(rtk_accel *accel, const rtk_render_params *p, float *rgb /* host [h][w][3] */,
                           float *noise /* host [h][w] */, rtk_counters *counters /* may be NULL */);
int rtk_render_frame_noise_device(rtk_accel *accel, const rtk_render_params *p, float *d_rgb, float *d_noise, void *hip_stream);
/* Diagnostic, like rtk_debug_counter_fills: the rtk_render_frame_noise calls on this accel that were redone because a queue
 * overflowed, since it was built.  Needs no device. */
int rtk_debug_noise_fallbacks(rtk_accel *accel, uint64_t *count);

/* ---- an edge-avoiding filter of a frame, guided by the g-buffer ----
 * Consumes what rtk_render_gbuffer and rtk_render_adaptive write: a 5x5 a-trous filter of `rgb` along the surfaces that `normal`,
 * `position` and `depth` describe, weighted by the variance that `noise` gives.  The reference has no denoiser; the arithmetic is
 * spelt out here and pinned, bit for bit, by tests/denoise_model.py.  The calls take no accel: the filter depends on no scene state.
 * Inputs are n_images images of width x height, one behind the other: rgb, normal, position and albedo [n_images][h][w][3], depth
 * and noise [n_images][h][w], in the layouts rtk_gbuffer and rtk_render_adaptive write.  noise may be NULL, albedo may be NULL.
 * The output is rgb_out [n_images][h][w][3].
 * All arithmetic is float, in the order written, without contraction.  A pixel is a HIT iff `depth >= 0.0f` evaluates true (a miss,
 * -1, or a NaN is not a hit).  lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b.  max(x, f) = x > f ? x : f.
 * Prologue, per pixel p.  With an albedo plane: a = max(albedo, albedo_floor) per channel; on a hit c = rgb / a per channel, on a
 *   miss c = rgb.  Without one c = rgb.  var = 1.0f without a noise plane, noise * noise with one; on a hit with albedo then
 *   var = var / (la * la) with la = lum(a).
 * Iterations k = 0 .. iterations - 1 with s = 1 << k; h = {1/16, 1/4, 3/8, 1/4, 1/16}, sl2 = sigma_luminance * sigma_luminance,
 *   sp2 = sigma_plane * sigma_plane.  A miss pixel's c and var pass through unchanged.  For a hit pixel p:
 *   1. lp = lum(c_p), den = sl2 * var_p + 1e-8f, sum_c = sum_v = sum_w = +0.
 *   2. The taps dy = -2..2 (outer loop), dx = -2..2 (inner loop), q = p + s * (dx, dy).  A tap outside the image is skipped (never
 *      clamped, never wrapped, never another image's pixel); a tap that is not a hit is skipped.
 *   3. The centre tap dx = dy = 0 gets w = 0.140625f.
 *   4. Every other tap: t = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z; t = t > 0 ? t : 0; normal_power_log2 times t = t * t;
 *      D = P_q - P_p; pd = (n_p.x * D.x + n_p.y * D.y) + n_p.z * D.z; wd = 1.0f / (1.0f + (pd * pd) / sp2);
 *      dl = lum(c_q) - lp; wl = 1.0f / (1.0f + (dl * dl) / den); w = (((h[dy + 2] * h[dx + 2]) * t) * wd) * wl.
 *   5. Per channel sum_c = sum_c + w * c_q; sum_v = sum_v + (w * w) * var_q; sum_w = sum_w + w.
 *   6. After the taps c_p' = sum_c / sum_w and var_p' = sum_v / (sum_w * sum_w).
 *   Every iteration reads the previous iteration's c and var of all pixels; the guide planes never change.
 * Epilogue.  On a hit with albedo rgb_out = c * a, otherwise rgb_out = c: a miss pixel leaves with the bits it came with.
 * rgb_out may be the very pointer rgb (in place); any other overlap of the output or the workspace with a plane is the caller's fault.
 * What runs (csrc/denoise.hip): k_denoise_prepare packs (c, var) and the guides into 16-byte records in the workspace; then one
 * launch of k_denoise_atrous per iteration, one 256-thread workgroup per 16x16 pixel tile of an image.  Steps up to
 * RTK_DENOISE_LDS_MAX_STEP (environment, read once per process; 0 = never, default 4, at most 8) load the tile with its halo of 2 * s pixels into LDS
 * and run the taps from there, larger steps read the records from global memory; the results do not depend on it.  The last
 * iteration applies the epilogue and writes rgb_out.
 * The caller supplies the workspace of the device variant: rtk_denoise_workspace_bytes says how much (at most 64 B per pixel; 0
 * for n_images == 0); it needs 16-byte alignment and is scratch, its contents before and after a call mean nothing.  The planes need
 * 4-byte alignment.  The device variant is stream-ordered on the current device, allocates nothing and never blocks the host.
 * Stream capture is neither claimed nor tested.  The host variant stages planes and workspace in device buffers of its own, which
 * it frees, and is synchronous.
 * Errors, in this order: a NULL p, in or (rtk_denoise_workspace_bytes) bytes -> RTK_ERR_INVALID.  Then width < 1 or height < 1;
 * more than 2^28 pixels per image; iterations outside [1, 8]; normal_power_log2 outside [0, 8]; a sigma_luminance, sigma_plane or
 * albedo_floor that is non-finite or not positive; n_images < 0; more than 2^31 pixels in total -> RTK_ERR_INVALID.  Then
 * n_images == 0 -> RTK_OK, nothing touched, device or not.  Then a NULL rgb, normal, position, depth or output -> RTK_ERR_INVALID.
 * Then (device variant) a plane that is not 4-byte aligned; a NULL workspace or one that is not 16-byte aligned; a workspace
 * smaller than asked for -> RTK_ERR_INVALID.  Then RTK_ERR_NO_DEVICE. */
typedef struct {
    int32_t width, height;        /* of every image; at most 2^28 pixels */
    int32_t iterations;           /* 1..8: steps 1, 2, 4, ... */
    int32_t normal_power_log2;    /* 0..8: the normal weight is max(n_p . n_q, 0) to the power 2^this */
    float   sigma_luminance;      /* finite, > 0: in standard deviations of the pixel's own luminance */
    float   sigma_plane;          /* finite, > 0: distance from the tangent plane of p, in scene units */
    float   albedo_floor;         /* finite, > 0: lower bound of the albedo that the colour is divided by */
    int32_t reserved;
} rtk_denoise_params;             /* 32 bytes */
typedef struct { const float *rgb, *noise, *albedo, *normal, *position, *depth; } rtk_denoise_inputs;   /* 48 bytes */

int rtk_denoise_workspace_bytes(const rtk_denoise_params *p, int32_t n_images, size_t *bytes);
int rtk_denoise_frame(const rtk_denoise_params *p, int32_t n_images, const rtk_denoise_inputs *in /* host planes */,
                      float *rgb_out /* host */);
int rtk_denoise_frame_device(const rtk_denoise_params *p, int32_t n_images,
                             const rtk_denoise_inputs *in /* struct on the HOST, DEVICE planes */, float *d_rgb_out,
                             void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* ---- temporal accumulation: reproject and blend a frame's history ----
 * The temporal step between rtk_render_frame_noise / rtk_render_gbuffer and rtk_denoise_frame: the new frame `cur` is blended with
 * the accumulated frame `prev` of the previous camera, fetched where each pixel's world position `P` lay in that camera's image.
 * Only camera motion is reprojected: the planes hold world positions, so a static scene under a moving camera needs no motion
 * vectors.  The reference has no such step; the arithmetic is spelt out here and pinned, bit for bit, by tests/temporal_model.py.
 * The calls take no accel: they depend on no scene state.  One image per call; both frames have the size and the fov of *p.
 * Planes: rgb, position and normal are [h][w][3]; noise, depth, length and mesh are [h][w], in the layouts rtk_gbuffer and
 * rtk_render_frame_noise write.  out->rgb, out->noise and out->length of one call are prev->rgb, prev->noise and prev->length of
 * the next; the caller keeps the guides (position, normal, depth, mesh) and the view of the last frame.  prev == NULL starts a history.
 * Optional planes come as families: cur->noise, out->noise and (with a prev) prev->noise are all set or all NULL; cur->mesh and
 * (with a prev) prev->mesh are both set or both NULL.
 * Aliasing: out->rgb may be cur->rgb and out->noise may be cur->noise (they are read only at the pixel that is written).  Any
 * overlap of an output with a plane of prev is the caller's fault, because neighbours are read there: callers ping-pong two sets.
 * All arithmetic is float, in the order written, without contraction.  max(x, f) = x > f ? x : f.  A pixel is a HIT iff
 * `depth >= 0.0f` evaluates true.  Host-side scalars, computed as for a frame's camera rays: aspect = (float)w / (float)h;
 * th = tanf((float)(fov_degrees * (pi / 180)) / 2.0f); wf = (float)w, hf = (float)h, nmax = (float)max_history.
 * Per pixel p with colour c, var_c = noise_p * noise_p (1.0f without noise planes), P, n and depth_p:
 *   1. No history -- prev == NULL, p is no hit, or step 2 or 3 finds nothing: out.rgb = c and out.noise = noise_p (the bits pass
 *      through), out.length = 1.0f.
 *   2. Project P into the previous view (C = prev->view->position, M = its matrix, row-major): D = P - C;
 *      cx = (M0 * D.x + M1 * D.y) + M2 * D.z, cy likewise with M3..M5, cz with M6..M8.  (The inverse of the camera rays'
 *      transpose(M) * dir for an orthonormal M; for any other M an approximation that the tests of step 3 still guard.)
 *      Require `cz < 0.0f` to evaluate true.  iz = -cz; qx = cx / iz; qy = cy / iz; ux = (qx / th) / aspect; uy = qy / th;
 *      fx = ((ux + 1.0f) * 0.5f) * wf - 0.5f; fy = ((1.0f - uy) * 0.5f) * hf - 0.5f.  Require
 *      `fx > -1.0f && fx < wf && fy > -1.0f && fy < hf` to evaluate true (a NaN or an infinity fails).  Only then:
 *      x0f = floorf(fx), y0f = floorf(fy), x0 = (int)x0f, y0 = (int)y0f, tx = fx - x0f, ty = fy - y0f.
 *   3. Four taps q = (x0 + i, y0 + j), j = 0, 1 the outer and i = 0, 1 the inner loop, w = (j ? ty : 1.0f - ty) * (i ? tx : 1.0f - tx).
 *      A tap is skipped when it lies outside the image; when `prev.depth_q >= 0.0f` is not true; when `prev.length_q >= 1.0f` is not
 *      true (zero-filled or NaN history); when mesh planes are given and prev.mesh_q != cur.mesh_p; when
 *      t = (n.x * nq.x + n.y * nq.y) + n.z * nq.z fails `t >= normal_min_dot`; when pd = (n.x * E.x + n.y * E.y) + n.z * E.z with
 *      E = Pq - P fails `fabsf(pd) <= plane_tolerance * depth_p`.  An accepted tap adds, with vq = noise_q * noise_q (or 1.0f):
 *      sum_c += w * c_q per channel; sum_v += (w * w) * vq; sum_l += w * length_q; sum_w += w.  History exists iff sum_w > 0.0f.
 *   4. Blend: hc = sum_c / sum_w; hv = sum_v / (sum_w * sum_w); N = sum_l / sum_w + 1.0f, then N = N < nmax ? N : nmax;
 *      a = max(1.0f / N, alpha_min); om = 1.0f - a; out.rgb = (om * hc) + (a * c) per channel;
 *      var = ((om * om) * hv) + ((a * a) * var_c); out.noise = (float)sqrt((double)var); out.length = N.
 * Non-finite colours in the history are the caller's business and propagate.  The positions should be those of the pixel centres:
 * a g-buffer of spp = 1 (with spp > 1 the ray of sample 0 is jittered inside its pixel, and a camera standing still would blend
 * every pixel with its neighbours).
 * What runs (csrc/temporal.hip): one launch of k_temporal_accumulate, one 256-thread workgroup per 16x16 pixel tile, the workgroups
 * striding over the tiles.  No workspace, no LDS, no atomics.
 * Errors, in this order, all RTK_ERR_INVALID: a NULL p, cur or out; the parameters in the struct's order (width, height outside
 * [1, 16384]; a fov_degrees that is not finite or not inside (0, 180); alpha_min not finite or outside (0, 1]; plane_tolerance not
 * finite or not positive; normal_min_dot not finite or outside [-1, 1]; max_history outside [1, 1048576]); a NULL cur->rgb,
 * position, normal or depth, or a NULL out->rgb or out->length; with a prev, a NULL rgb, length, position, normal, depth or view
 * of it; a broken noise family, then a broken mesh family; (device variant) a plane that is not 4-byte aligned.  Then
 * RTK_ERR_NO_DEVICE.
 * The device variant is stream-ordered on the current device, allocates nothing, never blocks the host and is one launch; the
 * structs, prev->view among them, are read on the host before it returns.  Stream capture is neither claimed nor tested.  The host
 * variant stages the planes in device buffers of its own, which it frees, and is synchronous. */
typedef struct {
    int32_t width, height;     /* 1..16384 each */
    double  fov_degrees;       /* of BOTH frames, as rtk_render_params.fov_degrees */
    float   alpha_min;         /* finite, 0 < alpha_min <= 1: lower bound of the new frame's weight */
    float   plane_tolerance;   /* finite, > 0: |n_p . (P_q - P_p)| <= plane_tolerance * depth_p */
    float   normal_min_dot;    /* finite, in [-1, 1]: n_p . n_q >= normal_min_dot */
    int32_t max_history;       /* 1..1048576: cap of the history length */
} rtk_temporal_params;         /* 32 bytes */
typedef struct { const float *rgb, *noise, *position, *normal, *depth; const uint32_t *mesh; } rtk_temporal_frame;   /* 48 bytes: the new frame */
typedef struct { const float *rgb, *noise, *length, *position, *normal, *depth; const uint32_t *mesh;
                 const rtk_view *view; /* HOST in both variants: the camera the history was rendered from */ } rtk_temporal_history;   /* 64 bytes */
typedef struct { float *rgb, *noise, *length; } rtk_temporal_outputs;                                                /* 24 bytes */

int rtk_temporal_accumulate(const rtk_temporal_params *p, const rtk_temporal_frame *cur /* host planes */,
                            const rtk_temporal_history *prev /* NULL: start a history */, const rtk_temporal_outputs *out);
int rtk_temporal_accumulate_device(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev,
                                   const rtk_temporal_outputs *out /* structs on the HOST, DEVICE planes, 4-byte aligned */,
                                   void *hip_stream);

/* ---- temporal accumulation, clamped: the history bounded by the new frame's neighbourhood ----
 * rtk_temporal_accumulate trusts any history that passes its geometric tests, whatever its colour: a shadow, a highlight or a
 * mirror image that has moved is blended in at weight 1 - 1/N.  The clamped call pulls the history's colour into the colour
 * statistics of the NEW frame around the pixel before it blends, raises the history's variance to that of the neighbourhood mean
 * where it did so, and can shorten the history there.  Structs, planes, families, scalars and steps 1 to 3 are those of
 * rtk_temporal_accumulate above, verbatim: the pass-through without history, the projection, the four guarded taps, sum_c, sum_v,
 * sum_l, sum_w, and "history exists iff sum_w > 0.0f".  All arithmetic is float, in the order written, without contraction; pinned
 * bit for bit by tests/temporal_clamp_model.py.  For a pixel p WITH history, with r = radius:
 *   3a. The box: nf = 0.0f; per channel s1 = s2 = 0.0f; sv = 0.0f.  Taps q = p + (dx, dy) in the NEW frame, dy = -r..r the outer
 *       and dx = -r..r the inner loop.  A tap is skipped when it lies outside the image (never clamped to the edge, never
 *       wrapped); when `cur.depth_q >= 0.0f` is not true; when mesh planes are given and cur.mesh_q != cur.mesh_p.  The centre tap
 *       always passes.  An accepted tap adds nf = nf + 1.0f; per channel s1 = s1 + c_q and s2 = s2 + c_q * c_q; sv = sv + var_q
 *       with var_q = noise_q * noise_q (1.0f without noise planes).
 *   3b. The bounds, per channel: m = s1 / nf; d = s2 / nf - m * m; d = d > 0.0f ? d : 0.0f; sg = (float)sqrt((double)d);
 *       e = gamma * sg; lo = m - e; hi = m + e.
 *   3c. The clamp, per channel: hc = sum_c / sum_w; hc' = hc < lo ? lo : (hc > hi ? hi : hc).  The pixel is CLAMPED iff in some
 *       channel `hc < lo` or `hc > hi` evaluated true.  A non-finite colour in the box makes the bounds non-finite, and the
 *       comparisons decide as written: a NaN bound clamps nothing.
 *   3d. The variance: hv = sum_v / (sum_w * sum_w).  On a clamped pixel also vb = (sv / nf) / nf and hv = hv > vb ? hv : vb: a
 *       history that was pulled to the neighbourhood mean is known no better than that mean, which reopens the luminance weight
 *       of rtk_denoise_frame where the history was wrong.
 *   4.  The blend of the plain call with hc' and that hv: L = sum_l / sum_w; on a clamped pixel L = L * history_keep;
 *       N = L + 1.0f, then N = N < nmax ? N : nmax; a = max(1.0f / N, alpha_min); om = 1.0f - a; out.rgb = (om * hc') + (a * c);
 *       var = ((om * om) * hv) + ((a * a) * var_c); out.noise = (float)sqrt((double)var); out.length = N.  history_keep = 1 gives
 *       the length of the plain call, 0 makes a clamped pixel start over.
 * A gamma so large that no comparison fires gives the plain call's bits.
 * Aliasing: neighbours of the new frame are read, so unlike the plain call out->rgb == cur->rgb is refused, and so is
 * out->noise == cur->noise when both are set.  Any other overlap of an output with a plane of cur or prev is the caller's fault.
 * What runs (csrc/temporal_clamp.hip): one launch of k_temporal_accumulate_clamped<radius>, one 256-thread workgroup per 16x16
 * pixel tile, the workgroups striding over the tiles; each stages its tile of the new frame with a halo of r pixels in
 * (16 + 2r)^2 * 20 bytes of LDS.  No workspace, no atomics.
 * Errors, in this order, all RTK_ERR_INVALID: a NULL p, k, cur or out; the checks of rtk_temporal_params in that struct's order;
 * radius outside [1, 3]; gamma not finite or negative; history_keep not finite or outside [0, 1]; the plane and family checks of
 * the plain call in its order; the two aliasing refusals; (device variant) a plane that is not 4-byte aligned.  Then
 * RTK_ERR_NO_DEVICE.
 * The device variant is stream-ordered on the current device, allocates nothing, never blocks the host and is one launch; the
 * structs are read on the host before it returns.  Stream capture is not claimed.  The host variant stages the planes as the plain
 * call's does and is synchronous. */
typedef struct {
    int32_t radius;        /* 1..3: the box is the (2r+1) x (2r+1) neighbourhood of the NEW frame */
    float   gamma;         /* finite, >= 0: per channel the history is clamped to mean +- gamma * standard deviation */
    float   history_keep;  /* finite, in [0, 1]: a clamped pixel keeps this share of its history length */
    int32_t reserved;      /* ignored */
} rtk_temporal_clamp;      /* 16 bytes */

int rtk_temporal_accumulate_clamped(const rtk_temporal_params *p, const rtk_temporal_clamp *k,
                                    const rtk_temporal_frame *cur /* host planes */, const rtk_temporal_history *prev,
                                    const rtk_temporal_outputs *out);
int rtk_temporal_accumulate_clamped_device(const rtk_temporal_params *p, const rtk_temporal_clamp *k, const rtk_temporal_frame *cur,
                                           const rtk_temporal_history *prev,
                                           const rtk_temporal_outputs *out /* structs on the HOST, DEVICE planes, 4-byte aligned */,
                                           void *hip_stream);

/* ---- motion: where each pixel's surface point was in the previous pose ----
 * rtk_temporal_accumulate reprojects camera motion only: it projects the g-buffer's world position through the previous view, and
 * after rtk_accel_update_vertices a surface's world position has moved, so the history of every pixel on a moved mesh fails the
 * tangent-plane test.  rtk_render_motion closes that: from a frame's `tri` and `bary` planes (rtk_gbuffer) and the vertices of the
 * PREVIOUS pose it gives `prev_position`, the point of the previous pose that each pixel's surface point was.  Handed to
 * rtk_temporal_accumulate as cur->position, the temporal contract runs unchanged in the previous frame's world: projection, mesh
 * test and tangent-plane test against the previous guides.  On request it also gives `motion`, the screen-space vector external
 * consumers expect.  Every mesh's vertex count is fixed for the accel's life, so a vertex array of any pose fits the accel's
 * CURRENT topology; the caller keeps last frame's vertices and view.  One image per call.  The reference has no such step; the
 * arithmetic is spelt out here and pinned, bit for bit, by tests/motion_model.py.
 * Planes: tri [h][w] and bary [h][w][2] as rtk_gbuffer writes them; prev_vertices [n_vertices][3], all meshes concatenated in the
 * layout of rtk_scene_desc.vertices; prev_position [h][w][3]; motion [h][w][2] (x, y).  Only the planes asked for are written.
 * The outputs may not alias the inputs or each other.
 * All arithmetic is float, in the order written, without contraction.  For each pixel (x, y), px = y * w + x:
 *   1. id = tri[px].  The pixel is a MISS iff id >= n_triangles of the accel's current topology (that of the last
 *      rtk_accel_update_geometry, else the scene's): this covers 0xFFFFFFFF and any stale or hostile id, and nothing is
 *      dereferenced with such an id.  A miss writes prev_position = 0 0 0 and both words of motion as the bits 0x7FC00000.
 *   2. i0, i1, i2 = the triangle's three global vertex ids; A, B, C = prev_vertices[i0], [i1], [i2]; u, v = bary[px];
 *      w = (1.0f - u) - v; per component P' = ((w * A) + (u * B)) + (v * C) -- u weighs vertex 1, v vertex 2 and w vertex 0, the
 *      reference's convention (kd_tree_simd.hpp:250).  A non-finite u or v propagates; it is not a miss.  prev_position = P'.
 *   3. motion: P' goes through step 2 of the temporal contract above with C and M of *prev_view and the scalars of *p, up to fx
 *      and fy.  If `cz < 0.0f` evaluates true, motion = (fx - (float)x, fy - (float)y): previous place minus present place, in
 *      pixels.  There is no range test: off-screen values pass as computed.  Otherwise both words are the miss bits.
 * The call reads the accel's live topology and nothing else of its state: the camera, the cost tables, the engine verdict and
 * the counters stay as they are.
 * What runs (csrc/motion.hip): one launch of k_motion, one thread per pixel, one 256-thread workgroup per 16x16 tile, the
 * workgroups striding over the tiles.  No workspace, no LDS, no atomics.
 * Errors, in this order, all RTK_ERR_INVALID: a NULL accel, p, tri, bary, prev_vertices or out; width or height outside
 * [1, 16384]; a fov_degrees that is not finite or not inside (0, 180); both outputs NULL; motion wanted without prev_view; (device
 * variant) a plane or the vertex array not 4-byte aligned.  Then RTK_ERR_NO_DEVICE.  A refused call changes nothing.
 * The device variant is stream-ordered, waits on the device for the last update's event as every entry point does, and allocates
 * nothing once the accel's topology tables exist: the first call on an accel that no update has touched makes them and may block
 * the host there once; otherwise the host is never blocked.  The structs and *prev_view are read on the host before it returns.
 * Stream capture is not claimed.  The host variant stages its planes on the device and is synchronous. */
typedef struct { int32_t width, height; double fov_degrees; } rtk_motion_params;      /* 16 bytes */
typedef struct { float *prev_position; /* [h][w][3] */ float *motion; /* [h][w][2] */ } rtk_motion_outputs;  /* 16 bytes; either may be NULL, not both */

int rtk_render_motion(rtk_accel *accel, const rtk_motion_params *p, const uint32_t *tri, const float *bary /* host planes */,
                      const float *prev_vertices /* host [n_vertices][3] */, const rtk_view *prev_view /* host; required iff out->motion */,
                      const rtk_motion_outputs *out /* host planes */);
int rtk_render_motion_device(rtk_accel *accel, const rtk_motion_params *p, const uint32_t *d_tri, const float *d_bary,
                             const float *d_prev_vertices /* DEVICE planes and vertices, 4-byte aligned */,
                             const rtk_view *prev_view /* HOST */, const rtk_motion_outputs *out /* struct on the HOST, DEVICE planes */,
                             void *hip_stream);

/* ---- lights, materials and background of a live accel ----
 * The reference keeps them plain mutable members of scene<F> (scene/scene.hpp:14-22, scene/light.hpp, scene/material/ *.hpp,
 * settings::background_color) and reads them when render_frame / color_hit run; so does the accel.  The two structs have the
 * layout of the tables the kernels read, so a table is one copy.
 * The contract of all three setters: after RTK_OK everything observable through the accel is, bit for bit and with the same
 * `rays`, what a fresh rtk_accel_build gives for a scene that differs only in the replaced part (same params, same environment
 * knobs): frames through every RTK_TRACE_* engine, sharded frames, rtk_render_views*, rtk_accel_radiance*, rtk_accel_occluded*
 * (its answers depend on which materials are refractive) and the counters.  The tree, rtk_accel_tree_dump, rtk_accel_intersect*
 * and rtk_camera_rays* depend on none of it and do not change.  The state survives rtk_accel_update_vertices / _update_geometry
 * and rtk_accel_set_camera, in any order.  None of the calls is stream-capturable. */
typedef struct { float position[3]; float intensity; } rtk_light;            /* scene/light.hpp; 16 bytes */
typedef struct { int32_t kind, smooth; float albedo[3]; float ior; int32_t texture; int32_t reserved; } rtk_material;  /* 32 bytes */

/* *n = the number of lights; with `out`, the first min(cap, *n) of them.  After rtk_accel_set_lights_device the table is fetched
 * from the device, which synchronises it. */
int rtk_accel_get_lights(const rtk_accel *accel, rtk_light *out /* may be NULL */, int32_t cap, int32_t *n);
/* n is free: 0, fewer, or more than ever before.  The values are taken as they are, as rtk_scene_create takes them (a negative,
 * zero, infinite or NaN intensity is the caller's business, as in the reference).
 * On an accel that has never been on a device the host variant only stores: it needs no GPU and never returns
 * RTK_ERR_NO_DEVICE.  Once the accel is on the device it SYNCHRONISES THE DEVICE AT ENTRY, as rtk_accel_update_vertices does
 * (nothing issued earlier, on any stream, can still be reading the table), then writes the table; a table that n outgrows is
 * replaced by one with head room, never by a smaller one, so a steady animation allocates nothing.
 * The device variant (d_lights in DEVICE memory, 4-byte aligned) puts an accel that is not resident yet on the device first (no
 * usable device -> RTK_ERR_NO_DEVICE), synchronises the device at entry, then copies on `hip_stream` and records the event later
 * work on any stream waits for; after entry it does not block the host.
 * The streaming workspace is sized by the light count: it grows at the next STREAM frame or radiance batch that needs it.
 * Launch order: a call that leaves the COUNT as it is keeps the cost-feedback launch order (a light that moves leaves the
 * silhouettes where they are); a changed count forgets it, because every block's cost scales with it.  RTK_TRACE_AUTO's engine
 * verdict is kept by both.  Neither changes a result.
 * Errors: NULL accel, n < 0, NULL lights with n > 0 -> RTK_ERR_INVALID; then (device variant) RTK_ERR_NO_DEVICE; RTK_ERR_HIP only
 * from the runtime, and the accel is then as it was. */
int rtk_accel_set_lights(rtk_accel *accel, const rtk_light *lights /* host */, int32_t n);
int rtk_accel_set_lights_device(rtk_accel *accel, const rtk_light *d_lights /* DEVICE, 4-byte aligned */, int32_t n, void *hip_stream);

int rtk_accel_get_materials(const rtk_accel *accel, rtk_material *out /* [n_materials] */);
/* n must equal the scene's n_materials: the meshes' material indices are fixed (rtk_accel_update_geometry).  Validation is
 * rtk_scene_create's: kind in [RTK_MAT_DIFFUSE, RTK_MAT_TEXTURE]; for RTK_MAT_TEXTURE 0 <= texture < n_textures, for every other
 * kind texture is stored as -1; `reserved` is ignored and stored as 0.  n_textures is the LIVE count: the textures themselves are
 * replaced through rtk_accel_set_textures ("textures and uvs of a live accel", below).
 * On an accel that has never been on a device the call only stores and needs no GPU.  On a resident accel it synchronises the
 * device at entry and writes the table.  What the launch paths derive from "some material is refractive" (early shadow exit, the
 * unlit-shadow skip, the lean / general kernel choice, the streaming plan, the one-launch path of rtk_render_views) follows; the
 * cost-feedback launch order and RTK_TRACE_AUTO's engine trial start over.
 * When the SET of refractive materials changed on a resident RTK_TRAVERSAL_FAST accel (with RTK_FAST_OCCLUDERS), the opaque-only
 * occlusion tree is re-made on the device from the active tree (csrc/occluders.hip): the host blocks once more to read one count
 * per leaf (and until the few hundred nodes it makes from them have left its memory), the copy is built into spare buffers and
 * swapped in at the end, and later work on any stream waits for the event recorded behind it.  The per-triangle opaque flags that later rtk_accel_update_vertices calls read are rewritten too.
 * Errors, in this order: NULL accel or materials; n != n_materials; a bad kind or texture index -> RTK_ERR_INVALID.  Then
 * RTK_ERR_HIP only from the runtime.  Never RTK_ERR_NO_DEVICE on an accel that is not resident.  A refused call leaves the accel
 * exactly as it was. */
int rtk_accel_set_materials(rtk_accel *accel, const rtk_material *materials /* host [n_materials] */, int32_t n);

/* The background is launch-argument data, like the camera: the calls touch no device memory, synchronise nothing, never return
 * RTK_ERR_NO_DEVICE and take the values as they are (a -0.0 and a denormal round-trip by their bits).  Frames already enqueued
 * keep the background they were launched with.  NULL accel or rgb -> RTK_ERR_INVALID. */
int rtk_accel_get_background(const rtk_accel *accel, float rgb[3]);
int rtk_accel_set_background(rtk_accel *accel, const float rgb[3]);

/* ---- textures and uvs of a live accel ----
 * scene::textures (scene/scene.hpp:18) and the meshes' uvs are plain mutable members in the reference as well.  The contract of
 * every setter below is that of the section above: after RTK_OK everything observable through the accel is, bit for bit and with
 * the same `rays`, what a fresh rtk_accel_build gives for a scene that differs only in the replaced part (same params, same
 * environment knobs): frames through every RTK_TRACE_* engine, sharded frames, rtk_render_views*, rtk_render_regions*,
 * rtk_accel_radiance* and the counters.  The tree, rtk_accel_tree_dump, rtk_accel_intersect*, rtk_accel_occluded* and
 * rtk_camera_rays* depend on none of it and do not change.  The state survives rtk_accel_update_vertices / _update_geometry (which
 * gathers the per-triangle uvs from the CURRENT per-vertex uvs), rtk_accel_set_camera / _lights / _materials / _background, in any
 * order.  A refused call leaves the accel exactly as it was and usable.  None of the calls is stream-capturable.
 * Residency and ordering are those of rtk_accel_set_lights[_device]: on an accel that has never been on a device the host setters
 * only store, need no GPU and never return RTK_ERR_NO_DEVICE; on a resident accel they SYNCHRONISE THE DEVICE AT ENTRY, build into
 * spare buffers where something has to move, and swap at the end.  The _device variants put the accel on the device first (no
 * usable device -> RTK_ERR_NO_DEVICE), synchronise the device at entry, work on `hip_stream` and record the event later work on any
 * stream waits for; after entry they do not block the host, except to allocate when something outgrows its buffer (and, for the
 * uvs of an accel no update has touched yet, once to put the build-time vertex ids on the device).
 * The cost-feedback launch order and RTK_TRACE_AUTO's engine verdict are KEPT by all of them: a texture moves no silhouette and
 * forks no ray.
 * Errors, in this order: a NULL accel or required pointer, n < 0, a texture index outside the live table -> RTK_ERR_INVALID; what
 * the call validates (below), rtk_accel_set_texture_* on a texture that is not a bitmap -> RTK_ERR_INVALID; then (_device variants)
 * RTK_ERR_NO_DEVICE; RTK_ERR_HIP only from the runtime. */
typedef struct { int32_t kind; float color_a[3]; float color_b[3]; float param; int32_t width, height; } rtk_texture; /* 40 bytes */

/* *n = the number of textures; with `out`, the first min(cap, *n) of them.  A bitmap reads back with color_a, color_b and param
 * 0 and its size; every other kind with width = height = 0. */
int rtk_accel_get_textures(const rtk_accel *accel, rtk_texture *out /* may be NULL */, int32_t cap, int32_t *n);
/* *n_bytes = width * height * 3 of texture `texture` (0 for a texture that is not a bitmap); with `out`, the first
 * min(cap, *n_bytes) bytes, rows top-down.  After a device-side replacement they are fetched from the device, which synchronises it. */
int rtk_accel_get_texture_pixels(const rtk_accel *accel, int32_t texture, uint8_t *out /* may be NULL */, size_t cap, size_t *n_bytes);
/* Replaces the whole table; n is free: 0, fewer, or more than before, and an accel built without textures can gain them.
 * Validation is rtk_scene_create's: kind in [RTK_TEX_ALBEDO, RTK_TEX_BITMAP]; a bitmap needs width, height >= 1,
 * width * height <= 2^28 and a non-NULL pixels[i] (host [height][width][3]), and the texel bytes of all bitmaps together must fit
 * an int32 offset.  Colours and param are taken as they are (a zero square_size, a NaN or an infinity is the caller's business).
 * While a texture material of the live table refers to a texture >= n the call is refused: change the materials first.
 * rtk_accel_set_materials validates against the live count. */
int rtk_accel_set_textures(rtk_accel *accel, const rtk_texture *textures, int32_t n,
                           const uint8_t *const *pixels /* [n]; entry i read only for RTK_TEX_BITMAP; may be NULL when no texture is a bitmap */);
/* Replace the texels of ONE texture, which must be a bitmap; the size may differ from before.  On a resident accel every bitmap
 * has a slot in one texel buffer: a replacement that fits its slot is written in place and allocates nothing (the device was
 * synchronised at entry, so no launch enqueued earlier still reads it); one that outgrows it gets a new slot with head room at the
 * buffer's end, or, when the buffer is full, a larger buffer into which the other bitmaps are copied on the device. */
int rtk_accel_set_texture_pixels(rtk_accel *accel, int32_t texture, int32_t width, int32_t height, const uint8_t *rgb /* host [h][w][3] */);
int rtk_accel_set_texture_pixels_device(rtk_accel *accel, int32_t texture, int32_t width, int32_t height, const uint8_t *d_rgb, void *hip_stream);
/* Render to texture: the texels become what rtk_frame_to_rgb8_device makes of the width * height * 3 floats,
 * uint8(255.999 * clamp(x, 0, 1)) with the product in double (ppm.hpp:17-19), rows top-down as a frame's and stbi_load's are;
 * one kernel reads the floats and writes the bytes into the texture's slot.  With rtk_render_views_device this shows a view on a
 * quad of the next frame without leaving the device. */
int rtk_accel_set_texture_frame_device(rtk_accel *accel, int32_t texture, int32_t width, int32_t height,
                                       const float *d_rgb /* device [h][w][3], a finished frame */, void *hip_stream);
/* Dense per-vertex uvs in the layout of `vertices`: n_vertices rows, all meshes concatenated.  A mesh without uvs has zeros in
 * the reference (loader.hpp:199-207), so the equivalent scene is "every mesh has these uvs", and on a fresh accel the getter
 * returns the scene's uvs with zeros for such meshes.  Values are taken as they are.  On an accel without textures the setters
 * only store; the per-triangle uvs are made when textures appear (csrc/topology.hip, k_tri_uv). */
int rtk_accel_get_uvs(const rtk_accel *accel, float *uvs /* [n_vertices][2] */);
int rtk_accel_set_uvs(rtk_accel *accel, const float *uvs /* host [n_vertices][2] */);
int rtk_accel_set_uvs_device(rtk_accel *accel, const float *d_uvs /* device, 4-byte aligned */, void *hip_stream);

/* ---- image out: replaces write_ppm (io/image/ppm.hpp:7-25) ---- */
/* The quantisation of write_ppm on the device: out[i] = uint8(255.999 * clamp(rgb[i], 0, 1)) (ppm.hpp:17-19, the product in
 * double), n = number of floats.  A finished frame leaves the GPU as 3 bytes per pixel instead of 12. */
int rtk_frame_to_rgb8_device(const float *d_rgb, size_t n, uint8_t *d_out, void *hip_stream);
/* the P3 text of write_ppm from such bytes (same output as rtk_format_ppm on the floats) */
int rtk_format_ppm_rgb8(const uint8_t *rgb8, int32_t width, int32_t height, char *buf, size_t cap, size_t *n);
int rtk_write_ppm(const float *rgb, int32_t width, int32_t height, const char *path);
/* returns the byte count in *n; writes at most cap bytes into buf (buf may be NULL to query) */
int rtk_format_ppm(const float *rgb, int32_t width, int32_t height, char *buf, size_t cap, size_t *n);

#ifdef __cplusplus
}
#endif
#endif /* RTK_H */
