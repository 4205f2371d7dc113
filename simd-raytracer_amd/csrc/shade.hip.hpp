// The shading arithmetic of render/render.hpp, stated once for every engine: the megakernel (kernels.hip), the streaming
// pipeline (stream.hip), the caller-ray fallback (radiance.hip) and the batched occlusion query (occluded.hip).
// Result parity with the reference rests on these expressions keeping its operand order and parentheses (and on
// -ffp-contract=off): change one here and every engine changes with it.
#pragma once

#include "common.hip.hpp"

namespace rtk {
namespace dev {

constexpr float PI_F = 3.14159265358979323846f;

// ------------------------------------------------------------------------------------------------
// node staging: the whole traversal-ordered node array goes to LDS with coalesced 16-byte loads.
__device__ __forceinline__ void stage_nodes(const DevNode *g_nodes, uint32_t n_nodes, DevNode *lds_nodes) {
    const float4 *src = reinterpret_cast<const float4 *>(g_nodes);
    float4 *dst = reinterpret_cast<float4 *>(lds_nodes);
    for (uint32_t i = threadIdx.x; i < n_nodes * 2u; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// per-ray statistics of a wave (STATS kernels).  The rays themselves are counted by the callers, in sharded words.
__device__ __forceinline__ void flush_stats(const Stats &st, uint32_t rays, unsigned long long *counters) {
    const uint32_t r = wave_sum(rays), h = wave_sum(st.hits), nd = wave_sum(st.nodes), bp = wave_sum(st.boxpass),
                   lv = wave_sum(st.leaves), tr = wave_sum(st.tris), pk = wave_sum(st.packets16);
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(counters + kWordRays, (unsigned long long)r);
        atomicAdd(counters + kWordHits, (unsigned long long)h);
        atomicAdd(counters + kWordNodes, (unsigned long long)nd);
        atomicAdd(counters + kWordBoxpass, (unsigned long long)bp);
        atomicAdd(counters + kWordLeaves, (unsigned long long)lv);
        atomicAdd(counters + kWordTris, (unsigned long long)tr);
        atomicAdd(counters + kWordPackets16, (unsigned long long)pk);
    }
}

// ------------------------------------------------------------------------------------------------
// Which 8x8 pixel block is where (tile/bucket.hpp:7-21 buckets, 8x8 blocks inside, buckets dealt to ranks by rank_bucket).
// Everything in BlockMap is wave-uniform when `block` is.
struct BlockMap { uint32_t local_bucket, bucket, bx, by, sub_x0, sub_y0; };
__device__ __forceinline__ BlockMap block_map(const RenderArgs &A, const uint32_t block) {
    const uint32_t bpb = A.blocks_per_bucket_side * A.blocks_per_bucket_side;
    BlockMap B;
    B.local_bucket = block / bpb;
    const uint32_t sub = block % bpb;
    B.bucket = rank_bucket((uint32_t)A.rank, B.local_bucket, (uint32_t)A.world, A.skew_q);
    B.bx = (B.bucket % A.tiles_x) * A.bucket; B.by = (B.bucket / A.tiles_x) * A.bucket;
    B.sub_x0 = (sub % A.blocks_per_bucket_side) * 8u; B.sub_y0 = (sub / A.blocks_per_bucket_side) * 8u;
    return B;
}
// lane `lane`'s pixel of that block: inside its bucket (lx, ly) and in the frame (px, py); pixel_valid: whether it exists
struct Pixel { uint32_t lx, ly, px, py; };
__device__ __forceinline__ Pixel block_pixel(const BlockMap &B, const uint32_t lane) {
    Pixel p;
    p.lx = B.sub_x0 + (lane & 7u); p.ly = B.sub_y0 + (lane >> 3);
    p.px = B.bx + p.lx; p.py = B.by + p.ly;
    return p;
}
__device__ __forceinline__ bool pixel_valid(const RenderArgs &A, const BlockMap &B, const Pixel &p) {
    return (B.bucket < A.n_buckets) & (p.lx < A.bucket) & (p.ly < A.bucket) & (p.px < A.width) & (p.py < A.height);
}

// ------------------------------------------------------------------------------------------------
// One light of the light loop (render.hpp:184-206, texture material :213-236) seen from P with the cosine law's normal
// `ncos`: the unit direction to the light, its distance and contrib = (intensity / area) * max(0, cosine).  The callers
// act on is_occluded's loop guard, 0.0f < radius (:114), each in their own way.
struct LightTerm { V3 dir; float radius, contrib; };
__device__ __forceinline__ LightTerm light_term(const DevLight *L, const V3 P, const V3 ncos) {
    V3 ld = mk(L->pos[0], L->pos[1], L->pos[2]) - P;
    const float radius = length(ld);
    const float area = 4.0f * PI_F * radius * radius;
    ld = normalized(ld);
    const float d0 = dot(ld, ncos);
    const float cosine = (0.0f < d0) ? d0 : 0.0f;                // std::max(0, dot)
    return LightTerm{ld, radius, (L->intensity / area) * cosine};
}

// One round of is_occluded's loop (render.hpp:110-131) once the closest hit `c` of the ray (o, d) is known: nothing nearer
// than max_t is "clear" (:117); a transmissive surface is stepped through (:126-127: the origin and max_t move on) and the
// query is asked again while 0 < max_t; anything else occludes.  `has_refractive` == 0: nothing in the scene is transmissive.
// (Values in, values out: through references the callers' loop variables change places in the register allocation.)
enum : int { OCC_CLEAR = 0, OCC_OCCLUDED = 1, OCC_AGAIN = 2 };
struct OccStep { int answer; V3 o; float max_t; };
__device__ __forceinline__ OccStep occlusion_step(const TreeView &T, const DevMaterial *materials, const float shadow_bias,
                                                  const int has_refractive, const Cand &c, const V3 o, const V3 d, const float max_t) {
    OccStep r = {OCC_OCCLUDED, o, max_t};
    if ((c.k == kMiss) | (max_t < c.t)) r.answer = OCC_CLEAR;
    else if (has_refractive) {
        const uint32_t m = T.shade[T.tri_ids[c.k]].material;
        if (materials[m].kind == RTK_MAT_REFRACTIVE) {
            const V3 hp = o + (c.t * d);
            r.o = hp + (shadow_bias * d);
            r.max_t -= c.t;
            r.answer = (0.0f < r.max_t) ? OCC_AGAIN : OCC_CLEAR;
        }
    }
    return r;
}

// ------------------------------------------------------------------------------------------------
// Secondary rays as (origin, direction); what becomes of them (a Ray with or without its inverse direction, a queue
// record) is the engine's business.
struct RayOD { V3 o, d; };

// reflection off the normal n (render.hpp:239-250; :268-271 with the refraction's i and n)
__device__ __forceinline__ RayOD reflect_at(const V3 P, const V3 n, const V3 d, const float reflection_bias) {
    RayOD r;
    r.d = d - ((2.0f * dot(d, n)) * n);
    r.o = P + (reflection_bias * r.d);
    return r;
}

// Refractive material (render.hpp:252-301), `n_shade` = the hit normal or the face normal by the material's smooth_shading.
// The reflection ray always exists; under total internal reflection (`tir`) it is the only one, otherwise the refraction
// ray and the Fresnel factor (x^5 in double, :300) are there too.
struct Refraction { bool tir; RayOD refl, refr; float fresnel; };
__device__ __forceinline__ Refraction refract_at(const RenderArgs &A, const DevMaterial *mat, const V3 P, const V3 n_shade, const V3 din) {
    V3 n = normalized(n_shade);
    const V3 i = normalized(din);
    float eta_i = 1.0f, eta_r = mat->ior;
    if (0.0f < dot(i, n)) { const float tmp = eta_i; eta_i = eta_r; eta_r = tmp; n = neg(n); }
    const float cos_i_n = -dot(i, n);
    const float sin_i_n = __builtin_sqrtf(1.0f - cos_i_n * cos_i_n);
    Refraction r;
    r.refl = reflect_at(P, n, i, A.reflection_bias);
    r.tir = eta_r / eta_i < sin_i_n;
    if (r.tir) return r;                                          // (refr and fresnel are not set, and not read)
    const float sin_r = ((sin_i_n * eta_i) / eta_r);
    const float cos_r = __builtin_sqrtf(1.0f - sin_r * sin_r);
    r.refr.d = (cos_r * neg(n)) + (sin_r * normalized(i + (cos_i_n * n)));
    r.refr.o = P + (A.refraction_bias * r.refr.d);
    const double x = (double)(1.0f + dot(i, n));
    r.fresnel = (float)(0.5 * (x * x * x * x * x));
    return r;
}

// GI ray `it` of the diffuse hit at P with hit normal hn, reached along d (render.hpp:151-176); `key` is the RNG key of the
// ray that hit (draws 2 + 2 it and 3 + 2 it, common.hip.hpp).
__device__ __forceinline__ RayOD gi_ray(const V3 P, const V3 hn, const V3 d, const uint32_t key, const uint32_t it,
                                        const float reflection_bias) {
    const V3 right = normalized(cross(d, hn));
    const V3 up = hn;
    const V3 fwd = cross(right, up);
    float s1, c1, s2, c2;
    det_sincos(PI_F * urand_key(key, 2u + 2u * it), s1, c1);
    V3 rv = mk(c1, s1, 0.0f);
    det_sincos(PI_F * urand_key(key, 3u + 2u * it) * 2.0f, s2, c2);
    rv = mk(c2 * rv.x + 0.0f * rv.y + (-s2) * rv.z, 0.0f * rv.x + 1.0f * rv.y + 0.0f * rv.z,
            s2 * rv.x + 0.0f * rv.y + c2 * rv.z);
    RayOD r;
    r.o = P + (reflection_bias * hn);
    r.d = mk(right.x * rv.x + right.y * rv.y + right.z * rv.z, up.x * rv.x + up.y * rv.y + up.z * rv.z,
             fwd.x * rv.x + fwd.y * rv.y + fwd.z * rv.z);
    return r;
}

}  // namespace dev
}  // namespace rtk
