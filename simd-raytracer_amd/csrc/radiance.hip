// HIP kernels for gfx950 behind rtk_accel_radiance (color_hit for caller-supplied rays, render/render.hpp:133-308).
//
// The batch's fast path is the streaming pipeline (stream.hip) with the caller's rays as its level 0.  A frame whose
// queues overflow is redone by the megakernel; caller rays have no megakernel, so this file holds their safety net:
// k_radiance_fallback evaluates the whole recursion for one ray per lane with an explicit stack.  It runs behind every
// chunk and does nothing unless the chunk's overflow word is set.  It is the slow path: its stack lives in scratch, its
// traces are the per-lane walk, and nothing but exactness is asked of it.
#include <hip/hip_runtime.h>

#include "shade.hip.hpp"
#include "stream.hpp"

namespace rtk {
namespace dev {

namespace {

// One color_hit invocation that waits for a child ray or a light: what the recursion keeps in its C++ stack frame.
struct RadFrame {
    uint32_t kind;          // NODE_PASS / NODE_REFR / NODE_DIFF / NODE_TEX (stream.hpp)
    uint32_t step;          // NODE_REFR: children returned; NODE_DIFF: GI rays spawned
    uint32_t light;         // NODE_DIFF / NODE_TEX: the light whose query is pending or next
    uint32_t key;           // RNG key of the ray that hit
    float contrib;          // (intensity / area) * cosine of the pending light
    float fresnel;
    V3 acc;                 // final_color so far; NODE_REFR: the refraction child's colour
    V3 albedo;              // the material's, or the sampled texture colour
    V3 P, hn, ncos, d;      // hit position, hit normal, the cosine law's normal, direction of the ray that hit
    V3 c1o, c1d;            // NODE_REFR: the reflection ray, traced second
};

}  // namespace

__global__ __launch_bounds__(256) void k_radiance_fold(const unsigned long long *lane_counters, unsigned long long *total,
                                                        const uint32_t *overflow) {
    if (threadIdx.x != 0u) return;
    if (*overflow != 0u) { atomicAdd(total + kRadianceRedone, 1ull); return; }   // the fallback counts the chunk from scratch
    unsigned long long rays = lane_counters[kWordRays];
    for (int i = 0; i < kRayCounterShards; ++i) rays += lane_counters[kRayShardWord + i];
    atomicAdd(total + kRadianceRays, rays);
}

template <bool LDS_NODES>
__global__ __launch_bounds__(256) void k_radiance_fallback(StreamArgs S, unsigned long long *total) {
    if (S.ws.ctrl[kCtrlOverflow] == 0u) return;                              // (wave-uniform: before any barrier)
    const RenderArgs &A = S.r;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevNode *lds_nodes = reinterpret_cast<DevNode *>(smem);
    if (LDS_NODES) stage_nodes(A.tree.nodes, A.tree.n_nodes, lds_nodes);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = i < S.user_n;
    const V3 background = mk(A.background[0], A.background[1], A.background[2]);
    const V3 black = mk(0.f, 0.f, 0.f);
    const uint32_t n_lights = (uint32_t)A.n_lights;

    RadFrame stack[kMaxRayDepth + 1];
    uint32_t sp = 0u;                                                        // frames on the stack = depth of the ray in flight
    enum : uint32_t { ST_TRACE = 0, ST_SHADOW = 1, ST_DONE = 2 };
    uint32_t state = have ? ST_TRACE : ST_DONE;
    Ray ray = make_ray(mk(0.f, 0.f, 0.f), mk(1.f, 1.f, 1.f));
    uint32_t key = 0u;
    bool cull = false, miss_bg = true;
    float max_t = 0.0f;
    V3 result = black;
    uint32_t nrays = 0u;
    if (have) {
        const float *p = reinterpret_cast<const float *>(S.user_rays + i);
        ray = make_ray(mk(p[0], p[1], p[2]), mk(p[3], p[4], p[5]));
        const uint32_t id = S.user_ids != nullptr ? S.user_ids[i] : S.user_id0 + i;
        key = root_key(pcg_hash(A.seed), id, S.user_sample);
        cull = S.user_cull != 0u;
    }
    Stats st = {0, 0, 0, 0, 0, 0};
    SliceCtx sx = {nullptr, 0u, 0u, true, 0u, nullptr};

    while (wave_any(state != ST_DONE)) {
        const bool want = state != ST_DONE;
        // occlusion queries may stop at the first answering hit when nothing is transmissive (RenderArgs::shadow_exit)
        const float exit_t = (state == ST_SHADOW && A.shadow_exit != 0) ? max_t : -1.0f;
        const Cand c = trace<RTK_TRACE_LANE, false, LDS_NODES>(A.tree, lds_nodes, ray, cull, want, st, sx, kAutoMinLanes, exit_t);
        if (!want) continue;
        nrays += 1u;
        // what the trace means for this lane: a value to hand to the caller (`ret`), a new frame, or the next shadow step
        bool returning = false, advance = false;
        V3 ret = black;
        if (state == ST_SHADOW) {
            RadFrame &f = stack[sp - 1u];
            const OccStep os = occlusion_step(A.tree, A.materials, A.shadow_bias, A.has_refractive, c, ray.o, ray.d, max_t);
            ray.o = os.o; max_t = os.max_t;
            if (os.answer != OCC_AGAIN) {
                if (os.answer == OCC_CLEAR) f.acc = f.acc + (f.contrib * f.albedo);
                f.light += 1u;
                advance = true;
            }
        } else {                                                             // color_hit's material switch, :133-308
            cull = false;                                                    // only the batch's own rays cull
            const uint32_t depth = sp;
            if (c.k == kMiss) { ret = miss_bg ? background : black; returning = true; }
            else if ((int)depth == A.max_depth) { ret = background; returning = true; }        // :138-139
            else {
                const Surface s = reconstruct(A.tree, c);
                const V3 P = ray.o + (c.t * ray.d);
                const V3 hn = s.hit_normal;
                const DevMaterial *m = A.materials + s.material;
                const int mkind = m->kind;
                RadFrame &f = stack[sp];
                f.key = key; f.step = 0u; f.light = 0u; f.acc = black; f.P = P; f.hn = hn; f.d = ray.d;
                f.contrib = 0.0f; f.fresnel = 0.0f; f.c1o = black; f.c1d = black; f.ncos = black; f.albedo = black;
                if (mkind == RTK_MAT_CONSTANT) { ret = mk(m->albedo[0], m->albedo[1], m->albedo[2]); returning = true; }
                else if (mkind == RTK_MAT_REFLECTIVE) {
                    const RayOD refl = reflect_at(P, hn, ray.d, A.reflection_bias);
                    f.kind = NODE_PASS; sp += 1u;
                    ray = make_ray(refl.o, refl.d); key = child_key(f.key, 0u); miss_bg = true;
                } else if (mkind == RTK_MAT_REFRACTIVE) {
                    const Refraction rf = refract_at(A, m, P, m->smooth ? hn : s.face_normal, ray.d);
                    if (rf.tir) {
                        f.kind = NODE_PASS; sp += 1u;
                        ray = make_ray(rf.refl.o, rf.refl.d); key = child_key(f.key, 0u); miss_bg = false;
                    } else {
                        f.fresnel = rf.fresnel;
                        f.c1o = rf.refl.o; f.c1d = rf.refl.d;
                        f.kind = NODE_REFR; sp += 1u;
                        ray = make_ray(rf.refr.o, rf.refr.d); key = child_key(f.key, 0u); miss_bg = false;
                    }
                } else if (mkind == RTK_MAT_TEXTURE) {                                          // :211-238
                    f.ncos = m->smooth ? hn : s.face_normal;
                    f.albedo = sample_texture(A.textures + m->texture, A.tri_uv + s.tri, c.u, c.v, A.tex_pixels);
                    f.kind = NODE_TEX; sp += 1u; advance = true;
                } else {                                                                        // diffuse, :148-209
                    f.ncos = m->smooth ? hn : s.face_normal;
                    f.albedo = mk(m->albedo[0], m->albedo[1], m->albedo[2]);
                    f.kind = NODE_DIFF; sp += 1u; advance = true;
                }
            }
        }
        // run the recursion on until the lane needs a trace again (or is done): no wave-wide operation in here
        while (returning || advance) {
            if (returning) {
                returning = false;
                if (sp == 0u) { result = ret; state = ST_DONE; break; }
                RadFrame &f = stack[sp - 1u];
                if (f.kind == NODE_PASS) { sp -= 1u; returning = true; }                        // :249 / :275
                else if (f.kind == NODE_REFR) {
                    if (f.step == 0u) {                                                         // refraction back: now the reflection
                        f.acc = ret; f.step = 1u;
                        ray = make_ray(f.c1o, f.c1d); key = child_key(f.key, 1u); miss_bg = false; state = ST_TRACE;
                    } else {                                                                    // :301
                        ret = (f.fresnel * ret) + ((1.0f - f.fresnel) * f.acc);
                        sp -= 1u; returning = true;
                    }
                } else { f.acc = f.acc + ret; advance = true; }                                 // a GI child, :176
                continue;
            }
            advance = false;
            RadFrame &f = stack[sp - 1u];
            if (f.kind == NODE_DIFF && f.step < (uint32_t)A.diffuse_rays) {                     // GI rays
                const uint32_t gi = f.step;
                f.step += 1u;
                const RayOD g = gi_ray(f.P, f.hn, f.d, f.key, gi, A.reflection_bias);
                ray = make_ray(g.o, g.d); key = child_key(f.key, gi); miss_bg = false; state = ST_TRACE;
                break;
            }
            bool shadow = false;
            while (f.light < n_lights) {                                                        // light loop
                const LightTerm lt = light_term(A.lights + f.light, f.P, f.ncos);
                const float contrib = lt.contrib;
                bool traced = 0.0f < lt.radius;                                                   // is_occluded's loop guard, :114
                if (traced && A.skip_unlit != 0 && unlit_query(contrib, albedo_reach(f.albedo))) { traced = false; nrays += 1u; }
                if (traced) {
                    f.contrib = contrib;
                    ray = make_ray(f.P + (A.shadow_bias * lt.dir), lt.dir); max_t = lt.radius; state = ST_SHADOW; shadow = true;
                    break;
                }
                f.acc = f.acc + (contrib * f.albedo);                                           // not occluded
                f.light += 1u;
            }
            if (shadow) break;
            if (f.kind == NODE_DIFF) {                                                          // :208
                const float div = (float)(A.diffuse_rays + 1);
                ret = mk(f.acc.x / div, f.acc.y / div, f.acc.z / div);
            } else ret = f.acc;
            sp -= 1u; returning = true;
        }
    }
    if (have) {                                                              // color{} += c, / 1 sample (render.hpp:33,66-72; k_combine)
        float *o = A.out + (size_t)i * 3;
        o[0] = 0.0f + result.x; o[1] = 0.0f + result.y; o[2] = 0.0f + result.z;
    }
    const uint32_t sum = wave_sum(nrays);
    if ((threadIdx.x & 63u) == 0u && sum != 0u) atomicAdd(total + kRadianceRays, (unsigned long long)sum);
}

}  // namespace dev

hipError_t launch_radiance_fold(const dev::StreamArgs &S, unsigned long long *total, hipStream_t s) {
    hipLaunchKernelGGL(dev::k_radiance_fold, dim3(1), dim3(64), 0, s, S.r.counters, total, S.ws.ctrl + dev::kCtrlOverflow);
    return hipGetLastError();
}

hipError_t launch_radiance_fallback(const dev::StreamArgs &S, unsigned long long *total, hipStream_t s) {
    const unsigned blocks = (S.user_n + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    const size_t lds_bytes = (size_t)S.r.tree.n_nodes * sizeof(DevNode);
    if (lds_bytes <= kMaxNodeLdsBytes) hipLaunchKernelGGL((dev::k_radiance_fallback<true>), dim3(blocks), dim3(256), lds_bytes, s, S, total);
    else hipLaunchKernelGGL((dev::k_radiance_fallback<false>), dim3(blocks), dim3(256), 0, s, S, total);
    return hipGetLastError();
}

}  // namespace rtk
