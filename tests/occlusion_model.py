"""is_occluded(accel, ray, max_t) (render/render.hpp:110-131) in numpy float32 over the oracle's closest hit.

A helper, not a test.  tests/test_occlusion_model.py pins it to the oracle's own renders; the GPU tests compare
rtk_accel_occluded with it byte for byte."""
import numpy as np

MISS = 0xFFFFFFFF
CLEAR, OCCLUDED, STEP_LIMIT = 0, 1, 2
REFRACTIVE = 2


def occluded_ref(oacc, flat, rays, max_t, shadow_bias, max_steps=1024, with_entered=False):
    """-> (answer uint8[n], steps int32[n]) [, entered bool[n]].

    steps[i] = times query i stepped through a transmissive surface (for a query that made `max_steps` closest-hit queries
    and would make another: max_steps, answer STEP_LIMIT); entered[i] = the query's last closest-hit query ended it by an
    answer (miss, beyond max_t, or an opaque hit) rather than by the loop guard or the limit.  The loop made
    (steps + entered).sum() calls of intersect."""
    rays = np.array(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    max_t = np.array(max_t, np.float32).reshape(-1).copy()
    bias = np.float32(shadow_bias)
    answer = np.zeros(n, np.uint8)
    steps = np.zeros(n, np.int32)
    entered = np.zeros(n, bool)
    refractive = np.asarray(flat.mat_kind)[np.asarray(flat.mesh_material)] == REFRACTIVE
    with np.errstate(all="ignore"):
        idx = np.flatnonzero(np.float32(0.0) < max_t)                           # the loop guard, :115 (false for NaN)
        while idx.size:
            h = oacc.intersect(np.concatenate([o[idx], d[idx]], axis=1), cull=False)
            miss = h["mesh"] == MISS
            t = h["t"]
            clear = miss | (max_t[idx] < t)                                     # :117
            through = ~clear & refractive[np.where(miss, 0, h["mesh"])]         # :121-124
            done = idx[~through]
            answer[done] = np.where(clear[~through], CLEAR, OCCLUDED)
            entered[done] = True
            s = idx[through]
            ts = t[through]
            pos = o[s] + ts[:, None] * d[s]                                     # hit<F>::position, kd_tree_simd.hpp:254
            o[s] = pos + bias * d[s]                                            # :126
            max_t[s] = max_t[s] - ts                                            # :127
            steps[s] += 1
            again = np.float32(0.0) < max_t[s]
            limit = again & (steps[s] >= max_steps)
            answer[s[limit]] = STEP_LIMIT
            idx = s[again & ~limit]
    return (answer, steps, entered) if with_entered else (answer, steps)


def segments(flat, n, seed):
    """n occlusion queries between uniform points of the scene's box inflated by 1: the first half with unit directions and
    max_t = length, the second half with the raw difference as direction and max_t = 1; every fourth max_t scaled by a
    factor from U(0.25, 2).  -> (rays float32[n,6], max_t float32[n])"""
    rng = np.random.default_rng(seed)
    v = np.asarray(flat.vertices, np.float32)
    lo, hi = v.min(axis=0) - np.float32(1.0), v.max(axis=0) + np.float32(1.0)
    a = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    b = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = b - a
    length = np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)
    max_t = np.ones(n, np.float32)
    half = n // 2
    d[:half] = d[:half] / length[:half, None]
    max_t[:half] = length[:half]
    scale = rng.uniform(0.25, 2.0, n).astype(np.float32)
    max_t[::4] = max_t[::4] * scale[::4]
    return np.ascontiguousarray(np.concatenate([a, d], axis=1), np.float32), max_t


def length3(v):
    """vec3::len (core/math/vec3.hpp:85-91): sqrt(x*x + y*y + z*z), summed left to right in float."""
    v = np.asarray(v, np.float32)
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=np.float32)


def normalized3(v):
    """normalized (vec3.hpp:104-108): every component times 1 / len."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / length3(v)
    return v * inv[:, None]


def dot3(a, b):
    """dot (vec3.hpp:119-122): (ax*bx + ay*by) + az*bz."""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def shadow_queries(flat, P, light, shadow_bias=1e-4):
    """The shadow ray of every point of P [m,3] towards light `light` as the light loop builds it (render/render.hpp:184-200).
    -> (rays float32[m,6], radius float32[m], light_direction float32[m,3])"""
    P = np.asarray(P, np.float32)
    ld = np.asarray(flat.light_pos, np.float32)[light][None, :] - P
    radius = length3(ld)
    ld = normalized3(ld)
    origin = P + np.float32(shadow_bias) * ld
    return np.ascontiguousarray(np.concatenate([origin, ld], axis=1), np.float32), radius, ld


def camera_hits(oacc, width, height):
    """Camera rays of a width x height frame (sample 0) and their closest hits with back-face culling (render.hpp:62-64).
    -> (rays [h*w,6], hits HIT_DTYPE[h*w], P float32[h*w,3] = origin + t * direction)"""
    rays = oacc.camera_rays(width, height).reshape(-1, 6)
    hits = oacc.intersect(rays, cull=True)
    with np.errstate(all="ignore"):
        P = rays[:, :3] + hits["t"][:, None] * rays[:, 3:]
    return rays, hits, P
