"""rtk_render_gbuffer_specular's contract (include/rtk.h) in numpy float32 (tests/test_specular_model.py,
tests/test_gpu_gbuffer_specular.py).  A helper, not a test.

Every segment of a chain is answered by the CPU oracle's Accel.intersect / intersect_rest (first segment with back-face culling,
the others without); the reflection (render/render.hpp:240-242), the refraction (:252-292: cos_r, r, normalized, with the NaN
directions iors of 0 and below produce) and the fold of the mirror normals are written out here in the reference's operand
order, one float32 operation at a time.  Nothing here looks at what the code under test computes."""
import numpy as np

from occlusion_model import dot3, normalized3

MISS = 0xFFFFFFFF
DIFFUSE, REFLECTIVE, REFRACTIVE, CONSTANT, TEXTURE = range(5)
PLANES = ("depth", "position", "normal", "surface_position", "surface_normal", "albedo", "bary", "tri", "mesh", "material", "bounces",
          "last_ray")
COMPS = dict(depth=1, position=3, normal=3, surface_position=3, surface_normal=3, albedo=3, bary=2, tri=1, mesh=1, material=1, bounces=1,
             last_ray=6)
FLOAT_PLANES = ("depth", "position", "normal", "surface_position", "surface_normal", "albedo", "bary", "last_ray")
SHARED = ("depth", "position", "normal", "albedo", "bary", "tri", "mesh", "material")       # the planes rtk_render_gbuffer has too

F = np.float32


def _scale(s, v):
    """s * v (vec3.hpp:94-97), s [n], v [n, 3]"""
    return (s[:, None] * v).astype(F)


def reflect(P, n, d, bias):
    """render.hpp:240-242: d - ((2 * dot(d, n)) * n), then P + (bias * direction)"""
    rd = (d - _scale(F(2.0) * dot3(d, n), n)).astype(F)
    return (P + (F(bias) * rd).astype(F)).astype(F), rd


def refract(P, n_shade, d, ior, reflection_bias, refraction_bias):
    """render.hpp:252-292 -> (tir bool[n], reflection (o, d), refraction (o, d)); the refraction's rows are meaningless under tir"""
    with np.errstate(all="ignore"):
        n = normalized3(n_shade).astype(F)
        i = normalized3(d).astype(F)
        leaving = F(0.0) < dot3(i, n)
        eta_i = np.where(leaving, ior, F(1.0)).astype(F)
        eta_r = np.where(leaving, F(1.0), ior).astype(F)
        n = np.where(leaving[:, None], -n, n).astype(F)
        cos_i = (-dot3(i, n)).astype(F)
        sin_i = np.sqrt(F(1.0) - cos_i * cos_i, dtype=F)
        refl = reflect(P, n, i, reflection_bias)
        tir = eta_r / eta_i < sin_i
        sin_r = ((sin_i * eta_i) / eta_r).astype(F)
        cos_r = np.sqrt(F(1.0) - sin_r * sin_r, dtype=F)
        r = normalized3((i + _scale(cos_i, n)).astype(F)).astype(F)
        rd = (_scale(cos_r, -n) + _scale(sin_r, r)).astype(F)
        ro = (P + (F(refraction_bias) * rd).astype(F)).astype(F)
    return tir, refl, (ro, rd)


def fold(M, m):
    """w_i = (M_i0 m.x + M_i1 m.y) + M_i2 m.z;  M_ij = M_ij - ((2 w_i) m_j)"""
    with np.errstate(all="ignore"):
        w = ((M[:, :, 0] * m[:, None, 0] + M[:, :, 1] * m[:, None, 1]) + M[:, :, 2] * m[:, None, 2]).astype(F)
        return (M - ((F(2.0) * w)[:, :, None] * m[:, None, :]).astype(F)).astype(F)


def apply(M, n):
    with np.errstate(all="ignore"):
        return ((M[:, :, 0] * n[:, None, 0] + M[:, :, 1] * n[:, None, 1]) + M[:, :, 2] * n[:, None, 2]).astype(F)


def specular_planes(oacc, flat, rays, max_depth, reflection_bias=1e-4, refraction_bias=1e-4):
    """The twelve planes of the camera rays `rays` [n, 6] of ONE view, flattened ([n] or [n, c]), and beside them what the tests
    select pixels by: "surface" bool[n], "reflections", "refractions", "tirs" (bounces of each kind, uint32 [n]) and "end_kind"
    (material kind of the end hit, -1 without a surface) and "chain_mesh" (uint32 [n, max_depth + 1]: the mesh every segment of
    the chain hit, MISS where there was none).  `flat` gives the materials, `oacc` (the oracle's accel of it) the hits."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n = len(rays)
    o, d = rays[:, 0:3].copy(), rays[:, 3:6].copy()
    L = np.zeros(n, F)
    M = np.tile(np.eye(3, dtype=F), (n, 1, 1))
    k = np.zeros(n, np.uint32)
    mirrored = np.zeros(n, bool)
    live = np.ones(n, bool)
    surface = np.zeros(n, bool)
    counts = {name: np.zeros(n, np.uint32) for name in ("reflections", "refractions", "tirs")}
    end = {"t": np.zeros(n, F), "u": np.zeros(n, F), "v": np.zeros(n, F), "tri": np.full(n, MISS, np.uint32),
           "mesh": np.full(n, MISS, np.uint32), "normal": np.zeros((n, 3), F)}
    chain = np.full((n, max_depth + 1), MISS, np.uint32)
    for bounce in range(max_depth + 1):
        idx = np.flatnonzero(live)
        if len(idx) == 0:
            break
        seg = np.ascontiguousarray(np.concatenate([o[idx], d[idx]], axis=1), F)
        hits, rest = oacc.intersect(seg, bounce == 0), oacc.intersect_rest(seg, bounce == 0)
        hit = hits["mesh"] != MISS
        assert np.array_equal(hit, hits["tri"] != MISS)
        chain[idx, bounce] = hits["mesh"]
        mat = flat.mesh_material[np.where(hit, hits["mesh"], 0)]
        kind = np.where(hit, flat.mat_kind[mat], -1)
        at_limit = bounce == max_depth                       # every live lane has k == bounce
        live[idx[~hit]] = False                              # a miss: NO SURFACE
        if at_limit:
            live[idx] = False                                # color_hit returns the background: NO SURFACE
            break
        t = hits["t"].astype(F)
        L[idx[hit]] = (L[idx] + t)[hit]
        P = (seg[:, 0:3] + _scale(t, seg[:, 3:6])).astype(F)
        hn = np.ascontiguousarray(hits["normal"], F)
        # the surface that is shaded
        ends = hit & (kind != REFLECTIVE) & (kind != REFRACTIVE)
        e = idx[ends]
        surface[e] = True
        live[e] = False
        for name in ("t", "u", "v", "tri", "mesh", "normal"):
            end[name][e] = hits[name][ends]
        # mirrors
        sel = hit & (kind == REFLECTIVE)
        if sel.any():
            j = idx[sel]
            with np.errstate(all="ignore"):
                o[j], d[j] = reflect(P[sel], hn[sel], seg[sel, 3:6], reflection_bias)
            M[j] = fold(M[j], hn[sel])
            mirrored[j] = True
            counts["reflections"][j] += 1
        # glass
        sel = hit & (kind == REFRACTIVE)
        if sel.any():
            j = idx[sel]
            n_shade = np.where((flat.mat_smooth[mat[sel]] != 0)[:, None], hn[sel], rest["face_normal"][sel]).astype(F)
            tir, refl, refr = refract(P[sel], n_shade, seg[sel, 3:6], flat.mat_ior[mat[sel]].astype(F), reflection_bias, refraction_bias)
            o[j] = np.where(tir[:, None], refl[0], refr[0])
            d[j] = np.where(tir[:, None], refl[1], refr[1])
            with np.errstate(all="ignore"):
                folded = fold(M[j], normalized3(n_shade).astype(F))
            M[j] = np.where(tir[:, None, None], folded, M[j])
            mirrored[j] |= tir
            counts["tirs"][j] += tir.astype(np.uint32)
            counts["refractions"][j] += (~tir).astype(np.uint32)
        k[idx[hit & ~ends]] += 1
    s = surface
    out = {"bounces": k, "last_ray": np.concatenate([o, d], axis=1).astype(F), "surface": s}
    out["depth"] = np.where(s, L, F(-1.0)).astype(F)
    with np.errstate(all="ignore"):
        vpos = (rays[:, 0:3] + _scale(L, rays[:, 3:6])).astype(F)
        spos = (o + _scale(end["t"], d)).astype(F)
        vn = np.where(mirrored[:, None], apply(M, end["normal"]), end["normal"]).astype(F)
    zero3 = np.zeros((n, 3), F)
    out["position"] = np.where(s[:, None], vpos, zero3)
    out["normal"] = np.where(s[:, None], vn, zero3)
    out["surface_position"] = np.where(s[:, None], spos, zero3)
    out["surface_normal"] = np.where(s[:, None], end["normal"], zero3)
    out["bary"] = np.where(s[:, None], np.stack([end["u"], end["v"]], axis=1), F(0.0)).astype(F)
    out["tri"], out["mesh"] = end["tri"], end["mesh"]
    material = np.where(s, flat.mesh_material[np.where(s, end["mesh"], 0)].astype(np.uint32), np.uint32(MISS)).astype(np.uint32)
    out["material"] = material
    # the end hit's albedo: the oracle's own sample(texture, hit, uvs) or material albedo of the last ray's first hit
    alb = np.tile(np.asarray(flat.background, F), (n, 1))
    for cull in (True, False):
        sel = s & ((k == 0) == cull)
        if sel.any():
            alb[sel] = oacc.first_hit_albedo(np.ascontiguousarray(out["last_ray"][sel]), cull)
    out["albedo"] = alb
    out["end_kind"] = np.where(s, flat.mat_kind[np.where(s, material, 0)], -1)
    out["chain_mesh"] = chain
    out.update(counts)
    return out


def camera_planes(oacc, flat, w, h, max_depth, spp=1, sample=0, **kw):
    """specular_planes of the oracle's own camera rays of `sample`"""
    rays = oacc.camera_rays(w, h, spp=spp, sample=sample).reshape(-1, 6)
    out = specular_planes(oacc, flat, rays, max_depth, **kw)
    out["camera_rays"] = rays
    return out


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """bit-equal; a NaN only has to meet a NaN (as everywhere in this suite)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(u32(np.where(na, F(0), a)), u32(np.where(nb, F(0), b)))
