"""The numpy float32 model of rtk_temporal_accumulate (include/rtk.h spells the arithmetic out) and the seeded synthetic pair of
frames that the temporal tests share.  Whole-array expressions, the four taps in the stated order (j outer, i inner), every
operation in float32 in the order the contract writes it: numpy does not contract a multiply and an add, so the bits are those of
the scalar C++ of csrc/temporal_math.hpp built with -ffp-contract=off, and of the kernel."""
import ctypes

import numpy as np

import ref_camera

F = np.float32
MISS_MESH = np.uint32(0xFFFFFFFF)
FOV = 60.0
# the parameters the issue's figures were measured with
PARAMS = dict(fov_degrees=FOV, alpha_min=0.05, plane_tolerance=0.01, normal_min_dot=0.9, max_history=32)
SIZES = ((37, 19), (5, 3), (1, 1), (70, 36))                  # width x height
COMBOS = ("noise+mesh", "noise", "mesh", "neither")           # which optional families a case hands in


def scalars(width, height, fov_degrees):
    """(aspect, th, wf, hf) as the host computes them: ref_camera's expressions (render.hpp:26, :55-57)"""
    aspect = F(width) / F(height)
    fov_radians = F(np.float64(fov_degrees) * (np.float64(np.pi) / np.float64(180.0)))
    th = F(ref_camera._libm.tanf(ctypes.c_float(float(fov_radians / F(2.0)))))
    return aspect, th, F(width), F(height)


def project(position, view, width, height, fov_degrees):
    """Step 2 for every pixel -> (ok, fx, fy): ok = cz < 0 and the range test hold; fx, fy are what the contract computes (garbage
    where ok is false)."""
    aspect, th, wf, hf = scalars(width, height, fov_degrees)
    C = np.asarray(view[0], F).reshape(3)
    M = np.asarray(view[1], F).reshape(9)
    P = np.asarray(position, F)
    with np.errstate(all="ignore"):
        D = [P[..., k] - C[k] for k in range(3)]
        cx = (M[0] * D[0] + M[1] * D[1]) + M[2] * D[2]
        cy = (M[3] * D[0] + M[4] * D[1]) + M[5] * D[2]
        cz = (M[6] * D[0] + M[7] * D[1]) + M[8] * D[2]
        front = cz < F(0.0)
        iz = -cz
        qx, qy = cx / iz, cy / iz
        ux, uy = (qx / th) / aspect, qy / th
        fx = ((ux + F(1.0)) * F(0.5)) * wf - F(0.5)
        fy = ((F(1.0) - uy) * F(0.5)) * hf - F(0.5)
        ok = front & (fx > F(-1.0)) & (fx < wf) & (fy > F(-1.0)) & (fy < hf)
    return ok, fx.astype(F), fy.astype(F)


def accumulate(cur, prev, *, fov_degrees, alpha_min, plane_tolerance, normal_min_dot, max_history, noise=True, mesh=True, detail=False):
    """cur: dict rgb, noise, position, normal, depth, mesh; prev: None or dict rgb, noise, length, position, normal, depth, mesh and
    view = (position[3], matrix[9]).  noise / mesh: whether those families are handed in.  -> dict rgb, noise (None without the
    family), length; with detail also accepted [h, w] (taps accepted per pixel), rejected [h, w] (taps inside the image that a
    test threw out), projected and blended [h, w] bool, used [h, w] bool (the history's pixels that some tap accepted)."""
    rgb = np.asarray(cur["rgb"], F)
    h, w = rgb.shape[:2]
    one = F(1.0)
    depth = np.asarray(cur["depth"], F)
    cnoise = np.asarray(cur["noise"], F) if noise else None
    out_rgb = rgb.copy()
    out_noise = cnoise.copy() if noise else None
    out_len = np.ones((h, w), F)
    accepted = np.zeros((h, w), np.int32)
    rejected = np.zeros((h, w), np.int32)
    projected = np.zeros((h, w), bool)
    blended = np.zeros((h, w), bool)
    used = np.zeros((h, w), bool)
    if prev is not None:
        with np.errstate(all="ignore"):
            hit = depth >= F(0.0)
            P, n = np.asarray(cur["position"], F), np.asarray(cur["normal"], F)
            var_c = cnoise * cnoise if noise else np.ones((h, w), F)
            ok, fx, fy = project(P, prev["view"], w, h, fov_degrees)
            ok &= hit
            projected = ok
            # the conversion happens behind the range test only: where it failed, a harmless stand-in
            fxs, fys = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
            x0f, y0f = np.floor(fxs), np.floor(fys)
            x0, y0 = x0f.astype(np.int32), y0f.astype(np.int32)
            tx, ty = fxs - x0f, fys - y0f
            pn = np.asarray(prev["noise"], F) if noise else None
            pl, pd_, pP, pN = (np.asarray(prev[k], F) for k in ("length", "depth", "position", "normal"))
            prgb = np.asarray(prev["rgb"], F)
            tol = F(plane_tolerance) * depth
            sum_c = np.zeros((h, w, 3), F)
            sum_v, sum_l, sum_w = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for j in (0, 1):
                for i in (0, 1):
                    wt = (ty if j else one - ty) * (tx if i else one - tx)
                    qx, qy = x0 + i, y0 + j
                    inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    gx, gy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    good = (pd_[gy, gx] >= F(0.0)) & (pl[gy, gx] >= one)
                    if mesh:
                        good &= np.asarray(prev["mesh"], np.uint32)[gy, gx] == np.asarray(cur["mesh"], np.uint32)
                    nq, Pq = pN[gy, gx], pP[gy, gx]
                    t = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    good &= t >= F(normal_min_dot)
                    E = Pq - P
                    pd = (n[..., 0] * E[..., 0] + n[..., 1] * E[..., 1]) + n[..., 2] * E[..., 2]
                    good &= np.abs(pd) <= tol
                    take = inside & good
                    rejected += inside & ~good
                    accepted += take
                    used[gy[take], gx[take]] = True
                    vq = pn[gy, gx] * pn[gy, gx] if noise else np.ones((h, w), F)
                    sum_c = np.where(take[..., None], sum_c + wt[..., None] * prgb[gy, gx], sum_c)
                    sum_v = np.where(take, sum_v + (wt * wt) * vq, sum_v)
                    sum_l = np.where(take, sum_l + wt * pl[gy, gx], sum_l)
                    sum_w = np.where(take, sum_w + wt, sum_w)
            blended = ok & (sum_w > F(0.0))
            hc = sum_c / sum_w[..., None]
            hv = sum_v / (sum_w * sum_w)
            N = sum_l / sum_w + one
            nmax = F(max_history)
            N = np.where(N < nmax, N, nmax)
            a = one / N
            a = np.where(a > F(alpha_min), a, F(alpha_min))
            om = one - a
            b_rgb = (om[..., None] * hc) + (a[..., None] * rgb)
            var = ((om * om) * hv) + ((a * a) * var_c)
            b_noise = np.sqrt(var.astype(np.float64)).astype(F)
            # a pixel without history keeps its bits: select by mask, on the bits
            out_rgb = np.where(blended[..., None], b_rgb.view(np.uint32), rgb.view(np.uint32)).view(F)
            if noise:
                out_noise = np.where(blended, b_noise.view(np.uint32), cnoise.view(np.uint32)).view(F)
            out_len = np.where(blended, N, one).astype(F)
    res = dict(rgb=np.ascontiguousarray(out_rgb, F), noise=None if out_noise is None else np.ascontiguousarray(out_noise, F),
               length=np.ascontiguousarray(out_len, F))
    if detail:
        res.update(accepted=accepted, rejected=rejected, projected=projected, blended=blended, used=used)
    return res


# ---- the shared fixture
def _rot_x(deg):
    c, s = np.cos(np.deg2rad(np.float64(deg))), np.sin(np.deg2rad(np.float64(deg)))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def _rot_y(deg):
    c, s = np.cos(np.deg2rad(np.float64(deg))), np.sin(np.deg2rad(np.float64(deg)))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


PREV_VIEW = (np.array((0.0, 1.5, 2.0), F), _rot_x(-15.0).astype(F).reshape(9))
CUR_VIEW = (np.array((0.25, 1.55, 1.9), F), (_rot_y(3.0) @ _rot_x(-15.0)).astype(F).reshape(9))


def first_hits(width, height, view, fov_degrees=FOV):
    """The analytic scene seen from `view`, in float32: a floor y = 0 for |x| < 8, z > -6 (mesh 0); a wall z = -6 for |x| < 8,
    0 <= y < 3 (mesh 1); a box's top y = 1 for |x| < 1, -4 < z < -2 and front z = -2 for |x| < 1, 0 <= y < 1 (mesh 2).
    -> dict depth [h, w] (-1 = miss), position, normal [h, w, 3], mesh [h, w] uint32 (0xFFFFFFFF = miss), hit [h, w] bool."""
    pos = np.asarray(view[0], F)
    d = ref_camera.camera_directions(width, height, fov_degrees, np.asarray(view[1], F).reshape(3, 3))
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    best = np.full((height, width), np.inf, F)
    mesh = np.full((height, width), MISS_MESH, np.uint32)
    normal = np.zeros((height, width, 3), F)
    with np.errstate(all="ignore"):
        def plane(t, inside, nrm, m):
            nonlocal best, mesh, normal
            x, y, z = pos[0] + t * dx, pos[1] + t * dy, pos[2] + t * dz
            take = (t > F(0.0)) & inside(x, y, z) & (t < best)
            best = np.where(take, t, best).astype(F)
            mesh = np.where(take, np.uint32(m), mesh)
            normal = np.where(take[..., None], np.asarray(nrm, F), normal)

        t_y0 = (F(0.0) - pos[1]) / dy
        t_y1 = (F(1.0) - pos[1]) / dy
        t_z6 = (F(-6.0) - pos[2]) / dz
        t_z2 = (F(-2.0) - pos[2]) / dz
        plane(t_y0, lambda x, y, z: (np.abs(x) < 8) & (z > -6), (0, 1, 0), 0)
        plane(t_z6, lambda x, y, z: (np.abs(x) < 8) & (y >= 0) & (y < 3), (0, 0, 1), 1)
        plane(t_y1, lambda x, y, z: (np.abs(x) < 1) & (z > -4) & (z < -2), (0, 1, 0), 2)
        plane(t_z2, lambda x, y, z: (np.abs(x) < 1) & (y >= 0) & (y < 1), (0, 0, 1), 2)
    hit = np.isfinite(best)
    depth = np.where(hit, best, F(-1.0)).astype(F)
    position = np.where(hit[..., None], pos + depth[..., None] * d, F(0.0)).astype(F)
    return dict(depth=depth, position=np.ascontiguousarray(position), normal=np.ascontiguousarray(normal), mesh=mesh, hit=hit)


_MESH_COLOUR = np.array(((0.9, 0.6, 0.3), (0.3, 0.5, 0.9), (0.4, 0.8, 0.4)), F)
BACKGROUND = np.array((0.2, 0.3, 0.4), F)


def _shade(g, rng):
    """seeded rgb and noise over the guides g, as denoise_model.synthetic seeds them: colour of the mesh x a ramp along world x,
    plus Gaussian noise whose per-pixel sigma lies in [0.02, 0.12] and is the `noise` plane (0 on a miss)"""
    h, w = g["depth"].shape
    hit = g["hit"]
    base = _MESH_COLOUR[np.where(hit, g["mesh"], 0).astype(np.int64)]
    ramp = (F(0.6) + F(0.05) * g["position"][..., 0])[..., None]
    clean = np.where(hit[..., None], base * ramp, BACKGROUND).astype(F)
    sigma = rng.uniform(0.02, 0.12, (h, w)).astype(F)
    sigma[~hit] = 0.0
    rgb = (clean + sigma[..., None] * rng.standard_normal((h, w, 3)).astype(F)).astype(F)
    return rgb, sigma, clean


def synthetic_pair(width, height, seed=0):
    """-> (cur, prev): the analytic scene from CUR_VIEW and from PREV_VIEW with seeded rgb and noise; prev also has `length`
    (history lengths in [1, 12], 1 on a miss) and `view`.  Both carry hit [h, w] and clean [h, w, 3] for the tests."""
    rng = np.random.default_rng([seed, width, height])
    prev = first_hits(width, height, PREV_VIEW)
    cur = first_hits(width, height, CUR_VIEW)
    prev["rgb"], prev["noise"], prev["clean"] = _shade(prev, rng)
    cur["rgb"], cur["noise"], cur["clean"] = _shade(cur, rng)
    length = rng.uniform(1.0, 12.0, (height, width)).astype(F)
    length[~prev["hit"]] = 1.0
    prev["length"] = length
    prev["view"] = PREV_VIEW
    cur["view"] = CUR_VIEW
    return cur, prev


def hostile_cases():
    """(name, cur, prev, params) at 37x19: legal inputs on which the range test before the conversion, the tests of a tap and the
    bounds of the blend decide; shared with the GPU tests"""
    w, h = 37, 19
    cur, prev = synthetic_pair(w, h)
    rng = np.random.default_rng(7)
    bad = cur["position"].copy()
    pick = rng.permutation(w * h)[: (w * h) // 10]
    values = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F)
    flat = bad.reshape(-1, 3)
    flat[pick, rng.integers(0, 3, pick.size)] = values[rng.integers(0, values.size, pick.size)]
    # a tenth of the pixels, hits among them
    assert cur["hit"].reshape(-1)[pick].sum() >= 10
    yield "positions", dict(cur, position=bad), prev, PARAMS
    yield "zero lengths", cur, dict(prev, length=np.zeros((h, w), F)), PARAMS
    # the previous camera far behind the wall, looking the same way: every surface is behind it
    behind = (np.array((0.0, 1.5, -40.0), F), PREV_VIEW[1])
    yield "view behind", cur, dict(prev, view=behind), PARAMS
    yield "alpha one", cur, prev, dict(PARAMS, alpha_min=1.0)


def run(cur, prev, combo, **params):
    return accumulate(cur, prev, noise="noise" in combo, mesh="mesh" in combo, **params)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
