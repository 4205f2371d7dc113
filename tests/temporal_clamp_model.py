"""The numpy float32 model of rtk_temporal_accumulate_clamped (include/rtk.h spells the arithmetic out) and the fixture its tests
share.  tests/temporal_model.py does not hand out the history's colour before the blend, so steps 2 and 3 of its accumulate() are
restated here as they stand there, and steps 3a to 4 of the clamped contract follow: the box over the NEW frame (dy outer, dx
inner), the bounds, the clamp, the variance floor and the blend.  Every operation in float32 in the order the contract writes it;
the bits are those of csrc/temporal_clamp_math.hpp built with -ffp-contract=off, and of the kernel."""
import numpy as np

import temporal_model as tm
from temporal_model import COMBOS, F, PARAMS, bits  # noqa: F401  (the fixtures the clamp tests share with the plain ones)

LIT = np.array((1.0, 0.6, 1.5), F)                      # what the history's colour is multiplied by, per mesh
CLAMP = dict(radius=1, gamma=1.0, history_keep=1.0)


def accumulate(cur, prev, *, radius, gamma, history_keep, fov_degrees, alpha_min, plane_tolerance, normal_min_dot, max_history,
               noise=True, mesh=True, detail=False):
    """cur, prev, noise, mesh as temporal_model.accumulate.  -> dict rgb, noise (None without the family), length; with detail
    also accepted [h, w] (history taps accepted), blended, clamped, below, above [h, w] bool (some channel's hc < lo / hc > hi),
    box [h, w] (accepted taps of the box), cut_mesh and cut_edge [h, w] bool (a tap of the box was thrown out by the mesh ids /
    lay outside the image)."""
    rgb = np.asarray(cur["rgb"], F)
    h, w = rgb.shape[:2]
    one = F(1.0)
    depth = np.asarray(cur["depth"], F)
    cnoise = np.asarray(cur["noise"], F) if noise else None
    out_rgb = rgb.copy()
    out_noise = cnoise.copy() if noise else None
    out_len = np.ones((h, w), F)
    zb = np.zeros((h, w), bool)
    accepted = np.zeros((h, w), np.int32)
    blended, clamped, below, above, cut_mesh, cut_edge = zb, zb, zb, zb, zb, zb
    box_n = np.zeros((h, w), F)
    if prev is not None:
        with np.errstate(all="ignore"):
            # ---- steps 2 and 3, as temporal_model.accumulate
            hit = depth >= F(0.0)
            P, n = np.asarray(cur["position"], F), np.asarray(cur["normal"], F)
            var_c = cnoise * cnoise if noise else np.ones((h, w), F)
            cmesh = np.asarray(cur["mesh"], np.uint32) if mesh else None
            ok, fx, fy = tm.project(P, prev["view"], w, h, fov_degrees)
            ok &= hit
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
                        good &= np.asarray(prev["mesh"], np.uint32)[gy, gx] == cmesh
                    nq, Pq = pN[gy, gx], pP[gy, gx]
                    t = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    good &= t >= F(normal_min_dot)
                    E = Pq - P
                    pd = (n[..., 0] * E[..., 0] + n[..., 1] * E[..., 1]) + n[..., 2] * E[..., 2]
                    good &= np.abs(pd) <= tol
                    take = inside & good
                    accepted += take
                    vq = pn[gy, gx] * pn[gy, gx] if noise else np.ones((h, w), F)
                    sum_c = np.where(take[..., None], sum_c + wt[..., None] * prgb[gy, gx], sum_c)
                    sum_v = np.where(take, sum_v + (wt * wt) * vq, sum_v)
                    sum_l = np.where(take, sum_l + wt * pl[gy, gx], sum_l)
                    sum_w = np.where(take, sum_w + wt, sum_w)
            blended = ok & (sum_w > F(0.0))
            # ---- 3a: the box over the new frame, for every pixel at once (only the blended ones are kept)
            r = int(radius)
            ys, xs = np.mgrid[0:h, 0:w]
            nf = np.zeros((h, w), F)
            s1, s2 = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
            sv = np.zeros((h, w), F)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    qx, qy = xs + dx, ys + dy
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    gx, gy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    take = inside & hit[gy, gx]
                    cut_edge = cut_edge | ~inside
                    if mesh:
                        same = cmesh[gy, gx] == cmesh
                        cut_mesh = cut_mesh | (take & ~same)
                        take = take & same
                    cq = rgb[gy, gx]
                    nf = np.where(take, nf + one, nf)
                    s1 = np.where(take[..., None], s1 + cq, s1)
                    s2 = np.where(take[..., None], s2 + cq * cq, s2)
                    sv = np.where(take, sv + var_c[gy, gx], sv)
            # ---- 3b
            m = s1 / nf[..., None]
            d = s2 / nf[..., None] - m * m
            d = np.where(d > F(0.0), d, F(0.0))
            sg = np.sqrt(d.astype(np.float64)).astype(F)
            e = F(gamma) * sg
            lo, hi = m - e, m + e
            # ---- 3c
            hc = sum_c / sum_w[..., None]
            lt, gt = hc < lo, hc > hi
            hc2 = np.where(lt, lo, np.where(gt, hi, hc))
            below, above = blended & lt.any(-1), blended & gt.any(-1)
            clamped = below | above
            # ---- 3d
            hv = sum_v / (sum_w * sum_w)
            vb = (sv / nf) / nf
            hv = np.where(clamped, np.where(hv > vb, hv, vb), hv)
            # ---- 4
            L = sum_l / sum_w
            L = np.where(clamped, L * F(history_keep), L)
            N = L + one
            nmax = F(max_history)
            N = np.where(N < nmax, N, nmax)
            a = one / N
            a = np.where(a > F(alpha_min), a, F(alpha_min))
            om = one - a
            b_rgb = (om[..., None] * hc2) + (a[..., None] * rgb)
            var = ((om * om) * hv) + ((a * a) * var_c)
            b_noise = np.sqrt(var.astype(np.float64)).astype(F)
            out_rgb = np.where(blended[..., None], b_rgb.view(np.uint32), rgb.view(np.uint32)).view(F)
            if noise:
                out_noise = np.where(blended, b_noise.view(np.uint32), cnoise.view(np.uint32)).view(F)
            out_len = np.where(blended, N, one).astype(F)
            box_n = np.where(blended, nf, F(0.0))
            cut_mesh, cut_edge = cut_mesh & blended, cut_edge & blended
    res = dict(rgb=np.ascontiguousarray(out_rgb, F), noise=None if out_noise is None else np.ascontiguousarray(out_noise, F),
               length=np.ascontiguousarray(out_len, F))
    if detail:
        res.update(accepted=accepted, blended=blended, clamped=clamped, below=below, above=above, box=box_n, cut_mesh=cut_mesh,
                   cut_edge=cut_edge)
    return res


def lit_pair(width, height, seed=0):
    """tm.synthetic_pair with the history's rgb multiplied per mesh by LIT (misses stay): a lighting change that leaves mesh 0
    alone, dims mesh 1 and brightens mesh 2, so the clamp fires from both sides and not everywhere"""
    cur, prev = tm.synthetic_pair(width, height, seed)
    factor = np.where(prev["hit"][..., None], LIT[np.where(prev["hit"], prev["mesh"], 0).astype(np.int64)][..., None], F(1.0))
    prev = dict(prev, rgb=(prev["rgb"] * factor.astype(F)).astype(F))
    return cur, prev


def hostile_cases():
    """(name, cur, prev, params, clamp) at 37x19: legal inputs on which the comparisons of the bounds decide; shared with the GPU
    tests"""
    w, h = 37, 19
    cur, prev = lit_pair(w, h)
    rng = np.random.default_rng(11)
    bad = cur["rgb"].copy()
    pick = rng.permutation(w * h)[: (w * h) // 10]
    values = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F)
    flat = bad.reshape(-1, 3)
    flat[pick, rng.integers(0, 3, pick.size)] = values[rng.integers(0, values.size, pick.size)]
    assert cur["hit"].reshape(-1)[pick].sum() >= 10
    yield "colours", dict(cur, rgb=bad), prev, PARAMS, dict(radius=2, gamma=2.0, history_keep=0.5)
    yield "gamma zero", cur, prev, PARAMS, dict(radius=1, gamma=0.0, history_keep=1.0)
    # only the pixels at even x and even y are hits: at radius 1 the box of each is its centre tap alone, so lo = hi = c
    ys, xs = np.mgrid[0:h, 0:w]
    lone = np.where((xs % 2 == 0) & (ys % 2 == 0), cur["depth"], F(-1.0)).astype(F)
    yield "box of one", dict(cur, depth=lone), prev, PARAMS, dict(radius=1, gamma=1.0, history_keep=0.0)


def run(cur, prev, combo, clamp=CLAMP, **params):
    return accumulate(cur, prev, noise="noise" in combo, mesh="mesh" in combo, **clamp, **params)
