"""The numpy float32 model of rtk_denoise_frame (include/rtk.h spells the arithmetic out) and the seeded synthetic planes that the
denoise tests share.  One shifted-array expression per tap, the taps in the stated order (dy outer, dx inner), every operation in
float32 in the order the contract writes it: numpy does not contract a multiply and an add, so the bits are those of the scalar
C++ of csrc/denoise_math.hpp built with -ffp-contract=off, and of the kernel."""
import numpy as np

F = np.float32
H5 = (F(1.0 / 16.0), F(0.25), F(0.375), F(0.25), F(1.0 / 16.0))
CENTRE = F(0.140625)
DEN_EPS = F(1e-8)
BACKGROUND = (0.2, 0.3, 0.4)
# the parameters the issue's figures were measured with
PARAMS = dict(iterations=5, normal_power_log2=2, sigma_luminance=1.5, sigma_plane=0.05, albedo_floor=0.01)
SIZES = ((37, 19), (5, 3), (1, 1), (70, 36))                  # width x height
ITERATIONS = {(37, 19): 5, (5, 3): 3, (1, 1): 2, (70, 36): 5}
COMBOS = ("noise+albedo", "neither", "noise")                # which optional planes a case hands in


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _shift(a, dx, dy):
    """out[.., y, x, ..] = a[.., y + dy, x + dx, ..] where that lies inside the image, else 0; a: [n, h, w, ...]"""
    out = np.zeros_like(a)
    h, w = a.shape[1], a.shape[2]
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y1 > y0 and x1 > x0:
        out[:, y0:y1, x0:x1] = a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def denoise(rgb, normal, position, depth, noise=None, albedo=None, *, iterations, normal_power_log2, sigma_luminance, sigma_plane,
            albedo_floor):
    """-> rgb_out, float32 of rgb's shape.  rgb, normal, position, albedo: [h, w, 3] or [n, h, w, 3]; depth, noise: [h, w] or [n, h, w]."""
    rgb = np.asarray(rgb, F)
    single = rgb.ndim == 3
    lift = (lambda a: None if a is None else np.asarray(a, F)[None]) if single else (lambda a: None if a is None else np.asarray(a, F))
    rgb, normal, position, depth, noise, albedo = (lift(a) for a in (rgb, normal, position, depth, noise, albedo))
    floor, sl, sp = F(albedo_floor), F(sigma_luminance), F(sigma_plane)
    one = F(1.0)
    with np.errstate(all="ignore"):
        hit = depth >= F(0.0)                                  # (a NaN is no hit)
        hit3 = hit[..., None]
        # ---- prologue
        c = rgb.copy()
        var = np.ones(depth.shape, F) if noise is None else noise * noise
        if albedo is not None:
            a = np.where(albedo > floor, albedo, floor)
            c = np.where(hit3, rgb / a, rgb)
            la = lum(a)
            var = np.where(hit, var / (la * la), var)
        # ---- iterations
        sl2, sp2 = sl * sl, sp * sp
        inside_all = np.ones(depth.shape, bool)
        for k in range(iterations):
            s = 1 << k
            lp = lum(c)
            den = sl2 * var + DEN_EPS
            sum_c = np.zeros_like(c)
            sum_v = np.zeros_like(var)
            sum_w = np.zeros_like(var)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        w = np.full(depth.shape, CENTRE, F)
                        ok, cq, vq = hit, c, var
                    else:
                        sx, sy = s * dx, s * dy
                        ok = hit & _shift(inside_all, sx, sy) & _shift(hit, sx, sy)
                        nq, pq, cq, vq = _shift(normal, sx, sy), _shift(position, sx, sy), _shift(c, sx, sy), _shift(var, sx, sy)
                        t = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2]
                        t = np.where(t > F(0.0), t, F(0.0))
                        for _ in range(normal_power_log2):
                            t = t * t
                        d = pq - position
                        pd = (normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1]) + normal[..., 2] * d[..., 2]
                        wd = one / (one + (pd * pd) / sp2)
                        dl = lum(cq) - lp
                        wl = one / (one + (dl * dl) / den)
                        w = (((H5[dy + 2] * H5[dx + 2]) * t) * wd) * wl
                    sum_c = np.where(ok[..., None], sum_c + w[..., None] * cq, sum_c)
                    sum_v = np.where(ok, sum_v + (w * w) * vq, sum_v)
                    sum_w = np.where(ok, sum_w + w, sum_w)
            c = np.where(hit3, sum_c / sum_w[..., None], c)
            var = np.where(hit, sum_v / (sum_w * sum_w), var)
        # ---- epilogue
        out = np.where(hit3, c * a, c) if albedo is not None else c
    out = np.ascontiguousarray(out, F)
    return out[0] if single else out


def synthetic(width, height, seed=0):
    """Seeded planes of one image: a floor (normal 0 1 0), a wall (normal 0.6 0 0.8) right of 55 % of the width, a band of misses
    in the top 20 % of the rows (rounded to whole rows), colour = albedo x a horizontal ramp + Gaussian noise whose per-pixel sigma
    lies in [0.02, 0.12] and is the `noise` plane.  -> dict of float32 arrays: rgb, clean, albedo, normal, position [h, w, 3];
    depth, noise [h, w]; and the bool masks hit, wall."""
    rng = np.random.default_rng([seed, width, height])
    ys, xs = np.mgrid[0:height, 0:width]
    wall = xs >= int(0.55 * width + 0.5)
    hit = ys >= int(0.2 * height + 0.5)
    wall &= hit
    floor = hit & ~wall
    normal = np.zeros((height, width, 3), F)
    normal[floor] = (0.0, 1.0, 0.0)
    normal[wall] = (0.6, 0.0, 0.8)
    # the floor is the plane y = 0; the wall is spanned by (0.8, 0, -0.6) and (0, 1, 0), both orthogonal to its normal
    u, v = xs.astype(F) * F(0.1), ys.astype(F) * F(0.1)
    position = np.zeros((height, width, 3), F)
    position[floor] = np.stack([u, np.zeros_like(u), v], -1)[floor]
    position[wall] = np.stack([F(0.8) * u, v, F(-0.6) * u], -1)[wall]
    depth = np.where(hit, F(1.0) + F(0.05) * v + F(0.01) * u, F(-1.0)).astype(F)
    # a checker of two albedos per surface: what dividing by the albedo is for
    check = (((xs // 3) + (ys // 3)) & 1).astype(F)[..., None]
    base = np.where(wall[..., None], np.array((0.3, 0.5, 0.9), F), np.array((0.9, 0.6, 0.3), F))
    albedo = (base * (F(0.6) + F(0.4) * check)).astype(F)
    albedo[~hit] = BACKGROUND
    ramp = (F(0.2) + F(0.8) * xs.astype(F) / F(max(width - 1, 1)))[..., None]
    clean = (albedo * ramp).astype(F)
    clean[~hit] = BACKGROUND
    sigma = rng.uniform(0.02, 0.12, (height, width)).astype(F)
    sigma[~hit] = 0.0
    rgb = (clean + sigma[..., None] * rng.standard_normal((height, width, 3)).astype(F)).astype(F)
    return dict(rgb=rgb, clean=clean, albedo=albedo, normal=normal, position=position, depth=depth, noise=sigma, hit=hit, wall=wall)


def stack(images):
    """several synthetic() images of one size as planes [n, h, w(, 3)]"""
    return {k: np.ascontiguousarray(np.stack([im[k] for im in images])) for k in images[0]}


def knob_case():
    """What the children of the RTK_DENOISE_LDS_MAX_STEP test filter: two different 130x70 images, six iterations (steps 1..32:
    staged and direct steps whatever the knob says, tiles with their halo inside the image and taps beyond the frame)."""
    return stack([synthetic(130, 70, seed=1), synthetic(130, 70, seed=2)]), dict(PARAMS, iterations=6)


def optional_planes(planes, combo):
    """(noise, albedo) of a case"""
    return (planes["noise"] if combo in ("noise+albedo", "noise") else None, planes["albedo"] if combo == "noise+albedo" else None)


def run(planes, combo, **params):
    noise, albedo = optional_planes(planes, combo)
    return denoise(planes["rgb"], planes["normal"], planes["position"], planes["depth"], noise, albedo, **params)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
