"""Ray bundles, triangles and boxes for the culling tests (tests/test_bundle_cull_model.py on the CPU model,
tests/test_gpu_cull_probe.py on the device): near-miss-heavy by construction, and rescaled over the coordinate range the
bundle culling claims (up to kBundleLimit) with the epsilons a scene may ask for."""
import functools

import numpy as np

f32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
KINDS = ("camera", "shadow", "raw")
GRID_SEEDS = {"camera": 11, "shadow": 12, "raw": 13}
# (largest |coordinate| of apex, origins, v0, e1, e2 after rescaling, eps).  Left out because no ray hits anything there, so
# they would prove nothing: 1e-3 with eps >= 1e-6, 1 with eps 0.25.
GRID = ([(t, e) for t in (1.0, 1.0e4) for e in (FLT_MIN, 1e-9, 1e-6, 1e-3)] + [(9.0e8, e) for e in (FLT_MIN, 1e-6, 0.25)] +
        [(1.0e-3, e) for e in (FLT_MIN, 1e-9)])


def bundle(rng, kind):
    C = (rng.normal(size=3) * rng.choice([1.0, 10.0, 60.0])).astype(f32)
    dc = rng.normal(size=3); dc /= np.linalg.norm(dc)
    width = 10.0 ** rng.uniform(-4, -0.5)
    d = dc[None] + width * rng.uniform(-1, 1, size=(64, 3))
    if kind != "raw":
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(f32)
    if kind == "camera":
        o = np.broadcast_to(C, (64, 3)).astype(f32).copy()
    else:                                                   # rays that end in C (shadow rays towards a light), plus some noise
        s = rng.uniform(0.5, 50.0, size=(64, 1))
        noise = rng.choice([0.0, 1e-6, 1e-3]) * rng.normal(size=(64, 3))
        o = (C[None].astype(np.float64) - s * d.astype(np.float64) + noise).astype(f32)
    return C, o, d


def triangles(rng, o, d, n):
    """Triangles placed around points ON the bundle's rays, so that rays pass near (or exactly through) edges and vertices."""
    r = rng.integers(0, 64, size=n)
    t = rng.uniform(0.05, 40.0, size=(n, 1)) * rng.choice([1.0, -0.2], size=(n, 1), p=[0.9, 0.1])
    X = o[r].astype(np.float64) + t * d[r].astype(np.float64)
    size = 10.0 ** rng.uniform(-3, 1, size=(n, 1))
    a = rng.normal(size=(n, 3)) * size; b = rng.normal(size=(n, 3)) * size
    mode = rng.integers(0, 5, size=n)
    bu = rng.uniform(-1.5, 2.5, size=(n, 1)); bv = rng.uniform(-1.5, 2.5, size=(n, 1))
    bu[mode == 1] = 0.0; bv[mode == 2] = 0.0                 # X on an edge
    bu[mode == 3] = 0.0; bv[mode == 3] = 0.0                 # X on the vertex v0
    v0 = X - bu * a - bv * b
    deg = rng.random(n) < 0.03
    b[deg] = a[deg] * rng.uniform(-2, 2, size=(deg.sum(), 1))   # degenerate (zero area)
    return v0.astype(f32), a.astype(f32), b.astype(f32)


def boxes(rng, o, d, n):
    """Boxes around points on the bundle's rays (in front and behind), a quarter of them well off the rays, a quarter flat in one axis and a quarter with a
    face exactly through a ray's origin in one axis (0 * inf in the slab test of a ray with a zero direction component)."""
    r = rng.integers(0, o.shape[0], size=n)
    t = rng.uniform(0.05, 40.0, size=(n, 1)) * rng.choice([1.0, -0.2], size=(n, 1), p=[0.9, 0.1])
    X = o[r].astype(np.float64) + t * d[r].astype(np.float64)
    half = 10.0 ** rng.uniform(-3, 1, size=(n, 3))
    mode = rng.integers(0, 4, size=n); ax = rng.integers(0, 3, size=n); idx = np.arange(n)
    off = rng.uniform(-1.5, 1.5, size=(n, 3)) * half * np.where(mode == 3, 20.0, 1.0)[:, None]     # mode 3: well off the rays
    lo = (X + off - half).astype(f32); hi = (X + off + half).astype(f32)
    flat = mode == 1
    hi[idx[flat], ax[flat]] = lo[idx[flat], ax[flat]]
    face = mode == 2
    lo[idx[face], ax[face]] = o[r[face], ax[face]]
    hi[idx[face], ax[face]] = np.maximum(hi[idx[face], ax[face]], lo[idx[face], ax[face]])
    return lo, hi


@functools.lru_cache(maxsize=None)
def grid_sets(kind, n_bundles=24, n_tris=512):
    """The sets every grid cell starts from, at the generators' natural size: [(C, o, d, v0, e1, e2)] (read-only)."""
    rng = np.random.default_rng(GRID_SEEDS[kind])
    out = []
    for _ in range(n_bundles):
        C, o, d = bundle(rng, kind)
        out.append((C, o, d) + triangles(rng, o, d, n_tris))
    for s in out:
        for a in s:
            a.setflags(write=False)
    return out


def rescale(C, o, d, v0, e1, e2, target, dscale=1.0):
    """The set with its largest |coordinate| (apex, origins, v0, e1, e2) brought to `target` (None: as it is): everything is
    multiplied by target / (the set's own maximum), so nothing is discarded.  Directions keep their length, times `dscale`."""
    s = 1.0 if target is None else float(target) / max(float(np.abs(a).max()) for a in (C, o, v0, e1, e2))
    k = lambda a: (a.astype(np.float64) * s).astype(f32)
    return k(C), k(o), (d.astype(np.float64) * dscale).astype(f32), k(v0), k(e1), k(e2)
