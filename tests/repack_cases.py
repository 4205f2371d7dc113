"""Ray families for the repacking model (tests/test_repack_model.py) and the device probe (tests/test_gpu_repack_probe.py):
small, seeded, and each with the decision it is built to get.  A ray is six float32: o.xyz, d.xyz."""
import numpy as np

f32 = np.float32
EYE = (0.3, 2.0, 1.5)


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def raster(w, h, fov_deg, eye=EYE):
    """The camera rays of a w x h pinhole frame in pixel order: unit directions, fov_deg across the frame's width, looking along -z."""
    t = np.tan(np.radians(fov_deg) / 2.0)
    x = ((np.arange(w) + 0.5) / w * 2.0 - 1.0) * t
    y = (1.0 - (np.arange(h) + 0.5) / h * 2.0) * t * h / w
    d = np.stack([np.tile(x, h), np.repeat(y, w), -np.ones(w * h)], axis=1)
    return np.concatenate([np.tile(np.asarray(eye, np.float64), (w * h, 1)), _unit(d)], axis=1).astype(f32)


def shuffled(rays, seed=1):
    return np.ascontiguousarray(rays[np.random.default_rng(seed).permutation(len(rays))])


def repeated(rays, n):
    """The frame over and over, cut at n rays (a ragged tail)."""
    return np.ascontiguousarray(np.tile(rays, (-(-n // len(rays)), 1))[:n])


def raster_then_noise(w, h, fov_deg, rows, seed=2):
    """A raster for its first `rows` rows and the first ray of the next one, the same frame's rays in no order after them."""
    r = raster(w, h, fov_deg)
    out = r.copy()
    out[rows * w + 1:] = shuffled(r, seed)[rows * w + 1:]
    return out


def one_origin_sphere(n, seed=3, first=(-1.0, 0.05, 0.02), zeros=True):
    """One origin, directions over the whole sphere; `first` picks the pole of the octahedral map; some zero directions."""
    rng = np.random.default_rng(seed)
    d = sphere(rng, n)
    d[0] = first
    if zeros and n > 8:
        d[5::101] = 0.0
    return np.concatenate([np.tile(np.asarray(EYE), (n, 1)), d], axis=1).astype(f32)


POLE_FIRSTS = {4: (-1.0, 0.05, 0.02), 1: (0.05, 1.0, 0.02), 6: (0.05, 0.02, -1.0)}      # pole -> first direction: -x, +y, -z


def uniform(n, seed=4, lo=-3.0, hi=2.0):
    """Origins uniform in a box, directions uniform on the sphere: six dimensions."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(lo, hi, size=(n, 3)), sphere(rng, n)], axis=1).astype(f32)


def all_negative(n, seed=5):
    """Every coordinate of every ray negative."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-9.0, -4.0, size=(n, 3)), -np.abs(sphere(rng, n)) - 1e-3], axis=1).astype(f32)


def few_origins(n, seed=6):
    """Three values of o.x, directions over the sphere: 1 + 3 dimensions."""
    rng = np.random.default_rng(seed)
    r = one_origin_sphere(n, seed, zeros=False)
    r[:, 0] += rng.integers(0, 3, n).astype(f32) * f32(4.0)
    k = min(3, n)
    r[:k, 0] = f32(EYE[0]) + f32(4.0) * np.arange(k, dtype=f32)              # every value is there, whatever n >= 3
    return r


def line(n, seed=7, shuffle=False):
    """Parallel rays from origins on a line along x: exactly one varying dimension.  In order: coherent; shuffled: spread out."""
    x = np.linspace(-5.0, 7.0, n) if n > 1 else np.zeros(1)
    r = np.zeros((n, 6), f32)
    r[:, 0] = x; r[:, 1] = 0.25; r[:, 2] = -1.5; r[:, 5] = -1.0
    return shuffled(r, seed) if shuffle else r


def one_ray(n):
    return np.tile(np.asarray([0.3, 2.0, 1.5, 0.6, 0.0, -0.8], f32), (n, 1))


def non_finite(n, seed=8):
    """Uniform rays with NaN, +-inf and +-1e30, 3e38 components sprinkled in, and whole waves of each (waves 1, 2, 4, where there are)."""
    rng = np.random.default_rng(seed)
    r = uniform(n, seed)
    bad = np.asarray([np.nan, np.inf, -np.inf, 1.0e30, -1.0e30, 3.0e38], f32)
    m = max(1, n // 16)
    r[rng.integers(0, n, m), rng.integers(0, 6, m)] = bad[rng.integers(0, len(bad), m)]
    for wave, val in ((1, np.nan), (2, np.inf), (4, -1.0e30)):
        r[wave * 64:(wave + 1) * 64] = val
    return r


def outside_sample(n, stride, seed=9):
    """Uniform rays whose extremes (o.x = +-100, d.y = +-50) sit in waves that a bounds pass of `stride` does not look at."""
    r = uniform(n, seed)
    waves = (n + 63) // 64
    hidden = [w for w in range(waves) if w % stride != 0]
    assert hidden, "every wave is sampled"
    w = hidden[len(hidden) // 2]
    r[w * 64 + 0, 0] = 100.0; r[w * 64 + 1, 0] = -100.0
    r[w * 64 + 2, 4] = 50.0; r[w * 64 + 3, 4] = -50.0
    return r, np.asarray([w * 64 + 0, w * 64 + 1, w * 64 + 2, w * 64 + 3])


# name -> (rays of n, (sort, dims) the probe is to find at stride 1; None: not stated)
def families(n):
    cam = raster(256, 64, 37.5)                                              # 64 pixels are a quarter of a row: 0.17 wide
    fam = {
        "camera_pixel_order": (repeated(cam, n), (0, 2)),
        "camera_shuffled": (shuffled(repeated(cam, n)), (1, 2)),
        "sphere_pole_-x": (one_origin_sphere(n, first=POLE_FIRSTS[4]), (1, 2)),
        "sphere_pole_+y": (one_origin_sphere(n, first=POLE_FIRSTS[1]), (1, 2)),
        "sphere_pole_-z": (one_origin_sphere(n, first=POLE_FIRSTS[6]), (1, 2)),
        "uniform": (uniform(n), (1, 6)),
        "all_negative": (all_negative(n), (1, 6)),
        "few_origins": (few_origins(n), (1, 4)),
        "line": (line(n), (0, 1)),
        "line_shuffled": (line(n, shuffle=True), (1, 1)),
        "one_ray": (one_ray(n), (0, 0)),
        "non_finite": (non_finite(n), None),
    }
    return fam
