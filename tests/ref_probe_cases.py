"""Inputs and comparisons shared by tests/test_ref_probe.py, tests/test_gpu_ref_probe.py, tests/test_material_scenes.py,
tests/test_gpu_material_scenes.py and tools/make_ref_probe_fixtures.py.

A helper, not a test.  The probe (oracle/ref_probe.cpp) is the reference's own code behind a file interface; what it wrote for
the inputs below is recorded under tests/golden/ref_probe/ and must be reproduced bit for bit by the oracle, by the Python
models and by the GPU.  Everything here is deterministic: the recorded inputs are stored with the outputs all the same, so
the tests that read fixtures never depend on a generator."""
import io
import json
import os
import zipfile

import numpy as np

from conftest import SCENES
from occlusion_model import MISS, occluded_ref, segments
from radiance_views import ViewBatch, interior_views, jittered_views, special_rays

FIXTURE_DIR = os.path.join(SCENES, "..", "ref_probe")
FIXTURE_SCENES = {"hw09_scene5": "hw09/scene5", "hw11_scene8": "hw11/scene8", "hw15_scene2": "hw15/scene2", "hw12_scene4": "hw12/scene4"}
FRAME = (96, 54)
DEPTHS = (5, 10)
WIDTHS = (4, 8, 16)
BIAS = 1e-4                      # the reference's shadow / reflection / refraction bias (config.hpp)
HIT_FIELDS = ("t", "u", "v", "w", "position", "hit_normal", "face_normal", "uvs")


def scene_path(rel):
    return os.path.join(SCENES, rel + ".crtscene")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_frame(a, b):
    """tests/test_random_scenes._same_frame: bit-identical, except that a NaN only has to be a NaN on both sides (which
    payload and sign a NaN carries through an addition is a property of the hardware: x86 and the GPU differ)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(np.where(na, np.float32(0), a)), bits(np.where(nb, np.float32(0), b)))


def first_difference(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    d = (na != nb) | (bits(np.where(na, np.float32(0), a)) != bits(np.where(nb, np.float32(0), b)))
    i = np.argwhere(d)
    return None if not len(i) else (tuple(int(x) for x in i[0]), a[tuple(i[0])], b[tuple(i[0])], int(d.sum()))


# ---------------------------------------------------------------- inputs

def ray_sets(flat, oacc, n, seed):
    """name -> float32 [n, 6].  camera: rays of the scene's camera; uniform: origins in the scene box, directions normal
    (un-normalised); axis: one or two direction components +-0; on_plane: origins exactly on a plane of the scene box or
    inside a triangle's plane; boundary: through vertices and edges (test_gpu_parity._boundary_rays, where equal-distance
    ties between neighbouring triangles live); special: zero directions, NaN and inf components."""
    from test_gpu_parity import _boundary_rays, _mixed_rays
    rng = np.random.default_rng(seed)
    v = np.asarray(flat.vertices, np.float32)
    lo, hi = v.min(axis=0), v.max(axis=0)
    cam = oacc.camera_rays(*FRAME).reshape(-1, 6)
    cam = cam[rng.choice(len(cam), n, replace=False)]
    mixed = _mixed_rays(flat, 4 * n, seed)                                   # quarters: camera-like | uniform | axis | vertex to vertex
    uniform, axis = mixed[n:2 * n], mixed[2 * n:3 * n]
    # on a box plane: one coordinate exactly lo or hi; the direction random, a third of them parallel to that plane
    o = rng.uniform(lo - 1, hi + 1, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 2
    ax = rng.integers(0, 3, k)
    o[np.arange(k), ax] = np.where(rng.integers(0, 2, k) == 0, lo[ax], hi[ax])
    par = np.arange(0, k, 3)
    d[par, ax[par]] = 0.0
    # inside a triangle's plane: a float32 barycentric point of a triangle as origin, half of the directions along an edge
    starts = np.concatenate([[0], np.cumsum(flat.mesh_nverts)[:-1]])
    gidx = flat.indices.astype(np.int64) + starts[np.repeat(np.arange(len(flat.mesh_ntris)), flat.mesh_ntris)][:, None]
    t = rng.integers(0, len(gidx), n - k)
    a, b = rng.uniform(0, 0.5, n - k).astype(np.float32), rng.uniform(0, 0.5, n - k).astype(np.float32)
    v0, v1, v2 = (v[gidx[t, j]] for j in range(3))
    o[k:] = v0 + a[:, None] * (v1 - v0) + b[:, None] * (v2 - v0)
    d[k::2] = (v1 - v0)[::2]
    on_plane = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    boundary = _boundary_rays(flat, n, seed + 1)
    special, _ = special_rays(np.concatenate([cam[: n // 2], uniform[: n - n // 2]]))
    special[::53, 3:] = -0.0
    return {"camera": cam, "uniform": uniform, "axis": axis, "on_plane": on_plane, "boundary": boundary, "special": special}


def occlusion_queries(flat, oacc, n, seed):
    """The query families of tests/test_gpu_occluded.py -> (rays, max_t): segments between points of the scene box; max_t
    exactly the closest hit's t (the loop ends through its guard behind a transmissive surface); max_t NaN, inf, negative
    and +-0; zero-length rays (zero direction); NaN and inf components."""
    rays, max_t = segments(flat, n, seed)
    r2, _ = segments(flat, n // 2, seed + 1)
    h = oacc.intersect(r2, cull=False)
    sel = h["mesh"] != MISS
    r2, t2 = r2[sel], h["t"][sel].copy()
    r3, t3 = segments(flat, n // 2, seed + 2)
    i = np.arange(len(r3))
    t3[i % 8 == 0] = np.nan
    t3[i % 8 == 1] = np.inf
    t3[i % 8 == 2] = -1.0
    t3[i % 8 == 3] = 0.0
    t3[i % 8 == 4] = -0.0
    r3, _ = special_rays(r3)
    return np.ascontiguousarray(np.concatenate([rays, r2, r3])), np.ascontiguousarray(np.concatenate([max_t, t2, t3]))


def radiance_views(ora, flat, name, k, w, h):
    """The view families of tests/test_gpu_radiance.py: views inside the scene, for the textured scenes views near the camera."""
    views = jittered_views(flat, k) if name.startswith("hw12") or name == "hw11_scene4" else interior_views(flat, k)
    return ViewBatch(ora, views, w, h)


# ---------------------------------------------------------------- what a scene's fixture holds

def record(ora, flat, name, n_rays=224, n_seg=1024, views=(2, 32, 32)):
    """Run the probe (width 8; the packet counts at every width) on the inputs above -> (arrays, command lines)."""
    oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
    out, argv = {}, []
    p5 = ora.RefProbe(flat, 8, 5, size=FRAME)
    p10 = ora.RefProbe(flat, 8, 10, size=FRAME)

    def ran(p):
        argv.append(" ".join(os.path.basename(a) for a in p.argv))

    out["tree_box"], out["tree_link"], out["tree_refs"], _ = p5.tree(); ran(p5)
    out["tree_packets"] = np.array([ora.RefProbe(flat, w).tree()[3] for w in WIDTHS], np.int64)
    sets = ray_sets(flat, oacc, n_rays, seed=5)
    out["rays"] = np.ascontiguousarray(np.concatenate(list(sets.values())))
    out["hits"] = p5.intersect(out["rays"]); ran(p5)
    out["occ_rays"], out["occ_max_t"] = occlusion_queries(flat, oacc, n_seg, seed=1)
    out["occ_answer"] = p5.occluded(out["occ_rays"], out["occ_max_t"]); ran(p5)
    out["occ_calls"] = np.array([p5.calls], np.int64)
    vb = radiance_views(ora, flat, name, *views)
    out["rad_rays"] = vb.rays
    for d, p in ((5, p5), (10, p10)):
        out[f"rad_rgb_d{d}"] = p.radiance(vb.rays); ran(p)
        out[f"rad_calls_d{d}"] = np.array([p.calls], np.int64)
        out[f"frame_d{d}"] = p.frame(); ran(p)
        out[f"frame_calls_d{d}"] = np.array([p.calls, p.hits], np.int64)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}, argv


# ---------------------------------------------------------------- the generated material scenes (tests/material_scenes.py)

MATERIAL_PREFIX = "material_"


def material_fixture_names():
    import material_scenes as ms
    return {MATERIAL_PREFIX + v: v for v in ms.VARIANTS}


def record_material(ora, flat):
    """Run the probe (width 8; the packet counts at every width) on one variant of tests/material_scenes.py -> (arrays, command
    lines): the tree, the 48 x 32 frame at max_ray_depth 1, 5, 10 and 16 with the probe's counts of intersect calls and hits,
    the radiance of the special rays and of a 32 x 32 view at depths 5 and 16, the stacked-glass occlusion queries, and the
    scene's own arrays."""
    import material_scenes as ms
    out, argv = {}, []
    probes = {d: ora.RefProbe(flat, 8, d, size=ms.SIZE) for d in ms.DEPTHS}

    def ran(p):
        argv.append(" ".join(os.path.basename(a) for a in p.argv))

    p5 = probes[5]
    out["tree_box"], out["tree_link"], out["tree_refs"], _ = p5.tree(); ran(p5)
    out["tree_packets"] = np.array([ora.RefProbe(flat, w).tree()[3] for w in WIDTHS], np.int64)
    out["occ_rays"], out["occ_max_t"], _ = ms.stacked_glass_queries()
    out["occ_answer"] = p5.occluded(out["occ_rays"], out["occ_max_t"]); ran(p5)
    out["occ_calls"] = np.array([p5.calls], np.int64)
    out["rad_rays"], _ = ms.radiance_rays(ora, flat)
    for d in ms.RAD_DEPTHS:
        out[f"rad_rgb_d{d}"] = probes[d].radiance(out["rad_rays"]); ran(probes[d])
        out[f"rad_calls_d{d}"] = np.array([probes[d].calls], np.int64)
    for d in ms.DEPTHS:
        out[f"frame_d{d}"] = probes[d].frame(); ran(probes[d])
        out[f"frame_calls_d{d}"] = np.array([probes[d].calls, probes[d].hits], np.int64)
    out.update(ms.scene_arrays(flat))
    return {k: np.ascontiguousarray(v) for k, v in out.items()}, argv


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w") as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


PARTS = ("queries", "frames")     # two files per scene keep every committed file small


def part_of(key):
    return "frames" if key.startswith(("frame_", "rad_")) else "queries"


def load_fixture(name):
    out = {}
    for part in PARTS:
        with np.load(os.path.join(FIXTURE_DIR, f"{name}_{part}.npz"), allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out


def manifest():
    with open(os.path.join(FIXTURE_DIR, "MANIFEST.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- comparisons against the oracle and the models

def oracle_hits(ora, oacc, rays):
    """The oracle's answer in the probe's record layout, REF_HIT_DTYPE [2, n] (row 0 cull off, row 1 cull on)."""
    out = np.zeros((2, len(rays)), ora.REF_HIT_DTYPE)
    for cull in (0, 1):
        h = oacc.intersect(rays, bool(cull))
        rest = oacc.intersect_rest(rays, bool(cull))
        hit = h["tri"] != MISS
        o = out[cull]
        o["hit"] = hit
        o["mesh"], o["tri"] = h["mesh"], h["tri"]
        for f in ("t", "u", "v"):
            o[f] = np.where(hit, h[f], np.float32(0))
        o["hit_normal"] = np.where(hit[:, None], h["normal"], np.float32(0))
        for f in ("w", "position", "face_normal", "uvs"):
            o[f] = rest[f]
    return out


def hits_differences(ref, got, fields=HIT_FIELDS, what="", nan_sign_free=False):
    """-> list of disagreements between two REF_HIT_DTYPE arrays.  The triangle index is compared where the reference's
    hit has exactly one owner (ref_probe.cpp: owner_of): a duplicated triangle gives the same hit<F> whichever copy wins.
    Floats are compared on their bits, NaNs included.
    nan_sign_free=True is for kd_tree_accel (--scalar) alone: a ray with a non-finite or zero component can give dist = NaN,
    which its `dist < eps` lets through as a hit (the packet test's `eps < t`, `0 <= u`, `0 <= v` reject every NaN).  Such a
    NaN then has to be a NaN in the same component on both sides, no more: which operand's sign and payload an x86 addition
    or multiplication of two NaNs keeps depends on the operand order the compiler chose, and the probe (clang) and the oracle
    (gcc) are built by different compilers."""
    bad = []
    for cull in (0, 1):
        r, g = ref[cull], got[cull]
        if not np.array_equal(r["hit"], g["hit"]):
            i = int(np.flatnonzero(r["hit"] != g["hit"])[0])
            bad.append(f"{what} cull={cull}: hit/miss differs first at ray {i}: reference {r['hit'][i]}, t={r['t'][i]!r} vs t={g['t'][i]!r}")
            continue
        hit = r["hit"] == 1
        if not np.array_equal(r["mesh"][hit], g["mesh"][hit]):
            bad.append(f"{what} cull={cull}: mesh differs first at ray {int(np.flatnonzero(hit & (r['mesh'] != g['mesh']))[0])}")
        one = hit & (r["owners"] == 1)
        if not np.array_equal(r["tri"][one], g["tri"][one]):
            i = int(np.flatnonzero(one & (r["tri"] != g["tri"]))[0])
            bad.append(f"{what} cull={cull}: triangle differs first at ray {i}: reference {r['tri'][i]} vs {g['tri'][i]}")
        for f in fields if hit.any() else ():
            a, b = r[f][hit].reshape(int(hit.sum()), -1), g[f][hit].reshape(int(hit.sum()), -1)
            d = bits(a) != bits(b)
            if nan_sign_free:
                d &= ~(np.isnan(a) & np.isnan(b))
            d = np.flatnonzero(d.any(axis=1))
            if d.size:
                i = int(np.flatnonzero(hit)[d[0]])
                bad.append(f"{what} cull={cull}: {f} differs at {d.size} rays, first ray {i}: reference {r[f][i]!r} vs {g[f][i]!r}")
    return bad


def model_occluded(oacc, flat, rays, max_t):
    """tests/occlusion_model.py over the oracle's closest hit -> (answer bytes, calls of intersect)"""
    want, steps, entered = occluded_ref(oacc, flat, rays, max_t, BIAS, max_steps=1 << 30, with_entered=True)
    return want, int(steps.sum(dtype=np.int64) + entered.sum())


def at_eps_rays(ora, flat, eps, n, seed):
    """Rays whose closest hit lies at a distance of exactly eps, where the packet test's `eps < t` and the scalar test's
    `dist < eps` part ways: straight down onto the floor quad of test_random_scenes._make_scene (y = -2, mesh 2) from a height
    of eps * s with a direction of length s, all coordinates multiples of 1/8.  Of n candidates, those for which the oracle,
    built with the smallest eps, computes t == float32(eps) to the bit.  -> float32 [m, 6]"""
    rng = np.random.default_rng(seed)
    s = rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 0.75, 1.5, 3.0], np.float32), n)
    o = np.empty((n, 3), np.float32)
    o[:, 0] = rng.integers(-47, 48, n) / np.float32(8)
    o[:, 2] = rng.integers(-47, 48, n) / np.float32(8)
    o[:, 1] = np.float32(-2.0) + np.float32(eps) * s
    d = np.zeros((n, 3), np.float32)
    d[:, 1] = -s
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    h = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD, eps=ora.FLT_MIN).intersect(rays, cull=False)
    return rays[(h["mesh"] == 2) & (bits(h["t"]) == bits(np.float32(eps)))]


# ---------------------------------------------------------------- the fixture for hits at exactly eps

EPS_FIXTURE = "generated100_eps025"      # test_random_scenes._make_scene(ora, 100) in front of the eps = 0.25 variant


def record_eps(ora, flat, n=256):
    """-> (arrays, command lines): at_eps_rays and, for comparison, the same rays started 1/8 higher (plain hits), in front
    of the reference built with eps = 0.25; the scene's vertices and indices go along so that a reader can tell that
    _make_scene still gives the recorded scene."""
    edge = at_eps_rays(ora, flat, 0.25, 4000, seed=3)[:n]
    above = edge.copy()
    above[:, 1] += np.float32(0.125) * -above[:, 4]
    rays = np.ascontiguousarray(np.concatenate([edge, above]))
    p = ora.RefProbe(flat, 8, 5, "eps_0.25")
    out = {"eps_rays": rays, "eps_hits": p.intersect(rays), "scene_vertices": np.ascontiguousarray(flat.vertices, np.float32),
           "scene_indices": np.ascontiguousarray(flat.indices, np.uint32)}
    return out, [" ".join(os.path.basename(a) for a in p.argv)]
