"""Views for the batched radiance query (rtk_accel_radiance) and their oracle side.

A frame the CPU oracle renders with spp = 1 IS the radiance of its camera rays (render/render.hpp:64-72), and oracle.FlatScene is
a dataclass: dataclasses.replace(flat, cam_pos=.., cam_mat=..) is the same geometry, lights and materials under another camera.
So k views of one scene give k oracle frames on one side and ONE batch of k * w * h caller-supplied rays on the other, for an
accel built once from the unmodified scene.  tests/test_radiance_views.py checks on the oracle alone that the views reach the
materials the GPU tests are there for."""
import dataclasses

import numpy as np

MISS = 0xFFFFFFFF
KIND_MISS = -1


def _bounds(flat):
    return flat.vertices.min(axis=0).astype(np.float64), flat.vertices.max(axis=0).astype(np.float64)


def interior_views(flat, k, seed=7):
    """Camera positions uniform in the middle 80 % of the vertex bounding box, orientation a random rotation."""
    lo, hi = _bounds(flat)
    rng = np.random.default_rng(seed)
    for _ in range(k):
        pos = (lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)).astype(np.float32)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        yield dataclasses.replace(flat, cam_pos=pos, cam_mat=q.astype(np.float32).reshape(-1))


def jittered_views(flat, k, seed=3):
    """The scene's own camera moved by +-10 % of the bounding-box extent per axis and turned by up to +-15 degrees about each axis."""
    lo, hi = _bounds(flat)
    rng = np.random.default_rng(seed)
    for _ in range(k):
        pos = (flat.cam_pos + (hi - lo) * rng.uniform(-0.1, 0.1, 3)).astype(np.float32)
        a = np.radians(rng.uniform(-15.0, 15.0, 3))
        (cx, cy, cz), (sx, sy, sz) = np.cos(a), np.sin(a)
        r = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
             @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
        yield dataclasses.replace(flat, cam_pos=pos,
                                  cam_mat=(r @ flat.cam_mat.reshape(3, 3).astype(np.float64)).astype(np.float32).reshape(-1))


class ViewBatch:
    """k views of one scene at w x h: the oracle accels (one per view: the camera lives in the scene), the batch of their camera
    rays in view-major, row-major order, and ids = pixel index within the view (the RNG root key of a frame's pixel)."""

    def __init__(self, ora, views, w, h, fov=90.0, **accel_kw):
        self.w, self.h, self.fov = w, h, fov
        self.views = list(views)
        self.accs = [ora.Accel(ora.Scene(v), ora.ACCEL_KD_SIMD, **accel_kw) for v in self.views]
        self.k = len(self.accs)
        self.n = self.k * w * h
        self.ids = np.tile(np.arange(w * h, dtype=np.uint32), self.k)
        self.rays = self.camera_rays()

    def camera_rays(self, spp=1, sample=0, seed=42):
        return np.concatenate([a.camera_rays(self.w, self.h, spp=spp, seed=seed, fov_degrees=self.fov, sample=sample).reshape(-1, 6)
                               for a in self.accs])

    def frames(self, spp=1, max_depth=5, diffuse_rays=0, seed=42):
        """-> (rgb float32 [k * w * h, 3] in the batch's order, the oracle's intersect() invocations summed over the views)"""
        rgb, rays = [], 0
        for a in self.accs:
            f, cn = a.render(self.w, self.h, spp, max_depth, diffuse_rays, seed=seed, fov_degrees=self.fov)
            rgb.append(f.reshape(-1, 3))
            rays += cn["rays"]
        return np.concatenate(rgb), rays

    def level0(self, cull=True):
        """Closest hits of the batch's own rays -> (hits HIT_DTYPE[n], kind int32[n]: the hit material's MAT_*, KIND_MISS on a miss)"""
        flat = self.views[0]
        hits = self.accs[0].intersect(self.rays, cull=cull)           # (the geometry is the same under every camera)
        hit = hits["mesh"] != MISS
        kind = np.full(self.n, KIND_MISS, np.int32)
        kind[hit] = flat.mat_kind[flat.mesh_material[hits["mesh"][hit]]]
        return hits, kind


def kind_counts(kind):
    return {int(k): int(c) for k, c in zip(*np.unique(kind, return_counts=True))}


def with_constant_material(ora, flat, from_kind):
    """`flat` with its first material of kind `from_kind` turned into a constant material (color_hit's :302-303)."""
    idx = int(np.flatnonzero(flat.mat_kind == from_kind)[0])
    mk = flat.mat_kind.copy()
    mk[idx] = ora.MAT_CONSTANT
    return dataclasses.replace(flat, mat_kind=mk)


def rtk_scene_from_flat(rtk, f):
    return rtk.Scene.from_arrays(f.mesh_material, f.mesh_nverts, f.mesh_ntris, f.vertices, f.indices, f.mat_kind, f.mat_albedo,
                                 f.mat_ior, f.mat_smooth, f.light_pos, f.light_intensity, f.cam_pos, f.cam_mat, f.background,
                                 f.width, f.height, f.bucket_size)


def special_rays(rays):
    """NaN / +-inf components and zero directions mixed into a copy of `rays` (the patterns of test_gpu_occluded's
    test_special_values) -> (rays, bool[n]: the ray was touched)"""
    rays = rays.copy()
    i = np.arange(len(rays))
    rays[i % 29 == 5, 3:] = 0.0                     # zero direction
    rays[i % 31 == 6, 1] = np.nan                   # NaN origin component
    rays[i % 37 == 7, 4] = np.inf                   # inf direction component
    rays[i % 41 == 9, 5] = -np.inf
    rays[i % 43 == 1, 0] = np.inf                   # inf origin component
    rays[i % 47 == 2, 3] = np.nan                   # NaN direction component
    touched = (i % 29 == 5) | (i % 31 == 6) | (i % 37 == 7) | (i % 41 == 9) | (i % 43 == 1) | (i % 47 == 2)
    return rays, touched
