"""What the tests of rtk_accel_set_camera / rtk_render_views share (test_views_abi.py, test_gpu_views.py): three finite cameras
made from a scene's own, and the CPU oracle's frame of the scene under any of them (computed once per shape, never changed)."""
import dataclasses

import numpy as np


def _big_mesh_centre(flat):
    m = int(np.argmax(flat.mesh_ntris))
    a = int(np.sum(flat.mesh_nverts[:m]))
    p = flat.vertices[a:a + int(flat.mesh_nverts[m])].astype(np.float64)
    return (p.min(axis=0) + p.max(axis=0)) / 2


def cameras(flat):
    """A: the scene's camera.  B: orbited 40 degrees about y around the big mesh and raised.  C: turned half round about its own
    up axis, so that it looks straight away from what A looks at.  Each [12] float32: position, matrix (rows: right, up, back)."""
    pos = flat.cam_pos.astype(np.float64)
    rows = flat.cam_mat.astype(np.float64).reshape(3, 3)
    a = np.concatenate([flat.cam_pos, flat.cam_mat]).astype(np.float32)
    th = np.deg2rad(40.0)
    ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    c = _big_mesh_centre(flat)
    rad = np.linalg.norm(pos - c)
    b = np.concatenate([c + ry @ (pos - c) + np.array([0.0, 0.15 * rad, 0.0]), (rows @ ry.T).reshape(-1)]).astype(np.float32)
    away = np.concatenate([pos, (rows * np.array([[-1.0], [1.0], [-1.0]])).reshape(-1)]).astype(np.float32)
    for v in (a, b, away):
        assert np.isfinite(v).all()
    return {"A": a, "B": b, "C": away}


def with_camera(flat, cam, vertices=None):
    kw = dict(cam_pos=np.ascontiguousarray(cam[:3], np.float32), cam_mat=np.ascontiguousarray(cam[3:], np.float32))
    if vertices is not None:
        kw["vertices"] = np.ascontiguousarray(vertices, np.float32)
    return dataclasses.replace(flat, **kw)


class Oracle:
    """oracle frames of one scene file under named cameras; every accel and every frame is made once"""

    def __init__(self, ora, path):
        self.ora = ora
        self.flat = ora.load_crtscene(path)
        self.cams = cameras(self.flat)
        self._acc = {}
        self._frames = {}

    def accel(self, name):
        if name not in self._acc:
            self._acc[name] = self.ora.Accel(self.ora.Scene(with_camera(self.flat, self.cams[name])), self.ora.ACCEL_KD_SIMD)
        return self._acc[name]

    def frame(self, name, w, h, spp=1, depth=5, gi=0):
        key = (name, w, h, spp, depth, gi)
        if key not in self._frames:
            rgb, cn = self.accel(name).render(w, h, spp, depth, gi)
            rgb.setflags(write=False)
            self._frames[key] = (rgb, cn)
        return self._frames[key]

    def views(self, names):
        return np.ascontiguousarray(np.stack([self.cams[n] for n in names]), np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
