"""The life of an accel's device memory (csrc/dev_mem.hpp, csrc/accel.hpp): staging buffers and workspaces that grow, are then
large enough, and grow again; the active and spare sets of the updates; and two accels that must not free each other's things.
Everything is compared bit for bit with the same call on a fresh accel, and the first frame with the CPU oracle.  The scene is the
16x16 floor, mirror and light of small_scenes.py: the smallest shapes at which a stale capacity or a lost pointer shows."""
import dataclasses
import gc

import numpy as np
import pytest

from small_scenes import two_quad_scene
from update_checks import _rtk_scene

pytestmark = pytest.mark.gpu

DEPTH = 5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _accel(rtk, flat, **kw):
    return rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), **kw)


def _grow_fit_grow(rtk, flat, call, operands, **kw):
    """call(accel, operand) -> tuple of arrays / numbers.  One accel takes the operands in order; each result must be the
    result of the same call on a fresh accel (made once per distinct operand)."""
    live = _accel(rtk, flat, **kw)
    fresh = {}
    for i, key in enumerate(operands):
        got = call(live, key)
        if key not in fresh:
            fresh[key] = call(_accel(rtk, flat, **kw), key)
        for j, (g, f) in enumerate(zip(got, fresh[key])):
            ok = _same(g, f) if isinstance(g, np.ndarray) and g.dtype == np.float32 else np.array_equal(g, f)
            assert ok, (i, key, j)
    return fresh


def _rays(rtk, flat, side):
    return _accel(rtk, flat).camera_rays(rtk.RenderConfig(width=side, height=side)).reshape(-1, 6)


# ---------------------------------------------------------------- (a) grow, fit, grow

@pytest.mark.parametrize("gi", [0, 2])
def test_radiance_and_occluded_grow_fit_grow(rtk, ora, gi):
    """64, 4096, 64 rays through the staging of rtk_accel_radiance (and the streaming workspace behind it) and of
    rtk_accel_occluded; gi = 2 makes the ray trees fork."""
    flat = two_quad_scene(ora)
    rays = {n: _rays(rtk, flat, side)[:n] for n, side in ((64, 16), (4096, 64))}
    assert all(r.shape == (n, 6) for n, r in rays.items())

    def call(acc, n):
        rgb, cn = acc.radiance(rays[n], cfg=rtk.RadianceConfig(max_ray_depth=DEPTH, diffuse_rays=gi))
        occ, n_int = acc.occluded(rays[n], np.full(n, 10.0, np.float32), count=True)
        return rgb, cn["rays"], occ, n_int

    fresh = _grow_fit_grow(rtk, flat, call, [64, 4096, 64])
    assert len(np.unique(_bits(fresh[4096][0]), axis=0)) > 8 and 0 < int(fresh[4096][2].sum()) < 4096


@pytest.mark.parametrize("mode,launch_units", [("TRACE_GROUP4", None), ("TRACE_GROUP4", 4), ("TRACE_STREAM", None)],
                         ids=["one launch", "a launch per view", "a frame per view"])
def test_render_views_grow_fit_grow(rtk, ora, monkeypatch, mode, launch_units):
    """1, 3, 1 views: all in one launch, cut into a launch per view (a view has 64 units) and, under the streaming pipeline,
    frame after frame; the last two fold the counters of their three parts into the call's."""
    if launch_units:
        monkeypatch.setenv("RTK_VIEWS_LAUNCH_UNITS", str(launch_units))     # (read when an accel is built)
    flat = two_quad_scene(ora)
    views = np.zeros((3, 12), np.float32)
    views[:, 3:] = np.eye(3, dtype=np.float32).reshape(-1)
    views[:, 0] = [0.0, 0.5, -0.5]
    cfg = rtk.RenderConfig(width=16, height=16, max_ray_depth=DEPTH, trace_mode=getattr(rtk, mode))

    def call(acc, k):
        rgb, cn = acc.render_views(cfg, views[:k])
        return rgb, cn["rays"]

    fresh = _grow_fit_grow(rtk, flat, call, [1, 3, 1])
    assert not _same(fresh[3][0][0], fresh[3][0][1])
    # the call's counters are the sum of its views', each view the frame of a fresh accel with that camera
    rays = 0
    for k in range(3):
        acc = _accel(rtk, flat)
        acc.set_camera(views[k, :3], views[k, 3:])
        rgb, cn = acc.render_frame(cfg)
        assert _same(rgb, fresh[3][0][k]), k
        rays += cn["rays"]
    assert fresh[3][1] == rays


@pytest.mark.parametrize("mode", ["TRACE_GROUP4", "TRACE_STREAM"])
def test_render_regions_grow_fit_grow(rtk, ora, mode):
    """One 4x4 rectangle, the whole frame, the 4x4 again, packed and in the frame: the table, the chunk of the streaming path
    and the host variant's staging."""
    flat = two_quad_scene(ora)
    cfg = rtk.RenderConfig(width=16, height=16, max_ray_depth=DEPTH, trace_mode=getattr(rtk, mode))
    rects = {"4x4": [(6, 6, 10, 10)], "frame": [(0, 0, 16, 16)]}

    def call(acc, key):
        packed, cp = acc.render_regions(cfg, rects[key], rtk.REGIONS_PACKED)
        frame, cf = acc.render_regions(cfg, rects[key], rtk.REGIONS_IN_FRAME)
        return packed[0], cp["rays"], frame, cf["rays"]

    fresh = _grow_fit_grow(rtk, flat, call, ["4x4", "frame", "4x4"])
    whole, _ = _accel(rtk, flat).render_frame(cfg)
    assert _same(fresh["frame"][0], whole) and _same(fresh["frame"][2], whole) and _same(fresh["4x4"][0], whole[6:10, 6:10])


@pytest.mark.parametrize("mode,spp,gi", [("TRACE_GROUP4", 1, 0), ("TRACE_STREAM", 1, 0), ("TRACE_STREAM", 3, 2), ("TRACE_TWOPASS", 1, 0)])
def test_render_frame_grow_fit_grow(rtk, ora, mode, spp, gi):
    """16x16, 48x32, 16x16 under every engine with a workspace of its own; the first frame is also the CPU oracle's."""
    flat = two_quad_scene(ora)

    def call(acc, size):
        rgb, cn = acc.render_frame(rtk.RenderConfig(width=size[0], height=size[1], spp=spp, max_ray_depth=DEPTH, diffuse_rays=gi,
                                                    trace_mode=getattr(rtk, mode)))
        return rgb, cn["rays"]

    fresh = _grow_fit_grow(rtk, flat, call, [(16, 16), (48, 32), (16, 16)])
    ref, ocn = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(16, 16, spp, DEPTH, gi)
    assert _same(fresh[(16, 16)][0], ref) and fresh[(16, 16)][1] == ocn["rays"]
    assert len(np.unique(_bits(ref).reshape(-1, 3), axis=0)) > 8


def test_intersect_repack_grow_fit_grow(rtk, ora):
    """RTK_TRACE_REPACK sorts (and takes its workspace) from two rays on (api_batch.hip, `sortable`): 2, 8, 2 rays."""
    flat = two_quad_scene(ora)
    rays = _rays(rtk, flat, 16)[100:108]
    oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)

    def call(acc, n):
        hit = acc.intersect(rays[:n], True, rtk.TRACE_REPACK)
        return hit["tri"], _bits(hit["t"]), _bits(hit["u"]), _bits(hit["v"])

    fresh = _grow_fit_grow(rtk, flat, call, [2, 8, 2])
    ref = oacc.intersect(rays, True)
    assert np.array_equal(fresh[8][0], ref["tri"]) and np.array_equal(fresh[8][1], _bits(ref["t"])) and (ref["tri"] != 0xFFFFFFFF).any()


# ---------------------------------------------------------------- (b) the sets still swap

def _frame(rtk, acc):
    rgb, cn = acc.render_frame(rtk.RenderConfig(width=16, height=16, max_ray_depth=DEPTH))
    return rgb, cn["rays"]


def _check_against_fresh(rtk, acc, flat, what, **kw):
    got, fresh = _frame(rtk, acc), _frame(rtk, _accel(rtk, flat, **kw))
    assert _same(got[0], fresh[0]) and got[1] == fresh[1], what
    return got[0]


def test_the_sets_still_swap(rtk, ora):
    """Vertices twice, a longer triangle list and back, the mirror refractive and back on a FAST accel (its opaque-only tree is
    re-made), one light to five and back: after each step the frame is a fresh accel's of the same arrays."""
    flat = two_quad_scene(ora)
    fast = dict(traversal=rtk.TRAVERSAL_FAST)
    acc = _accel(rtk, flat, **fast)
    frames = [_check_against_fresh(rtk, acc, flat, "build", **fast)]
    # 1. update_vertices twice
    for step, lift in enumerate([0.6, -1.1]):                            # (not a multiple of the half-pixel the 16x16 frame sees the mirror in)
        flat = dataclasses.replace(flat, vertices=(flat.vertices + np.float32([0.0, lift, 0.0]) * (np.arange(8) >= 4)[:, None]).astype(np.float32))
        acc.update_vertices(flat.vertices)
        frames.append(_check_against_fresh(rtk, acc, flat, ("vertices", step), **fast))
    # 2. update_geometry: a third triangle on the floor and one more on the mirror, then the short lists again
    short = flat
    longer = dataclasses.replace(flat, mesh_ntris=np.array([3, 3], np.int32),
                                 indices=np.array([[0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 2, 3], [1, 2, 3]], np.uint32))
    for step, f in enumerate([longer, short]):
        acc.update_geometry(f.vertices, f.indices, f.mesh_ntris)
        frames.append(_check_against_fresh(rtk, acc, f, ("geometry", step), **fast))
    # 3. set_materials: the mirror refractive and back
    glass = dataclasses.replace(flat, mat_kind=np.array([ora.MAT_DIFFUSE, ora.MAT_REFRACTIVE], np.int32), mat_ior=np.array([1.0, 1.5], np.float32))
    for step, f in enumerate([glass, flat]):
        acc.set_materials(f.mat_kind, f.mat_albedo, f.mat_ior, f.mat_smooth)
        frames.append(_check_against_fresh(rtk, acc, f, ("materials", step), **fast))
    # 4. set_lights: one to five and back
    five = dataclasses.replace(flat, light_pos=np.array([[x, 3, -2] for x in (-2, -1, 0, 1, 2)], np.float32),
                               light_intensity=np.full(5, 40, np.float32))
    for step, f in enumerate([five, flat]):
        acc.set_lights(f.light_pos, f.light_intensity)
        frames.append(_check_against_fresh(rtk, acc, f, ("lights", step), **fast))
    # the steps are not no-ops: the moved mirror, the glass and the five lights each change the picture
    assert not _same(frames[0], frames[1]) and not _same(frames[4], frames[5]) and not _same(frames[6], frames[7])
    assert _same(frames[2], frames[4]) and _same(frames[4], frames[6]) and _same(frames[6], frames[8])


# ---------------------------------------------------------------- (c) accels do not free each other's things

def test_accels_do_not_free_each_others_things(rtk, ora):
    """The lane and side streams of the streaming pipeline are the process's, everything else is an accel's own: deleting one
    accel leaves the other, and a third made afterwards, as they were."""
    flat = two_quad_scene(ora)
    cfg = rtk.RenderConfig(width=16, height=16, spp=3, max_ray_depth=DEPTH, diffuse_rays=2, trace_mode=rtk.TRACE_STREAM)
    a, b = _accel(rtk, flat), _accel(rtk, flat)
    first_a, _ = a.render_frame(cfg)
    first_b, _ = b.render_frame(cfg)
    assert _same(first_a, first_b)
    del a
    gc.collect()
    again, _ = b.render_frame(cfg)
    assert _same(again, first_b)
    third, _ = _accel(rtk, flat).render_frame(cfg)
    assert _same(third, first_b)
