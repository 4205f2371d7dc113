"""RTK_TRAVERSAL_FAST (rtk.h): front-to-back leaf order behind a flag, NOT the parity mode (the reference's
own to-do, README.md:118-124; kd_tree_simd.hpp:207-214 has no near/far ordering).

What must hold: the closest distance t of every ray is the parity mode's, bit for bit; hit / miss is the same; a different
triangle may win only where several are hit at exactly that t.  Frames differ on a stated, small number of tie pixels."""
import os

import numpy as np
import pytest

from conftest import CONFIG_SCENES, SCENE5, SCENE8
from test_reference_outputs import fixture, _device_rgb8


def test_flag_is_validated_and_off_by_default(rtk):
    sc = rtk.parse_scene_file(SCENE5)
    assert rtk.TRAVERSAL_REFERENCE == 0 and rtk.TRAVERSAL_FAST == 1
    rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST)               # builds its eight leaf orders on the host, no GPU needed
    with pytest.raises(rtk.RtkError) as e:
        rtk.KdTreeSimdAccel(sc, traversal=7)
    assert e.value.code == rtk.RTK_ERR_INVALID


def _mixed_rays(rtk, acc, n_secondary=30_000, seed=7):
    cam = acc.camera_rays(rtk.RenderConfig(width=320, height=180)).reshape(-1, 6)
    rng = np.random.default_rng(seed)
    o = rng.uniform(-12, 12, size=(n_secondary, 3)).astype(np.float32)
    d = rng.normal(size=(n_secondary, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([cam, np.concatenate([o, d], axis=1)]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(CONFIG_SCENES))
@pytest.mark.parametrize("cull", [True, False])
def test_fast_traversal_keeps_every_distance(rtk, scene, cull):
    sc = rtk.parse_scene_file(CONFIG_SCENES[scene])
    ref_acc, fast_acc = rtk.KdTreeSimdAccel(sc), rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST)
    rays = _mixed_rays(rtk, ref_acc)
    a = ref_acc.intersect(rays, cull, rtk.TRACE_WAVE)
    b = fast_acc.intersect(rays, cull, rtk.TRACE_WAVE)
    assert np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32))           # same closest distance (miss: t = -1 on both)
    assert np.array_equal(a["tri"] == 0xFFFFFFFF, b["tri"] == 0xFFFFFFFF)
    other = a["tri"] != b["tri"]
    assert other.mean() < 0.01                                                     # ties only: shared edges / vertices, duplicates
    # where another triangle won, the parity mode's triangle gives that same t: check by asking the parity accel per-lane
    c = ref_acc.intersect(rays[other], cull, rtk.TRACE_LANE)
    assert np.array_equal(c["t"].view(np.uint32), b["t"][other].view(np.uint32))


@pytest.mark.gpu
def test_fast_traversal_frame_equals_the_reference_render_except_on_tie_pixels(rtk):
    """hw11/scene8 at 1920x1080 (the reference's refractive_dragon.png): with front-to-back order the 8-bit frame differs from
    the reference's own render on at most 64 of 2,073,600 pixels (measured: see the assertion message), through both engines."""
    ref = fixture("refractive_dragon")
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8), traversal=rtk.TRAVERSAL_FAST)
    for mode in (3, 6):
        out = _device_rgb8(rtk, acc, rtk.RenderConfig(width=1920, height=1080, spp=1, max_ray_depth=5, trace_mode=mode), 1920, 1080)
        diff = int((out != ref).any(axis=2).sum())
        assert diff <= 64, f"{diff} pixels differ from the reference's render (mode {mode})"
        print(f"fast traversal, mode {mode}: {diff} of {ref.shape[0] * ref.shape[1]} pixels differ from outputs/refractive_dragon.png")


@pytest.mark.gpu
def test_env_switch(rtk, monkeypatch):
    """RTK_TRAVERSAL_FAST=1 in the environment when an accel is built turns it on as well (read once, at rtk_accel_build)."""
    sc = rtk.parse_scene_file(SCENE5)
    monkeypatch.setenv("RTK_TRAVERSAL_FAST", "1")
    fast = rtk.KdTreeSimdAccel(sc)
    monkeypatch.delenv("RTK_TRAVERSAL_FAST")
    parity = rtk.KdTreeSimdAccel(sc)
    explicit = rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST)
    cfg = rtk.RenderConfig(width=640, height=360)
    a, ca = fast.render_frame(cfg)
    b, cb = explicit.render_frame(cfg)
    c, cc = parity.render_frame(cfg)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ca["rays"] == cb["rays"] == cc["rays"]                                    # the same rays are spawned: same hits and misses
    assert (np.abs(a - c).max(axis=2) > 0).mean() < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(name + tag, path, kw, deep)
                                  for name, path, kw in [("scene8", SCENE8, dict(width=640, height=360, spp=2, max_ray_depth=10)),
                                                         ("hw15_scene2_gi", CONFIG_SCENES["hw15_scene2"],
                                                          dict(width=384, height=384, spp=4, max_ray_depth=5, diffuse_rays=1))]
                                  for tag, deep in [("", None), ("_deep_lane", (0, 1)), ("_deep_auto", (0, 0))]], ids=lambda c: c[0])
def test_fast_occlusion_through_transmissive_surfaces_is_one_query(rtk, case, monkeypatch):
    """RTK_TRAVERSAL_FAST on scenes with transmissive materials (rtk.h): the streaming pipeline's occlusion query is ONE any-hit query
    against the opaque triangles instead of is_occluded's stepping loop (render.hpp:110-131).  Fewer rays are traced, and the frame is
    the parity mode's except where the two rules really differ (an occluder within shadow_bias behind a transmissive surface, a ray
    grazing an occluder's edge): at most 1 pixel in 10,000 here (measured: 0).  RTK_FAST_OCCLUDERS=0 keeps the loop: the reference's
    ray count again.  The _deep cases also send the fast accels' levels through the per-lane walk (RTK_STREAM_DEEP_LEVEL / _MODE),
    which must step over the occlusion tree's empty leaves."""
    import torch

    name, path, kw, deep = case
    sc = rtk.parse_scene_file(path)
    st = torch.cuda.current_stream().cuda_stream

    def frame(acc):
        cfg = rtk.RenderConfig(trace_mode=6, **kw)
        out = torch.empty((kw["height"], kw["width"], 3), dtype=torch.float32, device="cuda")
        acc.render_frame_device(cfg, out.data_ptr(), st)
        torch.cuda.synchronize()
        return out, acc.last_counters()["rays"]

    ref, ref_rays = frame(rtk.KdTreeSimdAccel(sc))
    if deep is not None:                                                      # levels from deep[0] on: per lane (mode 1) or AUTO (0)
        monkeypatch.setenv("RTK_STREAM_DEEP_LEVEL", str(deep[0]))
        monkeypatch.setenv("RTK_STREAM_DEEP_MODE", str(deep[1]))
    fast, fast_rays = frame(rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST))
    assert fast_rays < ref_rays                                               # queries through the glass no longer cost a ray per surface
    differing = int((fast != ref).any(dim=2).sum())
    assert differing <= kw["width"] * kw["height"] // 10_000, differing
    monkeypatch.setenv("RTK_FAST_OCCLUDERS", "0")
    loop, loop_rays = frame(rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST))
    assert loop_rays == ref_rays
    assert int((loop != ref).any(dim=2).sum()) <= kw["width"] * kw["height"] // 10_000
