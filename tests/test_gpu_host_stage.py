"""The host variants of the C-ABI share one staging buffer per accel (csrc/stage_plan.hpp, HostStage in csrc/accel.hpp).  One accel
makes every host call that stages through it, one after another and then in reverse order, at image sizes 37x19, 5x3 and 70x36 and
ray counts 1, 63, 65 and 2520, so that the buffer grows, is reused while larger than needed, and grows again, with another call's
planes in it every time.  Every result and every counter must equal, bit for bit, the same call on a fresh accel that has made no
other call.  rtk_denoise_frame and rtk_temporal_accumulate take no accel and stage in a buffer of their own: they are compared with
their _device variants on torch buffers, with each optional plane absent in turn.  (That every staged plane begins at a multiple of
the alignment is tests/cpp/stage_plan_check.cpp's: the buffer's base is hipMalloc's.)"""
import dataclasses

import numpy as np
import pytest

import denoise_model as dm
import temporal_model as tm
from small_scenes import two_quad_scene
from update_checks import _rtk_scene

pytestmark = pytest.mark.gpu

SIZES = ((37, 19), (5, 3), (70, 36))
RAY_COUNTS = (1, 63, 65, 70 * 36)
DEPTH = 3
VIEWS = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], [0.5, 0.25, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1]], np.float32)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _flatten(x):
    """the arrays and numbers of a result, in order"""
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in _flatten(x[k])]
    if isinstance(x, (tuple, list)):
        return [v for e in x for v in _flatten(e)]
    return [x]


def _same(got, want):
    g, w = _flatten(got), _flatten(want)
    return len(g) == len(w) and all(
        (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_words(a), _words(b))) if isinstance(a, np.ndarray) else a == b
        for a, b in zip(g, w))


def _rects(w, h):
    return np.array([[0, 0, w // 2, h // 2], [w // 2, h // 2, w, h]], np.int32)


def _two_passes(render, cfg):
    """a progressive render of two samples in two calls, the second into the buffer of the first -> both results with their counters"""
    first, c1 = render(dataclasses.replace(cfg, spp=2, sample_begin=0, sample_count=1), None)
    buf = first[0].base if isinstance(first, list) else first          # (packed regions come back as views into one array)
    kept = buf.copy()
    second, c2 = render(dataclasses.replace(cfg, spp=2, sample_begin=1, sample_count=1), buf)
    return kept, c1, second, c2


def _image_calls(rtk):
    """name -> call(accel, w, h): the host variants that take an image size"""
    cfg = lambda w, h, **kw: rtk.RenderConfig(width=w, height=h, max_ray_depth=DEPTH, **kw)
    return {
        "gbuffer": lambda a, w, h: a.render_gbuffer(cfg(w, h), views=VIEWS),
        "frame_noise": lambda a, w, h: a.render_frame_noise(cfg(w, h, spp=2)),
        "adaptive": lambda a, w, h: a.render_adaptive(cfg(w, h, spp=2), rtk.AdaptiveConfig(min_samples=2, step=1)),
        "views": lambda a, w, h: _two_passes(lambda c, rgb: a.render_views(c, VIEWS, rgb), cfg(w, h)),
        "regions_in_frame": lambda a, w, h: _two_passes(
            lambda c, rgb: a.render_regions(c, _rects(w, h), rtk.REGIONS_IN_FRAME, rgb), cfg(w, h)),
        "regions_packed": lambda a, w, h: _two_passes(
            lambda c, rgb: a.render_regions(c, _rects(w, h), rtk.REGIONS_PACKED, rgb), cfg(w, h)),
        "camera_rays": lambda a, w, h: a.camera_rays(cfg(w, h)),
        "frame": lambda a, w, h: a.render_frame(cfg(w, h)),
    }


def _ray_calls(rtk, rays):
    """name -> call(accel, n): the host variants that take rays"""
    rcfg = rtk.RadianceConfig(max_ray_depth=DEPTH)
    ids = lambda n: (np.arange(n, dtype=np.uint32) * 7 + 3)
    return {
        "occluded": lambda a, n: a.occluded(rays[:n], np.full(n, 10.0, np.float32), count=True),
        "radiance": lambda a, n: a.radiance(rays[:n], None, rcfg),
        "radiance_ids": lambda a, n: a.radiance(rays[:n], ids(n), rcfg),
        "intersect": lambda a, n: a.intersect(rays[:n], True),
    }


def test_one_accel_through_every_host_variant_equals_fresh_accels(rtk, ora):
    flat = two_quad_scene(ora)
    accel = lambda: rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    rays = accel().camera_rays(rtk.RenderConfig(width=70, height=36)).reshape(-1, 6)
    assert rays.shape[0] == RAY_COUNTS[-1]
    image, batch = _image_calls(rtk), _ray_calls(rtk, rays)
    # the sequence: at every image size all image calls, then all ray calls at the ray count of the same position
    steps = []
    for i, (w, h) in enumerate(SIZES):
        steps += [(name, (w, h)) for name in image]
        steps += [(name, (RAY_COUNTS[i],)) for name in batch]
    steps += [(name, (RAY_COUNTS[3],)) for name in batch]
    calls = dict(image, **batch)
    fresh = {step: calls[step[0]](accel(), *step[1]) for step in steps}
    live = accel()
    for i, step in enumerate(steps + steps[::-1]):
        got = calls[step[0]](live, *step[1])
        assert _same(got, fresh[step]), (i, step)
    # (the cases show something: hits and misses, lit and shadowed, more than one colour)
    big = fresh[("gbuffer", (70, 36))]
    assert 0 < int((big["depth"] >= 0).sum()) < big["depth"].size
    occ, n_int = fresh[("occluded", (2520,))]
    assert 0 < int(occ.sum()) < 2520 and n_int > 0
    rgb, counters = fresh[("frame", (37, 19))]
    assert len(np.unique(_words(rgb).reshape(-1, 12), axis=0)) > 8 and counters["rays"] > counters["primary"] == 37 * 19


# ---------------------------------------------------------------- the calls without an accel: host against device variant

def _up(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("absent", ["nothing", "noise", "albedo"])
@pytest.mark.parametrize("w,h", [(37, 19), (5, 3)])
def test_denoise_host_variant_equals_the_device_variant(rtk, w, h, absent):
    import torch
    planes = dm.synthetic(w, h, 0)
    cfg = rtk.DenoiseConfig(**dict(dm.PARAMS, iterations=dm.ITERATIONS[(w, h)]))
    noise = None if absent == "noise" else planes["noise"]
    albedo = None if absent == "albedo" else planes["albedo"]
    host = rtk.denoise(planes["rgb"], planes["normal"], planes["position"], planes["depth"], noise, albedo, cfg)
    d = {k: _up(a) for k, a in dict(rgb=planes["rgb"], normal=planes["normal"], position=planes["position"], depth=planes["depth"],
                                    noise=noise, albedo=albedo).items()}
    need = rtk.denoise_workspace_bytes(w, h, 1, cfg)
    ws = torch.zeros(need // 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    rtk.denoise_device(w, h, _ptr(d["rgb"]), _ptr(d["normal"]), _ptr(d["position"]), _ptr(d["depth"]), out.data_ptr(), ws.data_ptr(), need,
                       d_noise_ptr=_ptr(d["noise"]), d_albedo_ptr=_ptr(d["albedo"]), cfg=cfg, stream=s.cuda_stream)
    s.synchronize()
    device = out.cpu().numpy().reshape(h, w, 3)
    assert np.array_equal(dm.bits(host), dm.bits(device))
    assert (dm.bits(host) != dm.bits(planes["rgb"])).any() or (w, h) == (5, 3)


@pytest.mark.parametrize("absent", ["nothing", "noise", "mesh", "history"])
@pytest.mark.parametrize("w,h", [(37, 19), (5, 3)])
def test_temporal_host_variant_equals_the_device_variant(rtk, w, h, absent):
    import torch
    cur, prev = tm.synthetic_pair(w, h)
    optional = [k for k in ("noise", "mesh") if k != absent]
    pick = lambda f, extra: {k: f[k] for k in ["rgb", "position", "normal", "depth"] + extra + optional}
    c, q = pick(cur, []), None if absent == "history" else dict(pick(prev, ["length"]), view=prev["view"])
    cfg = rtk.TemporalConfig(**tm.PARAMS)
    host = rtk.temporal_accumulate(c, q, cfg)
    dc = {k: _up(a) for k, a in c.items()}
    dq = None if q is None else {k: _up(a) for k, a in q.items() if k != "view"}
    outs = {k: torch.zeros(n, dtype=torch.float32, device="cuda")
            for k, n in dict(rgb=3 * w * h, length=w * h, **(dict(noise=w * h) if "noise" in optional else {})).items()}
    prev_ptrs = None if dq is None else dict({k: t.data_ptr() for k, t in dq.items()}, view=q["view"])
    s = torch.cuda.current_stream()
    rtk.temporal_accumulate_device(w, h, {k: t.data_ptr() for k, t in dc.items()}, prev_ptrs, {k: t.data_ptr() for k, t in outs.items()},
                                   cfg=cfg, stream=s.cuda_stream)
    s.synchronize()
    assert (host["noise"] is None) == ("noise" not in optional)
    for k, t in outs.items():
        assert np.array_equal(tm.bits(host[k]), tm.bits(t.cpu().numpy().reshape(host[k].shape))), k
