"""rtk_accel_set_camera and rtk_render_views[_device] on the GPU against the CPU oracle.  The oracle renders the scene with
cam_pos / cam_mat replaced (views_checks.py); every pixel of every frame and view is compared by its bits, `rays` and `primary` as
counts.  Cameras are finite: A the scene's own, B orbited 40 degrees and raised, C looking straight away."""
import numpy as np
import pytest

from conftest import SCENE2, SCENE5, SCENE8
from views_checks import Oracle, bits, same, with_camera

pytestmark = pytest.mark.gpu

_ORACLES = {}
_SCENES = {}


def _oracle(ora, path):
    if path not in _ORACLES:
        _ORACLES[path] = Oracle(ora, path)
    return _ORACLES[path]


def _scene(rtk, path):
    if path not in _SCENES:
        _SCENES[path] = rtk.parse_scene_file(path)
    return _SCENES[path]


def _modes(rtk):
    return {"auto": rtk.TRACE_AUTO, "lane": rtk.TRACE_LANE, "wave": rtk.TRACE_WAVE, "group4": rtk.TRACE_GROUP4,
            "group8": rtk.TRACE_GROUP8, "group16": rtk.TRACE_GROUP16, "stream": rtk.TRACE_STREAM, "twopass": rtk.TRACE_TWOPASS}


def _set(acc, cam):
    acc.set_camera(cam[:3], cam[3:])


def _check_views(o, rgb, cn, names, w, h, what, spp=1, depth=5, gi=0):
    rays = 0
    for v, name in enumerate(names):
        ref, ocn = o.frame(name, w, h, spp, depth, gi)
        bad = int((bits(rgb[v]) != bits(ref)).any(axis=-1).sum())
        assert bad == 0, (what, v, name, bad)
        rays += ocn["rays"]
    assert cn["rays"] == rays, (what, cn["rays"], rays)
    assert cn["primary"] == len(names) * w * h * spp, what


# ---------------------------------------------------------------- 1. set_camera on one accel, every frame engine

@pytest.mark.parametrize("mode", ["auto", "lane", "wave", "group4", "group8", "group16", "stream", "twopass"])
def test_set_camera_every_engine(rtk, ora, mode):
    o = _oracle(ora, SCENE5)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    for w, h in ((200, 120), (70, 45)):                          # ragged blocks and a ragged bucket
        cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
        for name in "ABCA":
            _set(acc, o.cams[name])
            ref, ocn = o.frame(name, w, h)
            for rep in range(3):                                 # from the second on, the previous camera's order and packed workgroups
                rgb, cn = acc.render_frame(cfg)
                assert same(rgb, ref), (mode, w, h, name, rep)
                assert (cn["rays"], cn["primary"]) == (ocn["rays"], w * h), (mode, w, h, name, rep)
    assert not same(o.frame("A", 200, 120)[0], o.frame("B", 200, 120)[0])
    assert not same(o.frame("B", 200, 120)[0], o.frame("C", 200, 120)[0])


# ---------------------------------------------------------------- 2. set_camera with the other calls

def test_set_camera_camera_rays_and_radiance(rtk, ora):
    o = _oracle(ora, SCENE5)
    w, h = 96, 54
    cfg = rtk.RenderConfig(width=w, height=h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    _set(acc, o.cams["B"])
    rays = acc.camera_rays(cfg)
    flat_b = with_camera(o.flat, o.cams["B"])
    from update_checks import _rtk_scene
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat_b))
    assert same(rays, fresh.camera_rays(cfg))
    assert same(rays, o.accel("B").camera_rays(w, h))
    ref, ocn = o.frame("B", w, h)
    rgb, cn = acc.radiance(rays.reshape(-1, 6))
    assert same(rgb.reshape(h, w, 3), ref) and cn["rays"] == ocn["rays"]
    # the tree and the batched intersect do not depend on the camera
    for x, y in zip(acc.tree_dump(), fresh.tree_dump()):
        assert x.tobytes() == y.tobytes()


def test_set_camera_survives_update_vertices(rtk, ora):
    from test_gpu_update import _twist
    o = _oracle(ora, SCENE5)
    w, h = 96, 54
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    _set(acc, o.cams["B"])
    v = _twist(o.flat, 0.5)
    acc.update_vertices(v)
    oacc = ora.Accel(ora.Scene(with_camera(o.flat, o.cams["B"], v)), ora.ACCEL_KD_SIMD)
    ref, ocn = oacc.render(w, h, 1, 5, 0)
    for rep in range(2):
        rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h))
        assert same(rgb, ref) and cn["rays"] == ocn["rays"], rep
    pos, mat = acc.camera()
    assert np.concatenate([pos, mat]).tobytes() == o.cams["B"].tobytes()


def test_set_camera_sharded_frame(rtk, ora):
    import torch
    o = _oracle(ora, SCENE5)
    w, h, world = 200, 120, 3
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    _set(acc, o.cams["B"])
    ref, ocn = o.frame("B", w, h)
    cfgs = [rtk.RenderConfig(width=w, height=h, rank=r, world_size=world) for r in range(world)]
    gathered = torch.full((world, acc.output_floats(cfgs[0])), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rays = 0
    for r in range(world):
        acc.render_frame_device(cfgs[r], gathered[r].data_ptr(), stream)
        rays += acc.last_counters()["rays"]
    acc.assemble_device(cfgs[0], gathered.data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), ref) and rays == ocn["rays"]


# ---------------------------------------------------------------- 3. set_camera on forking scenes

@pytest.mark.parametrize("scene,w,h,spp,depth,gi", [(SCENE8, 160, 90, 2, 10, 0), (SCENE2, 96, 96, 2, 4, 1)], ids=["scene8", "hw15_scene2"])
def test_set_camera_forking_scene_auto(rtk, ora, scene, w, h, spp, depth, gi):
    o = _oracle(ora, scene)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, scene))
    cfg = rtk.RenderConfig(width=w, height=h, spp=spp, max_ray_depth=depth, diffuse_rays=gi)
    rgb, _ = acc.render_frame(cfg)                               # the engine trial starts under the scene's own camera
    assert same(rgb, o.frame("A", w, h, spp, depth, gi)[0])
    _set(acc, o.cams["B"])
    ref, ocn = o.frame("B", w, h, spp, depth, gi)
    for rep in range(5):                                         # ... and runs through its states under B
        rgb, cn = acc.render_frame(cfg)
        assert same(rgb, ref), rep
        assert cn["rays"] == ocn["rays"], rep


# ---------------------------------------------------------------- 4. render_views, one launch

def _alternating(k):
    return [("B", "C", "A", "C")[i % 4] for i in range(k)]


@pytest.mark.parametrize("shape", [(8, 8, 1), (8, 8, 33), (9, 7, 5), (70, 45, 2), (200, 120, 5)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("mode", ["auto", "group4", "group8", "group16"])
def test_render_views_one_launch(rtk, ora, monkeypatch, mode, shape):
    w, h, k = shape
    o = _oracle(ora, SCENE5)
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    names = _alternating(k)
    views = o.views(names)
    # resort every call: the prior's order, then the cost order with the workgroup count unknown, then with it known
    monkeypatch.setenv("RTK_COST_RESORT_EVERY", "1")
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    monkeypatch.delenv("RTK_COST_RESORT_EVERY")
    for rep in range(4):
        rgb, cn = acc.render_views(cfg, views)
        _check_views(o, rgb, cn, names, w, h, (mode, shape, "resort", rep))
    # another view count and back, then the same count with other cameras
    small = names[:2] if k > 2 else names + ["A"]
    for step, ns in enumerate((small, names, names[1:] + names[:1], ["A"] * k)):
        rgb, cn = acc.render_views(cfg, o.views(ns))
        _check_views(o, rgb, cn, ns, w, h, (mode, shape, "then", step))
    default = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    for rep in range(3):
        rgb, cn = default.render_views(cfg, views)
        _check_views(o, rgb, cn, names, w, h, (mode, shape, "default", rep))
    pos, mat = default.camera()
    assert np.concatenate([pos, mat]).tobytes() == o.cams["A"].tobytes()


@pytest.mark.parametrize("mode", ["auto", "group4", "group8"])
def test_render_views_cut_into_launches(rtk, ora, monkeypatch, mode):
    """RTK_VIEWS_LAUNCH_UNITS = 150 against 64 blocks per 9x7 view: five views are launches of 2, 2 and 1 views, each with its own
    order tables, output and view-table offsets, and the counters folded on the device."""
    o = _oracle(ora, SCENE5)
    w, h = 9, 7
    monkeypatch.setenv("RTK_VIEWS_LAUNCH_UNITS", "150")
    monkeypatch.setenv("RTK_COST_RESORT_EVERY", "1")
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    monkeypatch.delenv("RTK_VIEWS_LAUNCH_UNITS")
    monkeypatch.delenv("RTK_COST_RESORT_EVERY")
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    for names in (_alternating(5), _alternating(5), _alternating(5), ["A", "B"], _alternating(7), ["C", "B", "A", "B", "C"]):
        rgb, cn = acc.render_views(cfg, o.views(names))
        _check_views(o, rgb, cn, names, w, h, (mode, names))
    big = rtk.RenderConfig(width=70, height=45, trace_mode=_modes(rtk)[mode])       # 128 blocks per view: one view per launch
    for rep in range(3):
        rgb, cn = acc.render_views(big, o.views(["B", "C", "A"]))
        _check_views(o, rgb, cn, ["B", "C", "A"], 70, 45, (mode, "one per launch", rep))


def test_render_views_one_launch_general_kernel(rtk, ora):
    """An explicit GROUP mode on a scene whose ray trees fork: one launch of the general (refraction) build of the kernel."""
    o = _oracle(ora, SCENE8)
    w, h, depth = 96, 54, 6
    names = ["B", "C", "A", "C", "B"]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE8))
    for mode in ("group4", "group8"):
        cfg = rtk.RenderConfig(width=w, height=h, max_ray_depth=depth, trace_mode=_modes(rtk)[mode])
        for rep in range(3):
            rgb, cn = acc.render_views(cfg, o.views(names))
            _check_views(o, rgb, cn, names, w, h, (mode, rep), depth=depth)


# ---------------------------------------------------------------- 5. RNG keys and passes

@pytest.mark.parametrize("mode", ["auto", "stream"])             # one launch, and view after view
def test_views_keys_and_passes(rtk, ora, mode):
    import torch
    o = _oracle(ora, SCENE5)
    w, h, spp = 70, 45, 4
    names = ["B", "B", "A"]
    views = o.views(names)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    tm = _modes(rtk)[mode]
    whole = rtk.RenderConfig(width=w, height=h, spp=spp, trace_mode=tm)
    for rep in range(2):
        rgb, cn = acc.render_views(whole, views)
        assert same(rgb[0], rgb[1]), rep                         # equal cameras, equal views: the key is the pixel inside the view
        _check_views(o, rgb, cn, names, w, h, (mode, rep), spp=spp)
    passes = [rtk.RenderConfig(width=w, height=h, spp=spp, trace_mode=tm, sample_begin=b, sample_count=2) for b in (0, 2)]
    buf, rays = None, 0
    for p in passes:
        buf, cn = acc.render_views(p, views, buf)
        assert cn["primary"] == 3 * w * h * 2
        rays += cn["rays"]
    assert same(buf, rgb) and rays == sum(o.frame(n, w, h, spp)[1]["rays"] for n in names)
    d_views = torch.from_numpy(views).cuda()
    d_out = torch.full((3, h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rays = 0
    for p in passes:
        acc.render_views_device(p, d_views.data_ptr(), 3, d_out.data_ptr(), stream)
        rays += acc.last_counters()["rays"]
    torch.cuda.synchronize()
    assert same(d_out.cpu().numpy(), rgb) and rays == sum(o.frame(n, w, h, spp)[1]["rays"] for n in names)


# ---------------------------------------------------------------- 6. view after view

@pytest.mark.parametrize("mode,stats", [("lane", 0), ("wave", 0), ("stream", 0), ("twopass", 0), ("auto", 1), ("group4", 2)])
def test_views_fallback_engines(rtk, ora, mode, stats):
    o = _oracle(ora, SCENE5)
    w, h = 96, 54
    names = ["B", "C", "A"]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode], collect_stats=stats)
    for rep in range(2):
        rgb, cn = acc.render_views(cfg, o.views(names))
        _check_views(o, rgb, cn, names, w, h, (mode, stats, rep))
    if stats:
        total = {}
        for n in names:
            _set(acc, o.cams[n])
            one, c1 = acc.render_frame(cfg)
            assert same(one, o.frame(n, w, h)[0])
            for f, x in c1.items():
                total[f] = total.get(f, 0) + x
        assert cn == total and cn["nodes"] > 0 and cn["tris"] > 0


@pytest.mark.parametrize("scene,w,h,spp,depth,gi", [(SCENE8, 96, 54, 1, 6, 0), (SCENE2, 64, 48, 1, 4, 1)], ids=["scene8", "hw15_scene2"])
def test_views_fallback_forking_scenes(rtk, ora, scene, w, h, spp, depth, gi):
    o = _oracle(ora, scene)
    names = ["B", "C", "A"]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, scene))
    cfg = rtk.RenderConfig(width=w, height=h, spp=spp, max_ray_depth=depth, diffuse_rays=gi)
    for rep in range(3):                                         # (the engine trial moves on with every view)
        rgb, cn = acc.render_views(cfg, o.views(names))
        _check_views(o, rgb, cn, names, w, h, (rep,), spp=spp, depth=depth, gi=gi)


# ---------------------------------------------------------------- 7. the device variant

def test_views_device_variant(rtk, ora):
    import torch
    o = _oracle(ora, SCENE5)
    w, h = 70, 45
    names = ["B", "C", "A", "C", "B"]
    k, guard = len(names), 64
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    _set(acc, o.cams["B"])                                       # the accel's own camera: not one the call may change
    cfg = rtk.RenderConfig(width=w, height=h)
    d_views = torch.from_numpy(o.views(names)).cuda()
    n = k * h * w * 3
    side = torch.cuda.Stream()
    for rep in range(3):
        buf = torch.full((n + guard,), float("nan"), dtype=torch.float32, device="cuda")
        buf[n:] = -7.0
        side.wait_stream(torch.cuda.current_stream())
        acc.render_views_device(cfg, d_views.data_ptr(), k, buf.data_ptr(), side.cuda_stream)
        cn = acc.last_counters()                                 # (synchronises the stream the call ran on)
        side.synchronize()
        got = buf.cpu().numpy()
        assert not np.isnan(got[:n]).any() and (got[n:] == -7.0).all(), rep
        _check_views(o, got[:n].reshape(k, h, w, 3), cn, names, w, h, ("device", rep))
        pos, mat = acc.camera()
        assert np.concatenate([pos, mat]).tobytes() == o.cams["B"].tobytes()
        # an ordinary frame of the same size right after: its own order tables, the accel's own camera
        rgb, c1 = acc.render_frame(cfg)
        ref, ocn = o.frame("B", w, h)
        assert same(rgb, ref) and c1["rays"] == ocn["rays"] and c1["primary"] == w * h, rep


# ---------------------------------------------------------------- 8. RTK_TRAVERSAL_FAST (not the parity mode): views == set_camera + frame

def test_views_fast_traversal_accel(rtk, ora, monkeypatch):
    o = _oracle(ora, SCENE8)
    w, h = 96, 54
    names = ["B", "C", "A"]
    # AUTO's engine trial off: the views and the frames compared with them then go through the same engine (the pipeline), and
    # `rays` is comparable (on a FAST accel with transmissive materials the two engines count occlusion queries differently)
    monkeypatch.setenv("RTK_AUTO_TRIALS", "0")
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE8), traversal=rtk.TRAVERSAL_FAST)
    monkeypatch.delenv("RTK_AUTO_TRIALS")
    for mode in ("auto", "group4"):                              # view after view (the scene forks), and one launch of the general kernel
        cfg = rtk.RenderConfig(width=w, height=h, max_ray_depth=6, trace_mode=_modes(rtk)[mode])
        rgb, cn = acc.render_views(cfg, o.views(names))
        rays = 0
        for v, name in enumerate(names):
            _set(acc, o.cams[name])
            one, c1 = acc.render_frame(cfg)
            assert same(rgb[v], one), (mode, v)
            rays += c1["rays"]
        assert cn["rays"] == rays and cn["primary"] == 3 * w * h, mode
