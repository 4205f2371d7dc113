"""rtk_render_gbuffer_specular[_device] on the GPU, on the generated 48 x 32 material scenes (tests/material_scenes.py: facing
mirrors whose chains run to the depth limit, a flat glass box around a smooth glass octahedron, total internal reflection on entry
and on exit, iors of 0 and below, a constant quad, textures).  The comparison side is tests/specular_model.py: the contract of
rtk.h in numpy float32 over the CPU oracle's hits.  Every plane is compared by its bits (a NaN only has to meet a NaN)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import material_scenes as ms
import specular_model as sm
from scene_state_checks import DIFFUSE, set_materials, with_material
from views_checks import with_camera

pytestmark = pytest.mark.gpu

W, H = ms.SIZE
N = W * H
MISS = sm.MISS
SENTINEL = 0xA5C3F00D
GUARD = 16                                     # dwords (64 bytes) in front of and behind every plane
DEPTHS = (1, 5, 16)
# looks at the mirror behind the scene's camera from close by: the constant quad shows in it (72 pixels at depth 5)
MIRROR_VIEW = np.array([4, -0.75, 8, -1, 0, 0, 0, 1, 0, 0, 0, -1], np.float32)
_cache = {}


def _flat(ora, variant):
    if ("flat", variant) not in _cache:
        _cache["flat", variant] = ms.make_scene(ora, variant)
    return _cache["flat", variant]


def _accel(rtk, ora, variant, **kw):
    key = ("acc", variant, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, _flat(ora, variant)), **kw)
    return _cache[key]


def _model(ora, flat, depth, cam=None, w=W, h=H, spp=1, sample=0, key=None):
    """the model's planes of one view, computed once per (scene, camera, depth, size, sample) and left unchanged"""
    k = ("model", key, None if cam is None else cam.tobytes(), depth, w, h, spp, sample)
    if key is None or k not in _cache:
        f = flat if cam is None else with_camera(flat, cam)
        m = sm.camera_planes(ora.Accel(ora.Scene(f), ora.ACCEL_KD_SIMD), f, w, h, depth, spp=spp, sample=sample)
        for a in m.values():
            a.setflags(write=False)
        if key is None:
            return m
        _cache[k] = m
    return _cache[k]


def _check(got, v, m, what, planes=sm.PLANES):
    """view v of the planes `got` ([K, h, w(, c)]) against the model's flattened planes"""
    for name in planes:
        g = got[name][v].reshape(m[name].shape)
        print(what, name, "differing pixels", int((sm.u32(g) != sm.u32(m[name])).reshape(len(g), -1).any(axis=1).sum()))
        assert g.dtype == m[name].dtype and sm.same_bits(g, m[name]), (what, v, name)


def _diffuse(flat):
    """the scene with the mirror and both glass materials turned diffuse"""
    for mat in (ms.M_MIRROR, ms.M_OUTER, ms.M_INNER):
        flat = with_material(flat, mat, kind=DIFFUSE)
    return flat


# ---------------------------------------------------------------- 1. model parity

@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_every_plane_is_the_models(rtk, ora, variant, depth):
    m = _model(ora, _flat(ora, variant), depth, key=variant)
    got = _accel(rtk, ora, variant).render_gbuffer_specular(rtk.RenderConfig(width=W, height=H, spp=1, max_ray_depth=depth))
    assert set(got) == set(sm.PLANES)
    _check(got, 0, m, (variant, depth))
    # the scene is what the module says it is: chains of every kind, some to the limit
    assert m["surface"].sum() > 500
    if depth > 1:
        assert (m["bounces"] > 1).sum() > 100 and (m["refractions"] > 0).sum() > 50 and (m["tirs"] > 0).sum() > 5
    if variant == "ior15_075":
        assert (m["bounces"] == depth).sum() >= 2


# ---------------------------------------------------------------- 2. nothing specular

def test_without_specular_materials_it_is_the_gbuffer(rtk, ora):
    flat = _diffuse(_flat(ora, "ior15_075"))
    acc = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, _flat(ora, "ior15_075")))
    set_materials(acc, flat)
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=5)
    got, gb = acc.render_gbuffer_specular(cfg), acc.render_gbuffer(cfg)
    assert not got["bounces"].any() and (gb["tri"] != MISS).sum() > 1000
    for name in sm.SHARED:
        assert got[name].tobytes() == gb[name].tobytes(), name
    assert got["position"].tobytes() == got["surface_position"].tobytes()           # negative zeros included
    assert got["normal"].tobytes() == got["surface_normal"].tobytes()
    assert got["last_ray"][0].tobytes() == np.ascontiguousarray(acc.camera_rays(cfg, 0)).tobytes()
    _check(got, 0, _model(ora, flat, 5), "diffuse")


# ---------------------------------------------------------------- 3. through the public queries

@pytest.mark.parametrize("depth", (5, 16))
def test_last_ray_reproduces_the_end_hit(rtk, ora, depth):
    acc = _accel(rtk, ora, "ior15_075")
    got = acc.render_gbuffer_specular(rtk.RenderConfig(width=W, height=H, max_ray_depth=depth))
    rays = np.ascontiguousarray(got["last_ray"][0].reshape(N, 6))
    k = got["bounces"][0].reshape(N)
    surface = got["tri"][0].reshape(N) != MISS
    assert (surface & (k > 0)).sum() > 300 and (~surface & (k < depth)).sum() > 50
    for cull in (True, False):
        sel = (k == 0) == cull
        hits = acc.intersect(rays[sel], cull)
        s = surface[sel]
        on = lambda name, c: got[name][0].reshape(N, c)[sel][s]                       # noqa: E731
        assert np.array_equal(hits["tri"][s], on("tri", 1)[:, 0]) and np.array_equal(hits["mesh"][s], on("mesh", 1)[:, 0])
        assert np.stack([hits["u"], hits["v"]], axis=1)[s].tobytes() == on("bary", 2).tobytes()
        assert np.ascontiguousarray(hits["normal"][s]).tobytes() == on("surface_normal", 3).tobytes()
        r, t = rays[sel][s], hits["t"][s]
        pos = (r[:, 0:3] + (t[:, None] * r[:, 3:6]).astype(np.float32)).astype(np.float32)
        assert pos.tobytes() == on("surface_position", 3).tobytes()
        # NO SURFACE before the depth limit: the last ray found nothing
        short = ~s & (k[sel] < depth)
        assert (hits["tri"][short] == MISS).all()


# ---------------------------------------------------------------- 4. against the frame, pinned to the reference

@pytest.mark.parametrize("depth", (5, 16))
def test_mirror_chains_to_constant_or_nothing_are_the_frames_pixels(rtk, ora, depth):
    """Chains of reflections alone that end on the constant quad or on no surface: color_hit returns the constant's albedo
    (render.hpp:302-303) or the background, through any number of mirrors unchanged (:239-250) -- the frame's pixel IS the albedo
    plane.  The pixels are the model's; the default camera reaches the quad directly only, MIRROR_VIEW through the front mirror."""
    flat = _flat(ora, "ior15_075")
    acc = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, flat))
    cfg = rtk.RenderConfig(width=W, height=H, spp=1, max_ray_depth=depth)
    seen = {"constant": 0, "nothing": 0}
    for cam in (None, MIRROR_VIEW):
        f = flat if cam is None else with_camera(flat, cam)
        m = _model(ora, flat, depth, cam=cam, key="ior15_075")
        pure = (m["refractions"] == 0) & (m["tirs"] == 0)
        constant = pure & m["surface"] & (m["end_kind"] == sm.CONSTANT) & (m["bounces"] > 0)
        nothing = pure & ~m["surface"]
        if cam is not None:
            acc.set_camera(cam[:3], cam[3:])
            assert constant.sum() >= 16 and nothing.sum() >= 16, (int(constant.sum()), int(nothing.sum()))
        sel = constant | nothing | (pure & m["surface"] & (m["end_kind"] == sm.CONSTANT))
        got = acc.render_gbuffer_specular(cfg, planes=("albedo", "bounces"))
        frame = acc.render_frame(cfg)[0].reshape(N, 3)
        ref = ora.Accel(ora.Scene(f), ora.ACCEL_KD_SIMD).render(W, H, 1, depth, 0)[0].reshape(N, 3)
        alb = got["albedo"][0].reshape(N, 3)
        assert frame[sel].tobytes() == alb[sel].tobytes() and ref[sel].tobytes() == alb[sel].tobytes()
        assert np.array_equal(got["bounces"][0].reshape(N), m["bounces"])
        seen["constant"] += int(constant.sum())
        seen["nothing"] += int(nothing.sum())
    assert seen["constant"] >= 16 and seen["nothing"] >= 16, seen


# ---------------------------------------------------------------- 5. shapes and masks

def _guarded(k, h, w, names):
    bufs, views = {}, {}
    for name in names:
        n = k * h * w * sm.COMPS[name]
        raw = np.full(GUARD + n + GUARD, SENTINEL, np.uint32)
        bufs[name] = raw
        body = raw[GUARD:GUARD + n]
        views[name] = (body.view(np.float32) if name in sm.FLOAT_PLANES else body).reshape((k, h, w) + ((sm.COMPS[name],) if sm.COMPS[name] > 1 else ()))
    return bufs, views


def _host_call(rtk, acc, cfg, sample, views, k, wanted):
    """through the C-ABI into guarded buffers: all twelve exist, only `wanted` are in the plane table"""
    bufs, out = _guarded(k, cfg.height, cfg.width, sm.PLANES)
    gb = rtk.SpecularGBuffer(**{n: out[n].ctypes.data for n in wanted})
    p = cfg.to_c()
    vptr = None if views is None else np.ascontiguousarray(views, np.float32).ctypes.data
    rc = rtk.lib().rtk_render_gbuffer_specular(acc._h, ctypes.byref(p), sample, vptr, k, ctypes.byref(gb))
    assert rc == rtk.RTK_OK, rtk.lib().rtk_last_error()
    for n in sm.PLANES:
        assert (bufs[n][:GUARD] == SENTINEL).all() and (bufs[n][-GUARD:] == SENTINEL).all(), n
        if n not in wanted:
            assert (bufs[n] == SENTINEL).all(), n
    return {n: out[n] for n in wanted}


def _device_call(rtk, acc, cfg, sample, views, k, wanted, stream=None):
    """the device variant on a non-default torch stream; every plane starts 4 bytes behind a 16-byte boundary"""
    import torch
    s = stream or torch.cuda.Stream()
    sent = int(np.array(SENTINEL, np.uint32).view(np.int32))
    raws, ptrs, sizes = {}, {}, {}
    for name in sm.PLANES:
        n = k * cfg.height * cfg.width * sm.COMPS[name]
        raw = torch.full((GUARD + 1 + n + GUARD,), sent, dtype=torch.int32, device="cuda")
        raws[name], sizes[name], ptrs[name] = raw, n, raw.data_ptr() + 4 * (GUARD + 1)
        assert ptrs[name] % 16 == 4
    d_views = None
    if views is not None:
        d_views = torch.zeros(1 + k * 12, dtype=torch.float32, device="cuda")
        d_views[1:] = torch.from_numpy(np.ascontiguousarray(views, np.float32).reshape(-1)).cuda()
    torch.cuda.synchronize()
    acc.render_gbuffer_specular_device(cfg, {n: ptrs[n] for n in wanted}, sample=sample,
                                       d_views_ptr=0 if d_views is None else d_views.data_ptr() + 4, n_views=k, stream=s.cuda_stream)
    s.synchronize()
    out = {}
    for name in sm.PLANES:
        raw = raws[name].cpu().numpy().view(np.uint32)
        n = sizes[name]
        assert (raw[:GUARD + 1] == SENTINEL).all() and (raw[GUARD + 1 + n:] == SENTINEL).all(), name
        body = raw[GUARD + 1:GUARD + 1 + n]
        if name not in wanted:
            assert (body == SENTINEL).all(), name
            continue
        out[name] = (body.view(np.float32) if name in sm.FLOAT_PLANES else body).reshape(
            (k, cfg.height, cfg.width) + ((sm.COMPS[name],) if sm.COMPS[name] > 1 else ()))
    return out


def _cams(flat):
    own = np.concatenate([flat.cam_pos, flat.cam_mat]).astype(np.float32)
    side = np.array([-3, 1, 7, 0.8, 0, -0.6, 0, 1, 0, 0.6, 0, 0.8], np.float32)      # turned towards the left mirror
    return [own, MIRROR_VIEW, side]


def test_partial_blocks_views_and_samples(rtk, ora):
    """13 x 9 (partial blocks, two blocks a view: the workgroup straddles the views), three views in one call against set_camera +
    one call each and against the model, and sample 2 of spp = 4 along rtk_camera_rays(.., 2)."""
    flat = _flat(ora, "swapped")
    acc = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, flat))
    cams = _cams(flat)
    w, h = 13, 9
    for spp, sample in ((1, 0), (4, 2)):
        cfg = rtk.RenderConfig(width=w, height=h, spp=spp, max_ray_depth=5)
        got = acc.render_gbuffer_specular(cfg, sample=sample, views=np.stack(cams))
        assert got["depth"].shape == (3, h, w) and got["last_ray"].shape == (3, h, w, 6)
        for v, cam in enumerate(cams):
            m = _model(ora, flat, 5, cam=cam, w=w, h=h, spp=spp, sample=sample)
            _check(got, v, m, ("13x9", spp, sample, v))
            acc.set_camera(cam[:3], cam[3:])
            one = acc.render_gbuffer_specular(cfg, sample=sample)
            for name in sm.PLANES:
                assert one[name][0].tobytes() == got[name][v].tobytes(), (v, name)
            # k == 0 pixels keep the camera ray of that sample
            rays = acc.camera_rays(cfg, sample).reshape(-1, 6)
            first = got["bounces"][v].reshape(-1) == 0
            assert first.sum() >= 8 and got["last_ray"][v].reshape(-1, 6)[first].tobytes() == rays[first].tobytes()
        acc.set_camera(cams[0][:3], cams[0][3:])
    assert _model(ora, flat, 5, cam=cams[0], w=w, h=h, spp=4, sample=2)["depth"].tobytes() != _model(ora, flat, 5, cam=cams[0], w=w, h=h)["depth"].tobytes()


@pytest.mark.parametrize("variant", ["host", "device"])
def test_plane_subsets_and_guards(rtk, ora, variant):
    """Each plane alone holds the bits it has with all twelve; planes not asked for and 64 guard bytes around every plane keep
    their canaries.  The device variant runs on a non-default stream into planes (and views) 4 bytes behind a 16-byte boundary."""
    flat = _flat(ora, "textured")
    acc = _accel(rtk, ora, "textured")
    cams = _cams(flat)[:2]
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=5)
    call = _host_call if variant == "host" else _device_call
    full = call(rtk, acc, cfg, 0, np.stack(cams), 2, sm.PLANES)
    for v, cam in enumerate(cams):
        _check(full, v, _model(ora, flat, 5, cam=cam, key="textured"), (variant, v))
    for name in sm.PLANES:
        got = call(rtk, acc, cfg, 0, np.stack(cams), 2, (name,))
        assert set(got) == {name} and got[name].tobytes() == full[name].tobytes(), name
    own = call(rtk, acc, cfg, 0, None, 1, ("depth", "bounces", "last_ray"))          # views = NULL: the accel's camera
    for name in own:
        assert own[name][0].tobytes() == full[name][0].tobytes(), name


# ---------------------------------------------------------------- 6. live state and side effects

def test_planes_follow_vertices_and_materials(rtk, ora):
    base = _flat(ora, "ior24_10")
    acc = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, base))
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=5)
    before = acc.render_gbuffer_specular(cfg)
    _check(before, 0, _model(ora, base, 5, key="ior24_10"), "built")
    moved = (base.vertices + 0.05 * np.sin(np.arange(base.vertices.size, dtype=np.float32)).reshape(-1, 3)).astype(np.float32)
    s1 = dataclasses.replace(base, vertices=moved)
    acc.update_vertices(moved)
    after = acc.render_gbuffer_specular(cfg)
    _check(after, 0, _model(ora, s1, 5), "update_vertices")
    fresh = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, s1)).render_gbuffer_specular(cfg)
    assert all(after[n].tobytes() == fresh[n].tobytes() for n in sm.PLANES)
    s2 = with_material(with_material(s1, ms.M_MIRROR, kind=DIFFUSE), ms.M_FLOOR, kind=sm.REFLECTIVE)
    set_materials(acc, s2)
    last = acc.render_gbuffer_specular(cfg)
    _check(last, 0, _model(ora, s2, 5), "set_materials")
    assert before["depth"].tobytes() != after["depth"].tobytes() and after["bounces"].tobytes() != last["bounces"].tobytes()


def test_frames_counters_and_camera_are_left_alone(rtk, ora):
    """GROUP4 frame x 3, a host and a device call on a stream of its own, a frame: the last frame is the third's bits and `rays` and
    issues no counter fill, the calls issued none, camera() and rtk_render_last_counters are unchanged."""
    import torch
    from conftest import SCENE5
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    cfg = rtk.RenderConfig(width=320, height=180, trace_mode=rtk.TRACE_GROUP4)
    s = torch.cuda.current_stream()

    def frame():
        buf = torch.full((acc.output_floats(cfg),), float("nan"), dtype=torch.float32, device="cuda")
        before = acc.counter_fills()
        acc.render_frame_device(cfg, buf.data_ptr(), s.cuda_stream)
        cn = acc.last_counters()
        return buf.cpu().numpy(), cn, acc.counter_fills() - before

    frames = [frame() for _ in range(3)]
    assert [f[2] for f in frames] == [1, 1, 0]
    own = [x.copy() for x in acc.camera()]
    fills = acc.counter_fills()
    views = np.stack([MIRROR_VIEW, np.concatenate(own).astype(np.float32)])
    got = acc.render_gbuffer_specular(cfg, views=views)
    d = _device_call(rtk, acc, cfg, 0, views, 2, ("depth", "bounces"))
    assert acc.counter_fills() == fills
    assert all(a.tobytes() == b.tobytes() for a, b in zip(own, acc.camera()))
    assert acc.last_counters() == frames[2][1]
    assert d["depth"].tobytes() == got["depth"].tobytes() and d["bounces"].tobytes() == got["bounces"].tobytes()
    assert (got["bounces"][1] > 0).sum() > 500                                   # scene5's floor is a mirror
    last = frame()
    assert last[2] == 0
    assert last[0].tobytes() == frames[2][0].tobytes() and last[1]["rays"] == frames[2][1]["rays"]


# ---------------------------------------------------------------- 7. RTK_TRAVERSAL_FAST

def test_fast_traversal_keeps_the_depth_of_direct_pixels(rtk, ora):
    """The call succeeds on an RTK_TRAVERSAL_FAST accel; where the model's chain has no bounce, depth has the parity accel's bits.
    Along a chain the tie caveat compounds: nothing more is claimed."""
    m = _model(ora, _flat(ora, "ior15_075"), 5, key="ior15_075")
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=5)
    parity = _accel(rtk, ora, "ior15_075").render_gbuffer_specular(cfg, planes=("depth",))
    fast = _accel(rtk, ora, "ior15_075", traversal=rtk.TRAVERSAL_FAST).render_gbuffer_specular(cfg)
    direct = m["bounces"] == 0
    assert direct.sum() > 500
    assert fast["depth"][0].reshape(N)[direct].tobytes() == parity["depth"][0].reshape(N)[direct].tobytes()
