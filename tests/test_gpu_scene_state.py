"""rtk_accel_set_lights[_device] / _set_materials / _set_background on the GPU.  The comparison side is the CPU oracle on the scene
with the part replaced (scene_state_checks.py): every pixel by its bits, `rays` and `primary` as counts.  For RTK_TRAVERSAL_FAST,
which is not the parity mode, it is a fresh product accel built from the modified scene under the same environment.  Every
sequence asserts that consecutive states really differ, so a call that does nothing cannot pass."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import SCENE2, SCENE5, SCENE8, SCENES
from occlusion_model import camera_hits, occluded_ref, segments, shadow_queries
from scene_state_checks import (DIFFUSE, REFRACTIVE, TEXTURE, TREE, States, light_states, octant_scene, same, scene5_material_states,
                                set_lights, set_materials, with_material)
from update_checks import _rtk_scene
from views_checks import cameras, with_camera

pytestmark = pytest.mark.gpu

SCENE4_TEX = os.path.join(SCENES, "hw12", "scene4.crtscene")
MODES = ["auto", "lane", "wave", "group4", "group8", "group16", "stream", "twopass"]
SHAPES = ((200, 120), (70, 45))                      # ragged blocks and a ragged bucket

_STATES = {}
_FLATS = {}
_SCENES = {}


def _states(ora):
    if "s" not in _STATES:
        _STATES["s"] = States(ora)
    return _STATES["s"]


def _flat(ora, path):
    if path not in _FLATS:
        _FLATS[path] = ora.load_crtscene(path)
    return _FLATS[path]


def _scene(rtk, path):
    if path not in _SCENES:
        _SCENES[path] = rtk.parse_scene_file(path)
    return _SCENES[path]


def _mode(rtk, name):
    return {"auto": rtk.TRACE_AUTO, "lane": rtk.TRACE_LANE, "wave": rtk.TRACE_WAVE, "group4": rtk.TRACE_GROUP4,
            "group8": rtk.TRACE_GROUP8, "group16": rtk.TRACE_GROUP16, "stream": rtk.TRACE_STREAM, "twopass": rtk.TRACE_TWOPASS}[name]


def _frames(rtk, acc, S, key, flat, mode, what, shapes=SHAPES, reps=3, **kw):
    """`reps` frames per shape (the second and third run under the learnt order) against the oracle's frame of state `key`"""
    for w, h in shapes:
        ref, ocn = S.frame(key, flat, w, h, **kw)
        cfg = rtk.RenderConfig(width=w, height=h, spp=kw.get("spp", 1), max_ray_depth=kw.get("depth", 5), diffuse_rays=kw.get("gi", 0),
                               trace_mode=_mode(rtk, mode))
        for rep in range(reps):
            rgb, cn = acc.render_frame(cfg)
            bad = int((rgb.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
            assert bad == 0, (what, mode, w, h, rep, bad)
            assert (cn["rays"], cn["primary"]) == (ocn["rays"], w * h * kw.get("spp", 1)), (what, mode, w, h, rep)


def _differ(S, seq, w=200, h=120, **kw):
    """consecutive states of `seq` [(key, flat)] give different oracle frames"""
    for (ka, fa), (kb, fb) in zip(seq, seq[1:]):
        assert not same(S.frame(ka, fa, w, h, **kw)[0], S.frame(kb, fb, w, h, **kw)[0]), (ka, kb)


# ---------------------------------------------------------------- 1. lights

@pytest.mark.parametrize("mode", MODES)
def test_set_lights_every_engine(rtk, ora, mode):
    S = _states(ora)
    seq = [("L " + n, f) for n, f in light_states(_flat(ora, SCENE5))]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    for i, (key, flat) in enumerate(seq):
        if i > 0:
            set_lights(acc, flat)
        _frames(rtk, acc, S, key, flat, mode, key)
        pos, inten = acc.lights()
        assert pos.tobytes() == flat.light_pos.tobytes() and inten.tobytes() == flat.light_intensity.tobytes()
    _differ(S, seq)


def test_set_lights_radiance_and_views(rtk, ora):
    S = _states(ora)
    base = _flat(ora, SCENE5)
    seq = [("L " + n, f) for n, f in light_states(base)]
    w, h = 96, 54
    cfg = rtk.RenderConfig(width=w, height=h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    rays = acc.camera_rays(cfg).reshape(-1, 6)
    hits = acc.intersect(rays, True)
    for i, (key, flat) in enumerate(seq):                            # the nine-light state makes the stream workspace grow mid-life
        if i > 0:
            set_lights(acc, flat)
        ref, ocn = S.frame(key, flat, w, h)
        rgb, cn = acc.radiance(rays)
        assert same(rgb.reshape(h, w, 3), ref) and cn["rays"] == ocn["rays"], key
    assert acc.intersect(rays, True).tobytes() == hits.tobytes()
    assert same(acc.camera_rays(cfg).reshape(-1, 6), rays)
    # three cameras in one call after a set_lights
    key, flat = seq[2]
    set_lights(acc, flat)
    cams = cameras(base)
    names = ["B", "C", "A"]
    for mode in ("auto", "stream"):
        vcfg = rtk.RenderConfig(width=70, height=45, trace_mode=_mode(rtk, mode))
        for rep in range(2):
            rgb, cn = acc.render_views(vcfg, np.stack([cams[n] for n in names]))
            rays_sum = 0
            for v, n in enumerate(names):
                ref, ocn = S.frame((key, n), with_camera(flat, cams[n]), 70, 45)
                assert same(rgb[v], ref), (mode, rep, n)
                rays_sum += ocn["rays"]
            assert cn["rays"] == rays_sum, (mode, rep)


# ---------------------------------------------------------------- 2. lights from the device

def test_set_lights_device(rtk, ora):
    import torch
    S = _states(ora)
    seq = [("L " + n, f) for n, f in light_states(_flat(ora, SCENE5))]
    w, h = 70, 45
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))                   # not resident yet: the first call puts it on the device
    side = torch.cuda.Stream()
    for step, (key, flat) in enumerate(seq[1:] + seq[:1]):
        tab = np.concatenate([flat.light_pos.reshape(-1, 3), flat.light_intensity.reshape(-1, 1)], axis=1).astype(np.float32)
        d_tab = torch.from_numpy(np.ascontiguousarray(tab)).cuda()
        torch.cuda.current_stream().synchronize()
        acc.set_lights_device(d_tab.data_ptr(), tab.shape[0], torch.cuda.current_stream().cuda_stream)
        # a frame on ANOTHER stream right after the call sees the new lights
        ref, ocn = S.frame(key, flat, w, h)
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        acc.render_frame_device(rtk.RenderConfig(width=w, height=h), out.data_ptr(), side.cuda_stream)
        cn = acc.last_counters()
        side.synchronize()
        assert same(out.cpu().numpy(), ref) and cn["rays"] == ocn["rays"], (key, step)
        pos, inten = acc.lights()
        assert np.concatenate([pos, inten[:, None]], axis=1).astype(np.float32).tobytes() == tab.tobytes(), key
        # ... and the same bytes as the host variant gives
        host = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
        set_lights(host, flat)
        rgb, hcn = host.render_frame(rtk.RenderConfig(width=w, height=h))
        assert same(rgb, out.cpu().numpy()) and hcn["rays"] == cn["rays"], key
        for mode in ("stream", "group4"):
            _frames(rtk, acc, S, key, flat, mode, ("device", key), shapes=((w, h),), reps=2)


# ---------------------------------------------------------------- 3. materials

@pytest.mark.parametrize("mode", MODES)
def test_set_materials_every_engine(rtk, ora, mode):
    """has_refractive goes false -> true -> false on one accel: lean and general kernels, early shadow exit and the unlit skip switch,
    and under auto the engine trial restarts in each direction."""
    S = _states(ora)
    seq = [("M " + n, f) for n, f in scene5_material_states(_flat(ora, SCENE5))]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    dump = acc.tree_dump()
    for i, (key, flat) in enumerate(seq):
        if i > 0:
            set_materials(acc, flat)
        _frames(rtk, acc, S, key, flat, mode, key, reps=4 if mode == "auto" else 3)
    _differ(S, seq)
    for x, y in zip(dump, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()


def test_set_materials_forking_through_gi(rtk, ora):
    """hw15/scene2 with diffuse GI: the scene forks on both sides of the switch of its glass sphere (material 2)."""
    S = _states(ora)
    base = _flat(ora, SCENE2)
    assert base.mat_kind[2] == REFRACTIVE
    seq = [("G own", base), ("G sphere diffuse", with_material(base, 2, kind=DIFFUSE, albedo=[0.6, 0.6, 0.9])), ("G own", base)]
    kw = dict(spp=2, depth=4, gi=2)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE2))
    for mode in ("auto", "stream", "group4"):
        for i, (key, flat) in enumerate(seq):
            set_materials(acc, flat)
            _frames(rtk, acc, S, key, flat, mode, key, shapes=((48, 48),), **kw)
    _differ(S, seq, 48, 48, **kw)


# ---------------------------------------------------------------- 4. batches follow the materials

def test_batches_follow_the_materials(rtk, ora):
    S = _states(ora)
    base = _flat(ora, SCENE5)
    glass = with_material(base, 1, kind=REFRACTIVE, ior=1.5)
    oacc = S.accel("M own", base)                                   # (the tree and the closest hits do not depend on the materials)
    _, _, P = camera_hits(oacc, 64, 48)
    P = P[np.isfinite(P).all(axis=1)]
    q = [shadow_queries(base, P, light)[:2] for light in range(4)]  # shadow segments of what the camera sees: many cross the dragon
    rays = np.concatenate([r for r, _ in q] + [segments(base, 2000, 5)[0]])
    max_t = np.concatenate([t for _, t in q] + [segments(base, 2000, 5)[1]])
    assert 3000 < rays.shape[0] < 20000
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    hits = acc.intersect(rays, False)
    answers = []
    for key, flat in (("own", base), ("glass", glass), ("own", base)):
        set_materials(acc, flat)
        ref, steps, entered = occluded_ref(oacc, flat, rays, max_t, 1e-4, with_entered=True)
        for mode in (rtk.TRACE_AUTO, rtk.TRACE_LANE, rtk.TRACE_WAVE):
            got, n_int = acc.occluded(rays, max_t, 1e-4, mode, count=True)
            assert got.tobytes() == ref.tobytes(), (key, mode)
            assert n_int == int(steps.sum()) + int(entered.sum()), (key, mode)
        answers.append(ref)
        assert acc.intersect(rays, False).tobytes() == hits.tobytes(), key
    assert (answers[0] != answers[1]).sum() > 50 and answers[0].tobytes() == answers[2].tobytes()


# ---------------------------------------------------------------- 5. textures

def test_set_materials_textures(rtk, ora):
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    assert base.mat_kind.tolist() == [TEXTURE] * 4 and base.mat_texture.tolist() == [0, 1, 2, 3]
    swapped = dataclasses.replace(base, mat_texture=np.array([3, 2, 1, 0], np.int32))          # the bitmap moves to material 0
    plain = with_material(swapped, 1, kind=DIFFUSE, albedo=[0.7, 0.2, 0.1])
    again = with_material(plain, 1, kind=TEXTURE, texture=3)                                   # two materials with the bitmap
    seq = [("T own", base), ("T swapped", swapped), ("T one diffuse", plain), ("T texture again", again), ("T own", base)]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    for mode in ("auto", "stream", "lane"):
        for key, flat in seq:
            set_materials(acc, flat)
            _frames(rtk, acc, S, key, flat, mode, key, reps=2)
    assert acc.materials()["texture"].tolist() == [0, 1, 2, 3]
    _differ(S, seq)


# ---------------------------------------------------------------- 6. background

@pytest.mark.parametrize("mode", MODES)
def test_set_background_every_engine(rtk, ora, mode):
    S = _states(ora)
    base = _flat(ora, SCENE5)
    cam = cameras(base)["B"]                                         # orbited and raised: sees sky above the floor's edge
    seen = with_camera(base, cam)
    seq = [("B own", seen), ("B red", dataclasses.replace(seen, background=np.array([0.9, -0.0, 0.25], np.float32))),
           ("B dark", dataclasses.replace(seen, background=np.array([3.0e-41, 0.0, 1.5], np.float32)))]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    acc.set_camera(cam[:3], cam[3:])
    for i, (key, flat) in enumerate(seq):
        if i > 0:
            acc.set_background(flat.background)
        assert acc.background().tobytes() == flat.background.tobytes()
        _frames(rtk, acc, S, key, flat, mode, key, reps=2)
    _differ(S, seq)


# ---------------------------------------------------------------- 7. RTK_TRAVERSAL_FAST: the opaque-only occlusion tree, re-made

def _fast(rtk, monkeypatch, scene, occluders=True, **tree):
    # AUTO's engine trial off: on a FAST accel with transmissive materials the two engines count occlusion queries differently, so
    # `rays` is comparable only when the live accel and the fresh one run the same engine (tests/test_gpu_views.py)
    monkeypatch.setenv("RTK_AUTO_TRIALS", "0")
    if not occluders:
        monkeypatch.setenv("RTK_FAST_OCCLUDERS", "0")
    acc = rtk.KdTreeSimdAccel(scene, traversal=rtk.TRAVERSAL_FAST, **tree)
    monkeypatch.delenv("RTK_AUTO_TRIALS")
    if not occluders:
        monkeypatch.delenv("RTK_FAST_OCCLUDERS")
    return acc


def _observe(rtk, acc, w, h, queries, depth=6):
    """everything the opaque-only tree can change: frames through the pipeline and through auto, their `rays`, the pipeline's
    radiance of the camera rays, and an occlusion batch"""
    out = []
    for mode in ("stream", "auto", "stream"):
        rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, max_ray_depth=depth, trace_mode=_mode(rtk, mode)))
        out.append((rgb, cn["rays"]))
    occ, n_int = acc.occluded(queries[0], queries[1], 1e-4, rtk.TRACE_AUTO, count=True)
    return out, occ, n_int


def _equal(a, b, what):
    (fa, oa, na), (fb, ob, nb) = a, b
    for i, ((ra, ca), (rb, cb)) in enumerate(zip(fa, fb)):
        bad = int((ra.view(np.uint32) != rb.view(np.uint32)).any(axis=-1).sum())
        assert bad == 0 and ca == cb, (what, i, bad, ca, cb)
    assert oa.tobytes() == ob.tobytes() and na == nb, what


def _changed(a, b):
    return not same(a[0][0][0], b[0][0][0])


def _scene8_queries(ora):
    base = _flat(ora, SCENE8)
    oacc = ora.Accel(ora.Scene(base), ora.ACCEL_KD_SIMD)
    _, _, P = camera_hits(oacc, 48, 32)
    P = P[np.isfinite(P).all(axis=1)]
    q = [shadow_queries(base, P, light)[:2] for light in range(4)]
    return np.concatenate([r for r, _ in q]), np.concatenate([t for _, t in q])


@pytest.mark.parametrize("occluders", [True, False], ids=["occluders", "RTK_FAST_OCCLUDERS=0"])
def test_fast_accel_regather(rtk, ora, monkeypatch, occluders):
    """hw11/scene8: material 1 is the dragon (refractive), 2..6 the walls and caps."""
    from test_gpu_update import _twist
    base = _flat(ora, SCENE8)
    assert base.mat_kind[1] == REFRACTIVE and base.mesh_material.tolist() == [2, 3, 4, 5, 6, 1]
    w, h = 96, 54
    queries = _scene8_queries(ora)
    wall = 2                                                         # mesh 0: asserted below to matter to the frame
    dragon_diffuse = with_material(base, 1, kind=DIFFUSE, albedo=[0.8, 0.7, 0.2])
    two = with_material(base, wall, kind=REFRACTIVE, ior=1.3)
    every = base
    for m in range(len(base.mat_kind)):
        every = with_material(every, m, kind=REFRACTIVE, ior=1.2 + 0.05 * m)

    def fresh(flat):
        return _observe(rtk, _fast(rtk, monkeypatch, _rtk_scene(rtk, flat), occluders), w, h, queries)

    def live(acc):
        return _observe(rtk, acc, w, h, queries)

    acc = _fast(rtk, monkeypatch, _rtk_scene(rtk, base), occluders)
    at_build = live(acc)
    _equal(at_build, fresh(base), "build")
    set_materials(acc, dragon_diffuse)                               # (a) the tree is dropped
    a = live(acc)
    _equal(a, fresh(dragon_diffuse), "a")
    assert _changed(at_build, a)
    set_materials(acc, base)                                         # (b) re-made on an accel that had one
    _equal(live(acc), at_build, "b")
    set_materials(acc, two)                                          # (c) a second material refractive as well
    c = live(acc)
    _equal(c, fresh(two), "c")
    assert _changed(at_build, c)
    set_materials(acc, every)                                        # (h) nothing opaque: the placeholders
    hh = live(acc)
    _equal(hh, fresh(every), "h")
    assert _changed(c, hh)
    set_materials(acc, base)
    _equal(live(acc), at_build, "back from h")
    # (d) first allocation: the dragon is diffuse when the accel is built
    late = _fast(rtk, monkeypatch, _rtk_scene(rtk, dragon_diffuse), occluders)
    _equal(live(late), a, "d before")
    set_materials(late, base)
    _equal(live(late), at_build, "d")
    # (e) update_vertices, then set_materials: the arrays exist on the device only
    v = _twist(base, 0.5).astype(np.float32)
    moved = dataclasses.replace(base, vertices=v)
    acc.update_vertices(v)
    e0 = live(acc)
    _equal(e0, fresh(moved), "e update")
    set_materials(acc, dataclasses.replace(two, vertices=v))
    e1 = live(acc)
    _equal(e1, fresh(dataclasses.replace(two, vertices=v)), "e")
    assert _changed(e0, e1)
    # (g) set_materials, then update_vertices: the flags the rebuild reads.  The dragon turns OPAQUE while a wall keeps the scene
    # transmissive: a rebuild from stale flags would leave the dragon out of the opaque-only tree, and with it every shadow it casts
    solid = with_material(dragon_diffuse, wall, kind=REFRACTIVE, ior=1.3)
    want = fresh(solid)
    assert _changed(c, want)
    set_materials(acc, dataclasses.replace(solid, vertices=v))       # device-made flags (the update of (e) made them)
    acc.update_vertices(base.vertices)
    _equal(live(acc), want, "g")
    fresh_flags = _fast(rtk, monkeypatch, _rtk_scene(rtk, base), occluders)
    live(fresh_flags)                                                # resident, never updated: the flags do not exist yet
    set_materials(fresh_flags, solid)
    fresh_flags.update_vertices(base.vertices)                       # ... and are made on the host, from the new materials
    _equal(live(fresh_flags), want, "g host-made flags")
    set_materials(acc, two)
    _equal(live(acc), c, "g back")
    # (f) update_geometry to 1,000 dragon triangles, then set_materials
    ntris = base.mesh_ntris.copy()
    first = int(ntris[:5].sum())
    ntris[5] = 1000
    idx = np.ascontiguousarray(base.indices[:first + 1000])
    small = dataclasses.replace(base, mesh_ntris=ntris, indices=idx)
    acc.update_geometry(base.vertices, idx, ntris)
    set_materials(acc, dataclasses.replace(dragon_diffuse, mesh_ntris=ntris, indices=idx))
    set_materials(acc, dataclasses.replace(two, mesh_ntris=ntris, indices=idx))
    _equal(live(acc), fresh(dataclasses.replace(two, mesh_ntris=ntris, indices=idx)), "f")
    acc.update_vertices(base.vertices)                               # ... and the rebuild behind it reads the flags of the NEW topology
    _equal(live(acc), fresh(dataclasses.replace(two, mesh_ntris=ntris, indices=idx)), "f then g")
    assert small.mesh_ntris[5] == 1000


# ---------------------------------------------------------------- 8. the smallest shapes the gather can get wrong

def test_fast_accel_regather_leaf_sizes(rtk, ora, monkeypatch):
    """Leaves of exactly 1, 63, 64, 65 and more than 128 references, a leaf with no opaque reference and one with only opaque ones;
    either material toggled to refractive, both, and back."""
    flat, _, _ = octant_scene(ora)
    w = h = 64
    rays, max_t = segments(flat, 4000, 9)

    def state(a, b):
        f = with_material(flat, 0, kind=REFRACTIVE if a else DIFFUSE)
        return with_material(f, 1, kind=REFRACTIVE if b else DIFFUSE)

    def fresh(f):
        return _observe(rtk, _fast(rtk, monkeypatch, _rtk_scene(rtk, f), **TREE), w, h, (rays, max_t), depth=4)

    acc = _fast(rtk, monkeypatch, _rtk_scene(rtk, flat), **TREE)
    seen = [_observe(rtk, acc, w, h, (rays, max_t), depth=4)]
    _equal(seen[0], fresh(flat), "build")
    for a, b in ((1, 0), (0, 1), (1, 1), (0, 0), (0, 1), (1, 0)):
        f = state(a, b)
        set_materials(acc, f)
        seen.append(_observe(rtk, acc, w, h, (rays, max_t), depth=4))
        _equal(seen[-1], fresh(f), (a, b))
        assert _changed(seen[-2], seen[-1]), (a, b)
    acc.update_vertices(flat.vertices)                               # the device-made copy of the same tree, then the regather on it
    for a, b in ((0, 1), (1, 0)):
        f = state(a, b)
        set_materials(acc, f)
        _equal(_observe(rtk, acc, w, h, (rays, max_t), depth=4), fresh(f), ("updated", a, b))
        acc.update_vertices(flat.vertices)                           # ... and a rebuild from the flags that call left
        _equal(_observe(rtk, acc, w, h, (rays, max_t), depth=4), fresh(f), ("updated, rebuilt", a, b))


# ---------------------------------------------------------------- 9. a refused call on a resident accel

def test_refused_set_materials_on_a_resident_accel(rtk, ora):
    S = _states(ora)
    base = _flat(ora, SCENE5)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    _frames(rtk, acc, S, "M own", base, "auto", "before", shapes=((70, 45),), reps=2)
    m = acc.materials()
    for bad_kind in (5, -1, TEXTURE):
        kind = m["kind"].copy()
        kind[1] = bad_kind
        with pytest.raises(rtk.RtkError) as e:
            acc.set_materials(kind, m["albedo"] * 0.5, m["ior"], m["smooth"], np.zeros(2, np.int32))
        assert e.value.code == rtk.RTK_ERR_INVALID
        for mode in ("auto", "stream"):
            _frames(rtk, acc, S, "M own", base, mode, ("refused", bad_kind), shapes=((70, 45),), reps=1)
    glass = with_material(base, 1, kind=REFRACTIVE, ior=1.5)
    set_materials(acc, glass)
    _frames(rtk, acc, S, "M dragon refractive", glass, "auto", "after", shapes=((70, 45),), reps=2)
