"""rtk_accel_radiance / rtk_accel_radiance_device against the CPU oracle's frames: a frame rendered with spp = 1 is the radiance of
its camera rays, so k views of a scene (tests/radiance_views.py) are k oracle frames on one side and ONE batch of caller-supplied
rays on the other, for an accel built once from the unmodified scene.  Colours are compared on bits, ray counters exactly.
Every family first asserts, on the oracle side, that its rays reach the materials it is there for."""
import os
import re

import numpy as np
import pytest

from conftest import SCENE2, SCENE5, SCENE8, SCENES
from radiance_views import (KIND_MISS, ViewBatch, interior_views, jittered_views, kind_counts, rtk_scene_from_flat, special_rays,
                            with_constant_material)

pytestmark = pytest.mark.gpu

HW12_1 = os.path.join(SCENES, "hw12", "scene1.crtscene")
HW12_4 = os.path.join(SCENES, "hw12", "scene4.crtscene")
HW11_4 = os.path.join(SCENES, "hw11", "scene4.crtscene")
DIFFUSE, REFLECTIVE, REFRACTIVE, CONSTANT, TEXTURE = 0, 1, 2, 3, 4
INTERIOR = {
    "hw09_scene5": (SCENE5, {DIFFUSE: 1000, REFLECTIVE: 1000, KIND_MISS: 1000}),
    "hw11_scene8": (SCENE8, {DIFFUSE: 1000, REFRACTIVE: 1000, KIND_MISS: 200}),
    "hw15_scene2": (SCENE2, {DIFFUSE: 1000, REFLECTIVE: 1000, REFRACTIVE: 1000}),
}

_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _accel(rtk, path):
    if ("acc", path) not in _cache:
        _cache["acc", path] = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    return _cache["acc", path]


def _interior(ora, name, k=32, w=64, h=64):
    key = ("views", name, k, w, h)
    if key not in _cache:
        _cache[key] = ViewBatch(ora, interior_views(ora.load_crtscene(INTERIOR[name][0]), k), w, h)
    return _cache[key]


def _frames(vb, name, **kw):
    key = ("frames", name, vb.n, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = vb.frames(**kw)
    return _cache[key]


def _shuffle(n, seed=11):
    return np.random.default_rng(seed).permutation(n)


def _same(got, ref, what):
    diff = np.flatnonzero((_bits(got) != _bits(ref)).any(axis=1))
    print(f"{what}: {len(ref)} rays, {diff.size} differ")
    assert diff.size == 0, (what, diff.size, diff[:8], got[diff[:8]], ref[diff[:8]])


# ---- 1. interior views
@pytest.mark.parametrize("name,depth", [("hw09_scene5", 5), ("hw11_scene8", 5), ("hw11_scene8", 10), ("hw15_scene2", 5)])
def test_interior_views(rtk, ora, name, depth):
    vb = _interior(ora, name)
    assert vb.n == 131_072
    counts = kind_counts(vb.level0()[1])
    print(name, "level-0 kinds", counts)
    for kind, least in INTERIOR[name][1].items():
        assert counts.get(kind, 0) >= least, (kind, counts)
    ref, ref_rays = _frames(vb, name, max_depth=depth)
    acc = _accel(rtk, INTERIOR[name][0])
    cfg = rtk.RadianceConfig(max_ray_depth=depth, cull=True)
    got, cn = acc.radiance(vb.rays, vb.ids, cfg)
    print(name, "depth", depth, "rays", cn["rays"], "oracle", ref_rays)
    _same(got, ref, f"{name} depth {depth}")
    assert cn["rays"] == ref_rays and cn["primary"] == vb.n
    assert cn["hits"] == cn["nodes"] == cn["tris"] == 0
    perm = _shuffle(vb.n)
    got2, cn2 = acc.radiance(vb.rays[perm], vb.ids[perm], cfg)
    _same(got2, ref[perm], f"{name} depth {depth} shuffled")
    assert cn2 == cn


# ---- 2. views near the scene's own camera: texture materials, the bitmap included
@pytest.mark.parametrize("scene", [HW12_4, HW12_1, HW11_4], ids=["hw12_scene4", "hw12_scene1", "hw11_scene4"])
def test_views_near_the_camera(rtk, ora, scene):
    flat = ora.load_crtscene(scene)
    vb = ViewBatch(ora, jittered_views(flat, 16), 48, 48)
    counts = kind_counts(vb.level0()[1])
    print(scene, "level-0 kinds", counts, "texture kinds", flat.tex_kind)
    if scene != HW11_4:
        assert counts.get(TEXTURE, 0) >= 2000 and 3 in flat.tex_kind.tolist()      # (3: a bitmap texture)
    ref, ref_rays = vb.frames(max_depth=5)
    got, cn = _accel(rtk, scene).radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=5))
    _same(got, ref, scene)
    assert cn["rays"] == ref_rays and cn["primary"] == vb.n


# ---- 3. constant material (no scene file has one in view)
def test_constant_material(rtk, ora):
    flat = with_constant_material(ora, ora.load_crtscene(SCENE5), REFLECTIVE)
    vb = ViewBatch(ora, interior_views(flat, 32), 64, 64)
    counts = kind_counts(vb.level0()[1])
    print("level-0 kinds", counts)
    assert counts.get(CONSTANT, 0) >= 1000
    ref, ref_rays = vb.frames(max_depth=5)
    acc = rtk.KdTreeSimdAccel(rtk_scene_from_flat(rtk, flat))
    got, cn = acc.radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=5))
    _same(got, ref, "constant")
    assert cn["rays"] == ref_rays


# ---- 4. diffuse GI: ids and sample name the RNG keys
def _gi_views(ora):
    return _interior(ora, "hw15_scene2", k=8, w=32, h=32)


def test_diffuse_gi_keys_follow_ids(rtk, ora):
    vb = _gi_views(ora)
    assert vb.n == 8192
    counts = kind_counts(vb.level0()[1])
    print("level-0 kinds", counts)
    assert counts.get(DIFFUSE, 0) >= 4000
    ref, ref_rays = _frames(vb, "hw15_scene2", max_depth=5, diffuse_rays=1)
    acc = _accel(rtk, SCENE2)
    cfg = rtk.RadianceConfig(max_ray_depth=5, diffuse_rays=1)
    got, cn = acc.radiance(vb.rays, vb.ids, cfg)
    print("rays", cn["rays"], "oracle", ref_rays)
    _same(got, ref, "GI spp 1")
    assert cn["rays"] == ref_rays and cn["primary"] == vb.n
    one = vb.w * vb.h                                        # a single view: index and pixel coincide
    got1, _ = acc.radiance(vb.rays[:one], None, cfg)
    _same(got1, ref[:one], "GI ids=None")
    wrong, _ = acc.radiance(vb.rays, (vb.ids + 1).astype(np.uint32), cfg)
    n_diff = int((_bits(wrong) != _bits(ref)).any(axis=1).sum())
    print("wrong ids: colours that differ", n_diff)
    assert n_diff >= 1                                       # the keys are seen: other ids, other GI rays
    other, _ = acc.radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=5, diffuse_rays=1, seed=43))
    assert int((_bits(other) != _bits(ref)).any(axis=1).sum()) >= 1
    # without diffuse rays ids, seed and sample cannot change a result
    a, _ = acc.radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=5))
    b, _ = acc.radiance(vb.rays, None, rtk.RadianceConfig(max_ray_depth=5, seed=7, sample=3))
    _same(a, b, "no GI: keys unused")


def test_diffuse_gi_samples_sum_to_the_frame(rtk, ora):
    vb = _gi_views(ora)
    ref, ref_rays = _frames(vb, "hw15_scene2", spp=4, max_depth=5, diffuse_rays=1)
    acc = _accel(rtk, SCENE2)
    total = np.zeros((vb.n, 3), np.float32)
    rays = 0
    for s in range(4):
        got, cn = acc.radiance(vb.camera_rays(spp=4, sample=s), vb.ids, rtk.RadianceConfig(max_ray_depth=5, diffuse_rays=1, sample=s))
        total = total + got                                  # float32, in sample order (render.hpp:66-70)
        rays += cn["rays"]
    total = total / np.float32(4)                            # render.hpp:72
    assert total.dtype == np.float32
    _same(total, ref, "GI spp 4")
    assert rays == ref_rays


# ---- 5. cull = 0
def test_cull_flag(rtk, ora):
    """Rays whose oracle hit record is the same with and without back-face culling must keep the colour they have with cull = 1.
    For the others the oracle has no colour to offer without being changed (its frame path always culls camera rays), so the test
    asserts only that they come back finite and that at least one changed colour against cull = 1: the flag reaches the trace."""
    vb = _interior(ora, "hw15_scene2")
    h1, _ = vb.level0(cull=True)
    h0, _ = vb.level0(cull=False)
    same = (h1.view(np.uint8).reshape(vb.n, -1) == h0.view(np.uint8).reshape(vb.n, -1)).all(axis=1)
    print("identical records", same.sum(), "differ", (~same).sum())
    assert same.sum() >= 50_000 and (~same).sum() >= 5_000
    ref, _ = _frames(vb, "hw15_scene2", max_depth=5)
    got, cn = _accel(rtk, SCENE2).radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=5, cull=False))
    _same(got[same], ref[same], "cull=0, same record")
    assert np.isfinite(got[~same]).all()
    changed = int((_bits(got[~same]) != _bits(ref[~same])).any(axis=1).sum())
    print("changed colour", changed)
    assert changed >= 1 and cn["primary"] == vb.n


# ---- 6. against the frame path itself
@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_camera_rays_give_the_frame(rtk, ora, mode):
    tm = {"auto": rtk.TRACE_AUTO, "stream": rtk.TRACE_STREAM}[mode]
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    fcfg = rtk.RenderConfig(width=480, height=270, max_ray_depth=10, trace_mode=tm)
    frame, fcn = acc.render_frame(fcfg)
    rays = acc.camera_rays(fcfg).reshape(-1, 6)
    got, cn = acc.radiance(rays, None, rtk.RadianceConfig(max_ray_depth=10, cull=True, trace_mode=tm))
    _same(got, frame.reshape(-1, 3), f"frame {mode}")
    print("rays", cn["rays"], fcn["rays"])
    assert cn["rays"] == fcn["rays"] and cn["primary"] == fcn["primary"] == 480 * 270
    assert acc.last_counters() == fcn                        # the frame's counters survive the batch


# ---- 7. queue overflow: the per-ray fallback kernel
def _redone(capfd):
    err = capfd.readouterr().err
    m = re.findall(r"\[rtk radiance\] rays (\d+) chunks (\d+) redone (\d+)", err)
    assert m, err
    return [(int(a), int(b), int(c)) for a, b, c in m]


def test_queue_overflow_is_redone_on_the_device(rtk, ora, monkeypatch, capfd):
    """With room for the batch's own rays only, refraction / GI children and the shading points overflow the queues: every chunk must
    be redone by the per-ray kernel (asserted through RTK_STREAM_DEBUG's report) and still be exact, counters included."""
    monkeypatch.setenv("RTK_STREAM_NODE_FACTOR", "1")              # environment knobs are read when an accel is built
    monkeypatch.setenv("RTK_STREAM_DEBUG", "1")
    vb = _interior(ora, "hw11_scene8")
    ref, ref_rays = _frames(vb, "hw11_scene8", max_depth=10)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    capfd.readouterr()
    got, cn = acc.radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=10))
    report = _redone(capfd)
    print("scene8 depth 10:", report)
    assert report[-1][0] == vb.n and report[-1][2] >= 1 and report[-1][2] == report[-1][1]
    _same(got, ref, "overflow scene8")
    assert cn["rays"] == ref_rays and cn["primary"] == vb.n
    perm = _shuffle(vb.n)
    got, cn = acc.radiance(vb.rays[perm], vb.ids[perm], rtk.RadianceConfig(max_ray_depth=10))
    assert _redone(capfd)[-1][2] >= 1
    _same(got, ref[perm], "overflow scene8 shuffled")
    assert cn["rays"] == ref_rays
    # diffuse GI
    gv = _gi_views(ora)
    gref, gref_rays = _frames(gv, "hw15_scene2", max_depth=5, diffuse_rays=1)
    acc2 = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    got, cn = acc2.radiance(gv.rays, gv.ids, rtk.RadianceConfig(max_ray_depth=5, diffuse_rays=1))
    report = _redone(capfd)
    print("hw15/scene2 GI:", report)
    assert report[-1][2] >= 1
    _same(got, gref, "overflow GI")
    assert cn["rays"] == gref_rays
    # and without the knob nothing is redone (no GI: the ray tree of this batch is a fraction of the default queues)
    monkeypatch.delenv("RTK_STREAM_NODE_FACTOR")
    acc3 = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    got, cn = acc3.radiance(gv.rays, gv.ids, rtk.RadianceConfig(max_ray_depth=5))
    assert _redone(capfd)[-1][2] == 0
    _same(got, _frames(gv, "hw15_scene2", max_depth=5)[0], "default queues")


def test_small_chunks_over_all_lanes(rtk, ora, monkeypatch, capfd):
    """A small memory budget cuts the batch into many chunks dealt over the lane streams; chunk borders need not be multiples of
    anything the caller knows.  Same colours, same counters, ids == None counted across chunks."""
    monkeypatch.setenv("RTK_STREAM_MEM_GB", "1")
    monkeypatch.setenv("RTK_STREAM_NODE_FACTOR", "400")
    monkeypatch.setenv("RTK_STREAM_DEBUG", "1")
    vb = _gi_views(ora)
    ref, ref_rays = _frames(vb, "hw15_scene2", max_depth=5, diffuse_rays=1)
    big = _interior(ora, "hw15_scene2")
    bref, bref_rays = _frames(big, "hw15_scene2", max_depth=5)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    capfd.readouterr()
    got, cn = acc.radiance(big.rays[:100_003], big.ids[:100_003], rtk.RadianceConfig(max_ray_depth=5))
    report = _redone(capfd)
    print("chunks", report)
    assert report[-1][1] >= 5 and report[-1][2] == 0
    _same(got, bref[:100_003], "chunked")
    # ids == None: ray i is pixel index i of the BATCH, whichever chunk it falls into (diffuse GI: the keys matter)
    one = vb.w * vb.h
    rays = np.tile(vb.rays[:one], (40, 1))
    gi = rtk.RadianceConfig(max_ray_depth=5, diffuse_rays=1)
    got, cn = acc.radiance(rays, None, gi)
    report = _redone(capfd)
    print("chunks", report)
    assert report[-1][1] >= 4 and report[-1][2] == 0
    want, wcn = _accel(rtk, SCENE2).radiance(rays, np.arange(len(rays), dtype=np.uint32), gi)
    _same(got, want, "chunked, ids=None, GI")
    _same(want[:one], ref[:one], "explicit ids, GI")
    assert cn == wcn
    assert int((_bits(want[one:2 * one]) != _bits(want[:one])).any(axis=1).sum()) >= 1        # other ids, other GI rays


# ---- 8. ragged sizes, guard words, two streams
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100_003])
def test_ragged_sizes(rtk, ora, n):
    import torch

    vb = _interior(ora, "hw11_scene8")
    ref, _ = _frames(vb, "hw11_scene8", max_depth=5)
    perm = _shuffle(vb.n)
    rays, ids, want = vb.rays[perm][:n], vb.ids[perm][:n], ref[perm][:n]
    acc = _accel(rtk, SCENE8)
    cfg = rtk.RadianceConfig(max_ray_depth=5)
    got, cn = acc.radiance(rays, ids, cfg)
    assert got.shape == (n, 3) and cn["primary"] == n
    _same(got, want, f"n={n}")
    guard = 5
    d_rays = torch.from_numpy(np.ascontiguousarray(vb.rays[perm][:max(n, 1)])).to("cuda")
    d_ids = torch.from_numpy(np.ascontiguousarray(vb.ids[perm][:max(n, 1)]).view(np.int32)).to("cuda")
    d_rgb = torch.full((n * 3 + 2 * guard,), -7.5, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    acc.radiance_device(d_rays.data_ptr(), d_ids.data_ptr(), n, d_rgb.data_ptr() + 4 * guard, cfg, s.cuda_stream)
    s.synchronize()
    out = d_rgb.cpu().numpy()
    assert (out[:guard] == -7.5).all() and (out[guard + 3 * n:] == -7.5).all()
    _same(out[guard:guard + 3 * n].reshape(n, 3), want, f"device n={n}")


def test_two_streams_at_once(rtk, ora):
    import torch

    vb = _interior(ora, "hw11_scene8")
    ref, _ = _frames(vb, "hw11_scene8", max_depth=5)
    perm = _shuffle(vb.n)
    rays, ids, want = np.ascontiguousarray(vb.rays[perm]), np.ascontiguousarray(vb.ids[perm]), ref[perm]
    acc = _accel(rtk, SCENE8)
    cfg = rtk.RadianceConfig(max_ray_depth=5)
    half = vb.n // 2 + 1
    d_rays = torch.from_numpy(rays).to("cuda")
    d_ids = torch.from_numpy(ids.view(np.int32)).to("cuda")
    out1 = torch.full((vb.n * 3,), -7.5, dtype=torch.float32, device="cuda")
    out2 = torch.full((vb.n * 3,), -7.5, dtype=torch.float32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    acc.radiance_device(d_rays.data_ptr(), d_ids.data_ptr(), half, out1.data_ptr(), cfg, s1.cuda_stream)
    acc.radiance_device(d_rays.data_ptr() + 24 * half, d_ids.data_ptr() + 4 * half, vb.n - half, out2.data_ptr() + 12 * half, cfg,
                        s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    o1, o2 = out1.cpu().numpy().reshape(-1, 3), out2.cpu().numpy().reshape(-1, 3)
    _same(o1[:half], want[:half], "stream 1")
    _same(o2[half:], want[half:], "stream 2")
    assert (o1[half:] == -7.5).all() and (o2[:half] == -7.5).all()


# ---- 9. special values
def test_special_values(rtk, ora):
    """NaN / +-inf components and zero directions cannot come out of a camera, so the oracle has nothing to say about them: the
    call returns, and every OTHER ray of the batch keeps its exact colour."""
    vb = _interior(ora, "hw11_scene8")
    ref, _ = _frames(vb, "hw11_scene8", max_depth=5)
    rays, touched = special_rays(vb.rays[:16_384])
    assert touched.sum() >= 1500 and (~touched).sum() >= 10_000
    got, cn = _accel(rtk, SCENE8).radiance(rays, vb.ids[:16_384], rtk.RadianceConfig(max_ray_depth=5))
    _same(got[~touched], ref[:16_384][~touched], "untouched rays")
    assert cn["primary"] == 16_384


# ---- 10. bad arguments; frames before and after
def test_bad_arguments_leave_the_accel_working(rtk, ora):
    import torch

    vb = _interior(ora, "hw11_scene8")
    ref, _ = _frames(vb, "hw11_scene8", max_depth=5)
    acc = _accel(rtk, SCENE8)
    rays, ids = np.ascontiguousarray(vb.rays[:1000]), np.ascontiguousarray(vb.ids[:1000])
    d_rays = torch.from_numpy(rays).to("cuda")
    d_rgb = torch.zeros(3000, dtype=torch.float32, device="cuda")
    R = rtk.RadianceConfig
    bad = [R(trace_mode=m) for m in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_GROUP4, rtk.TRACE_TWOPASS, rtk.TRACE_REPACK, -1)]
    bad += [R(max_ray_depth=17), R(max_ray_depth=-1), R(diffuse_rays=-1), R(sample=-1), R(shadow_bias=float("nan")),
            R(reflection_bias=float("inf")), R(refraction_bias=float("-inf"))]
    for cfg in bad:
        with pytest.raises(rtk.RtkError) as e:
            acc.radiance(rays, ids, cfg)
        assert e.value.code == rtk.RTK_ERR_INVALID, cfg
        with pytest.raises(rtk.RtkError) as e:
            acc.radiance_device(d_rays.data_ptr(), 0, 1000, d_rgb.data_ptr(), cfg)
        assert e.value.code == rtk.RTK_ERR_INVALID, cfg
    for ptrs in ((0, d_rgb.data_ptr()), (d_rays.data_ptr(), 0)):
        with pytest.raises(rtk.RtkError) as e:
            acc.radiance_device(ptrs[0], 0, 1000, ptrs[1])
        assert e.value.code == rtk.RTK_ERR_INVALID
    acc.radiance_device(0, 0, 0, 0)
    got, _ = acc.radiance(rays, ids, R(max_ray_depth=5))
    _same(got, ref[:1000], "after bad arguments")
    acc.radiance_device(d_rays.data_ptr(), 0, 1000, d_rgb.data_ptr(), R(max_ray_depth=5))
    torch.cuda.synchronize()
    _same(d_rgb.cpu().numpy().reshape(-1, 3), ref[:1000], "device, after bad arguments")


@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_frames_before_and_after_a_batch_are_the_same(rtk, ora, mode):
    vb = _interior(ora, "hw11_scene8")
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    cfg = rtk.RenderConfig(width=480, height=270, max_ray_depth=10, collect_stats=1,
                           trace_mode={"auto": rtk.TRACE_AUTO, "stream": rtk.TRACE_STREAM}[mode])
    rgb0, cn0 = acc.render_frame(cfg)
    got, cn = acc.radiance(vb.rays, vb.ids, rtk.RadianceConfig(max_ray_depth=5))
    assert cn["rays"] >= vb.n
    assert acc.last_counters() == cn0
    rgb1, cn1 = acc.render_frame(cfg)
    assert np.array_equal(rgb0.view(np.uint32), rgb1.view(np.uint32)) and cn0 == cn1
    _same(got, _frames(vb, "hw11_scene8", max_depth=5)[0], "between frames")
