"""rtk_render_motion on the device against the numpy model of the contract (tests/motion_model.py), bit for bit: the planes of
hw09/scene5 at every size with each output alone and both, on a second stream and twice; the scene's own pose and camera; a rigid
translation; hostile but legal planes; stale ids after rtk_accel_update_geometry; the first call on a fresh accel; and the chain
update_vertices -> render_gbuffer -> render_motion -> temporal_accumulate on the device."""
import numpy as np
import pytest

import motion_model as mm
import temporal_model as tm
from conftest import SCENE5

pytestmark = pytest.mark.gpu

GUARD = 64
COMPS = dict(prev_position=3, motion=2)
PREV_VIEW_OFFSET = np.array((0.5, -0.25, 1.0), np.float32)


@pytest.fixture(scope="module")
def accel(rtk):
    """an accel of scene5 that no test of this module updates"""
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))


def _fresh(rtk):
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))


def _host(rtk, acc, tri, bary, verts, view, outputs, fov=mm.FOV):
    return acc.render_motion(tri, bary, verts, view, rtk.MotionConfig(fov_degrees=fov), planes=outputs)


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a.astype(np.float32, copy=False)).cuda()


def _device(rtk, acc, tri, bary, verts, view, outputs, stream=None, twice=False, fov=mm.FOV):
    """the device variant on torch buffers with guard words behind every output; the inputs must come back untouched"""
    import torch
    h, w = tri.shape
    n = w * h
    ins = dict(tri=_up(tri), bary=_up(bary), verts=_up(verts))
    outs = {k: torch.full((COMPS[k] * n + GUARD,), 7.0, dtype=torch.float32, device="cuda") for k in outputs}
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        for _ in range(2 if twice else 1):
            acc.render_motion_device(w, h, ins["tri"].data_ptr(), ins["bary"].data_ptr(), ins["verts"].data_ptr(),
                                     {k: t.data_ptr() for k, t in outs.items()}, prev_view=view, cfg=rtk.MotionConfig(fov_degrees=fov),
                                     stream=s.cuda_stream)
    s.synchronize()
    res = {}
    for k, t in outs.items():
        a = t.cpu().numpy()
        assert (a[COMPS[k] * n:] == 7).all(), k                                  # nothing written behind an output
        res[k] = a[:COMPS[k] * n].reshape(h, w, COMPS[k])
    for k, src in (("tri", tri), ("bary", bary), ("verts", verts)):              # the inputs are inputs
        assert np.array_equal(ins[k].cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(src).view(np.uint32).reshape(-1)), k
    return res


def _gbuffer(rtk, acc, w, h, planes=("tri", "bary", "position", "depth", "normal", "mesh")):
    gb = acc.render_gbuffer(rtk.RenderConfig(width=w, height=h, spp=1, fov_degrees=mm.FOV), sample=0, planes=planes)
    return {k: gb[k][0] for k in planes}


@pytest.mark.parametrize("w,h", mm.SIZES)
def test_host_device_and_model_agree_in_every_bit(rtk, ora, accel, w, h):
    import torch
    flat, _, index, view = mm.scene5(ora)
    base = mm.planes(ora, w, h)
    verts = mm.moved_vertices(flat)
    prev_view = (view[0] + PREV_VIEW_OFFSET, view[1])
    want = mm.render_motion(base["tri"], base["bary"], index, verts, prev_view)
    for outputs in mm.OUTPUTS:
        v = prev_view if "motion" in outputs else None
        got = _host(rtk, accel, base["tri"], base["bary"], verts, v, outputs)
        assert sorted(got) == sorted(outputs)
        mm.assert_same(got, want, outputs, ("host", outputs))
        mm.assert_same(_device(rtk, accel, base["tri"], base["bary"], verts, v, outputs), want, outputs, ("device", outputs))
    both = ("prev_position", "motion")
    mm.assert_same(_device(rtk, accel, base["tri"], base["bary"], verts, prev_view, both, stream=torch.cuda.Stream()), want, both, "second stream")
    mm.assert_same(_device(rtk, accel, base["tri"], base["bary"], verts, prev_view, both, twice=True), want, both, "twice")
    mm.assert_same(_host(rtk, accel, base["tri"], base["bary"], verts, prev_view, both), want, both, "host again")
    # a view that is handed in without a motion plane is not read
    mm.assert_same(_device(rtk, accel, base["tri"], base["bary"], verts, prev_view, ("prev_position",)), want, ("prev_position",), "idle view")


@pytest.mark.parametrize("w,h", mm.SIZES)
def test_own_pose_and_own_camera_give_the_position_and_no_motion(rtk, ora, accel, w, h):
    flat, _, _, _ = mm.scene5(ora)
    verts = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    gb = _gbuffer(rtk, accel, w, h)
    base = mm.planes(ora, w, h)
    assert np.array_equal(gb["tri"], base["tri"]) and np.array_equal(mm.bits(gb["bary"]), mm.bits(base["bary"]))     # the planes the CPU test measured
    got = _device(rtk, accel, gb["tri"], gb["bary"], verts, accel.camera(), ("prev_position", "motion"))
    hit = gb["depth"] >= 0
    assert hit.any()
    err = float(np.abs(got["prev_position"].astype(np.float64) - gb["position"])[hit].max())
    move = float(np.abs(got["motion"].astype(np.float64))[hit].max())
    print(f"{w}x{h}: max |P' - position| = {err:.4g} (allowed {mm.POSITION_TOL:.4g}), max |motion| = {move:.4g} px (bound {mm.MOTION_BOUND:.4g})")
    assert err <= mm.POSITION_TOL
    assert move <= mm.MOTION_BOUND
    assert not mm.bits(got["prev_position"])[~hit].any() and (mm.bits(got["motion"])[~hit] == mm.MISS_BITS).all()


def test_a_rigid_translation_comes_back_as_position_minus_d(rtk, ora, accel):
    """every vertex of the previous pose lay at v - d: so did every surface point"""
    flat, _, _, _ = mm.scene5(ora)
    d = np.array((0.25, -0.5, 0.125), np.float32)
    verts = (np.asarray(flat.vertices, np.float32).reshape(-1, 3) - d).astype(np.float32)
    for w, h in ((64, 64), (130, 70)):
        gb = _gbuffer(rtk, accel, w, h)
        hit = gb["depth"] >= 0
        for got in (_host(rtk, accel, gb["tri"], gb["bary"], verts, None, ("prev_position",)),
                    _device(rtk, accel, gb["tri"], gb["bary"], verts, None, ("prev_position",))):
            err = float(np.abs(got["prev_position"].astype(np.float64) - (gb["position"].astype(np.float64) - d))[hit].max())
            assert err <= mm.POSITION_TOL, err
            assert not mm.bits(got["prev_position"])[~hit].any()               # misses are exactly zero


@pytest.mark.parametrize("case", ["ids", "barycentrics", "both"])
def test_hostile_but_legal_planes(rtk, ora, accel, case):
    """ids n_triangles, 0xFFFFFFFE and 0xFFFFFFFF among valid ones, NaN, +-inf and 1e30 among the barycentrics: the bounds test
    comes before every dependent load, so the calls finish, and they equal the model"""
    flat, _, index, view = mm.scene5(ora)
    verts = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    base = mm.planes(ora, 130, 70)
    name, tri, bary = next(c for c in mm.hostile_planes(base, index.shape[0]) if c[0] == case)
    both = ("prev_position", "motion")
    want = mm.render_motion(tri, bary, index, verts, view)
    mm.assert_same(_host(rtk, accel, tri, bary, verts, view, both), want, both, (name, "host"))
    mm.assert_same(_device(rtk, accel, tri, bary, verts, view, both), want, both, (name, "device"))
    miss = ~want["hit"]
    assert miss.sum() >= 100 and (tri[miss] >= index.shape[0]).all()
    assert not mm.bits(want["prev_position"])[miss].any() and (mm.bits(want["motion"])[miss] == mm.MISS_BITS).all()


def test_a_previous_view_behind_the_surfaces_has_no_motion(rtk, ora, accel):
    flat, _, index, view = mm.scene5(ora)
    verts = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    base = mm.planes(ora, 64, 64)
    behind = (view[0] + np.array((0.0, -60.0, -120.0), np.float32), view[1])
    both = ("prev_position", "motion")
    want = mm.render_motion(base["tri"], base["bary"], index, verts, behind)
    assert not want["computed"].any()
    for got in (_host(rtk, accel, base["tri"], base["bary"], verts, behind, both), _device(rtk, accel, base["tri"], base["bary"], verts, behind, both)):
        mm.assert_same(got, want, both, "behind")
        assert (mm.bits(got["motion"]) == mm.MISS_BITS).all()


def test_the_first_call_on_a_fresh_accel_makes_its_tables(rtk, ora):
    """no frame, no update before it: the device variant brings the accel to the device and makes the topology tables on demand"""
    flat, _, index, view = mm.scene5(ora)
    base = mm.planes(ora, 130, 70)
    verts = mm.moved_vertices(flat)
    both = ("prev_position", "motion")
    want = mm.render_motion(base["tri"], base["bary"], index, verts, view)
    acc = _fresh(rtk)
    mm.assert_same(_device(rtk, acc, base["tri"], base["bary"], verts, view, both), want, both, "fresh, device")
    mm.assert_same(_host(rtk, _fresh(rtk), base["tri"], base["bary"], verts, view, both), want, both, "fresh, host")
    # ... and an update behind it goes on from the same tables
    acc.update_vertices(verts)
    mm.assert_same(_device(rtk, acc, base["tri"], base["bary"], verts, view, both), want, both, "after an update")


def test_stale_ids_after_update_geometry(rtk, ora):
    """After update_geometry to 3/4 of every triangle list an old frame's ids at or above the new count are misses, and the ids
    below it are read through the NEW lists (mesh 0 lost a triangle, so every id of mesh 1 now names another triangle)."""
    flat, _, old_index, view = mm.scene5(ora)
    verts = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    starts = np.concatenate([[0], np.cumsum(flat.mesh_ntris)]).astype(np.int64)
    ntris = (np.asarray(flat.mesh_ntris, np.int64) * 3 // 4).astype(np.int32)
    local = np.asarray(flat.indices, np.uint32).reshape(-1, 3)
    indices = np.ascontiguousarray(np.concatenate([local[starts[m]:starts[m] + ntris[m]] for m in range(len(ntris))]), np.uint32)
    import dataclasses
    new_index = mm.global_indices(dataclasses.replace(flat, indices=indices, mesh_ntris=ntris))
    nt = int(ntris.sum())
    assert new_index.shape == (nt, 3) and nt < old_index.shape[0] and not np.array_equal(new_index[:nt], old_index[:nt])
    base = mm.planes(ora, 130, 70)                                             # a frame of the OLD topology
    stale = base["hit"] & (base["tri"] >= nt)
    live = base["hit"] & (base["tri"] < nt)
    assert stale.sum() >= 50 and live.sum() >= 50
    acc = _fresh(rtk)
    acc.update_geometry(verts, indices, ntris)
    assert acc.tree_info().n_triangles == nt
    both = ("prev_position", "motion")
    want = mm.render_motion(base["tri"], base["bary"], new_index, verts, view)
    assert not want["hit"][stale].any() and want["hit"][live].all()
    assert not np.array_equal(mm.bits(want["prev_position"]), mm.bits(mm.render_motion(base["tri"], base["bary"], old_index, verts, view)["prev_position"]))
    mm.assert_same(_host(rtk, acc, base["tri"], base["bary"], verts, view, both), want, both, "host")
    mm.assert_same(_device(rtk, acc, base["tri"], base["bary"], verts, view, both), want, both, "device")


def test_the_chain_on_the_device_keeps_a_moved_meshs_history(rtk, ora):
    """update_vertices with one moved mesh, then render_gbuffer, render_motion and temporal_accumulate, all on device planes: fed
    prev_position the moved mesh keeps its history, fed position it loses it, and both are the models' bits given the device's
    own g-buffer planes."""
    import torch
    flat, _, index, view = mm.scene5(ora)
    w, h = 130, 70
    n = w * h
    old = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    new = mm.moved_vertices(flat)
    acc = _fresh(rtk)
    cfg = rtk.RenderConfig(width=w, height=h, spp=1, fov_degrees=mm.FOV)
    prev = _gbuffer(rtk, acc, w, h)
    # 1. the new pose
    acc.update_vertices(new)
    # 2. its g-buffer, on the device
    f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
    g = dict(depth=f32(n), position=f32(3 * n), normal=f32(3 * n), bary=f32(2 * n), tri=i32(n), mesh=i32(n))
    acc.render_gbuffer_device(cfg, {k: t.data_ptr() for k, t in g.items()})
    # 3. where its surface points were
    d_old = _up(old)
    back = f32(3 * n)
    acc.render_motion_device(w, h, g["tri"].data_ptr(), g["bary"].data_ptr(), d_old.data_ptr(), dict(prev_position=back.data_ptr()),
                             cfg=rtk.MotionConfig(fov_degrees=mm.FOV))
    # 4. temporal, fed prev_position and fed position
    grey = torch.full((3 * n,), 0.5, dtype=torch.float32, device="cuda")
    ones = torch.ones(n, dtype=torch.float32, device="cuda")
    d_prev = {k: _up(prev[k]) for k in ("position", "normal", "depth", "mesh")}
    hist = dict(rgb=grey.data_ptr(), length=ones.data_ptr(), view=view, **{k: t.data_ptr() for k, t in d_prev.items()})
    tcfg = rtk.TemporalConfig(**dict(tm.PARAMS, fov_degrees=mm.FOV))
    lengths = []
    for position in (back, g["position"]):
        o_rgb, o_len = f32(3 * n), f32(n)
        rtk.temporal_accumulate_device(w, h, dict(rgb=grey.data_ptr(), position=position.data_ptr(), normal=g["normal"].data_ptr(),
                                                  depth=g["depth"].data_ptr(), mesh=g["mesh"].data_ptr()), hist,
                                       dict(rgb=o_rgb.data_ptr(), length=o_len.data_ptr()), cfg=tcfg)
        lengths.append(o_len)
    torch.cuda.synchronize()
    cur = {k: t.cpu().numpy() for k, t in g.items()}
    cur = dict(depth=cur["depth"].reshape(h, w), position=cur["position"].reshape(h, w, 3), normal=cur["normal"].reshape(h, w, 3),
               bary=cur["bary"].reshape(h, w, 2), tri=cur["tri"].view(np.uint32).reshape(h, w), mesh=cur["mesh"].view(np.uint32).reshape(h, w))
    cur["hit"] = cur["depth"] >= 0
    # the models, given the device's own planes
    want = mm.render_motion(cur["tri"], cur["bary"], index, old)
    mm.assert_same(dict(prev_position=back.cpu().numpy().reshape(h, w, 3)), want, ("prev_position",), "chain")
    params = dict(tm.PARAMS, fov_degrees=mm.FOV)
    shares = []
    for position, length in zip((want["prev_position"], cur["position"]), lengths):
        c, p = mm.temporal_inputs(cur, position, prev, view)
        model = tm.accumulate(c, p, noise=False, mesh=True, **params)
        got = length.cpu().numpy().reshape(h, w)
        assert np.array_equal(mm.bits(got), mm.bits(model["length"]))
        shares.append(mm.kept_share(got, cur))
    print(f"kept with prev_position {shares[0]:.3f}, with position {shares[1]:.3f}")
    assert shares[0] >= mm.SHARE_WITH
    assert shares[1] <= mm.SHARE_WITHOUT
