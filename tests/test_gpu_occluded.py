"""rtk_accel_occluded / rtk_accel_occluded_device against the reference's is_occluded loop (tests/occlusion_model.py, which
tests/test_occlusion_model.py pins to the oracle's renders): the answer bytes and the number of closest-hit queries, exactly.
Every family first asserts, on the reference side, that its inputs reach the outcomes it is there for."""
import os

import numpy as np
import pytest

from conftest import SCENE2, SCENE5, SCENE8, SCENES
from occlusion_model import MISS, camera_hits, occluded_ref, segments, shadow_queries

pytestmark = pytest.mark.gpu

SCENE4 = os.path.join(SCENES, "hw11", "scene4.crtscene")
SEGMENT_SCENES = {"hw09_scene5": SCENE5, "hw11_scene8": SCENE8, "hw15_scene2": SCENE2, "hw11_scene4": SCENE4}
GLASS = ("hw11_scene8", "hw15_scene2", "hw11_scene4")
N_SEG = 60_000
BIAS = 1e-4

_pairs = {}


def _pair(rtk, ora, path):
    if path not in _pairs:
        flat = ora.load_crtscene(path)
        _pairs[path] = (rtk.KdTreeSimdAccel(rtk.parse_scene_file(path)), ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD), flat)
    return _pairs[path]


def _modes(rtk):
    return {"auto": rtk.TRACE_AUTO, "lane": rtk.TRACE_LANE, "wave": rtk.TRACE_WAVE}


def _check(rtk, acc, oacc, flat, rays, max_t, bias=BIAS, modes=None, what=""):
    """GPU bytes and intersection count == the model's, in every mode.  -> (answer, steps, entered) of the model."""
    want, steps, entered = occluded_ref(oacc, flat, rays, max_t, bias, rtk.OCCLUDED_MAX_STEPS, with_entered=True)
    calls = int(steps.sum(dtype=np.int64) + entered.sum())
    for name, mode in (modes or _modes(rtk)).items():
        got, n_int = acc.occluded(rays, max_t, shadow_bias=bias, trace_mode=mode, count=True)
        diff = np.flatnonzero(got != want)
        print(f"{what} {name}: {len(want)} queries, {diff.size} differ, intersections {n_int} vs {calls}")
        assert np.array_equal(got, want), (what, name, diff.size, diff[:8], got[diff[:8]], want[diff[:8]])
        assert n_int == calls, (what, name, n_int, calls)
        assert np.array_equal(acc.occluded(rays, max_t, shadow_bias=bias, trace_mode=mode), want), (what, name, "count=False")
    return want, steps, entered


# ---- 1. segments
@pytest.mark.parametrize("scene", list(SEGMENT_SCENES))
def test_segments(rtk, ora, scene):
    acc, oacc, flat = _pair(rtk, ora, SEGMENT_SCENES[scene])
    rays, max_t = segments(flat, N_SEG, seed=1)
    want, steps, _ = _check(rtk, acc, oacc, flat, rays, max_t, what=scene)
    print(scene, "occluded", (want == 1).sum(), "clear", (want == 0).sum(), "stepped", (steps > 0).sum(),
          "stepped then occluded", ((steps > 0) & (want == 1)).sum(), "longest", steps.max() + 1)
    assert (want == 1).sum() >= N_SEG // 10 and (want == 0).sum() >= N_SEG // 10
    assert not (want == 2).any()
    if scene in GLASS:
        assert (steps > 0).sum() >= 500 and ((steps > 0) & (want == 1)).sum() >= 100


# ---- 2. the shadow rays of a frame
@pytest.mark.parametrize("scene", ["hw09_scene5", "hw11_scene8"])
def test_shadow_rays_of_a_frame(rtk, ora, scene):
    acc, oacc, flat = _pair(rtk, ora, SEGMENT_SCENES[scene])
    _, hits, P = camera_hits(oacc, 480, 270)
    P = P[hits["mesh"] != MISS]
    assert len(P) >= 10_000
    n_stepped = n_occluded = 0
    for k in range(len(flat.light_intensity)):
        rays, radius, _ = shadow_queries(flat, P, k, BIAS)
        want, steps, _ = _check(rtk, acc, oacc, flat, rays, radius, what=f"{scene} light {k}")
        n_stepped += int((steps > 0).sum())
        n_occluded += int((want == 1).sum())
    if scene == "hw09_scene5":
        assert n_occluded >= len(flat.light_intensity) * len(P) // 10
    else:
        assert n_stepped >= 1000


# ---- 3. max_t equal to the closest hit's t: the only way the loop ends through its guard
def test_max_t_equal_to_the_closest_hit(rtk, ora):
    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    rays, _ = segments(flat, N_SEG, seed=1)
    h = oacc.intersect(rays, cull=False)
    sel = h["mesh"] != MISS
    rays, max_t = rays[sel], h["t"][sel].copy()
    refractive = (flat.mat_kind[flat.mesh_material] == 2)[h["mesh"][sel]]
    want, steps, entered = _check(rtk, acc, oacc, flat, rays, max_t, what="max_t = t")
    by_guard = (steps == 1) & ~entered & (want == 0)
    print("opaque first hit -> occluded", (~refractive & (want == 1)).sum(), "transmissive first hit -> guard", by_guard.sum())
    assert (~refractive & (want == 1)).sum() >= 1000 and by_guard.sum() >= 1000
    assert np.array_equal(by_guard, refractive) and np.array_equal(want == 1, ~refractive)


# ---- 4. special values
def test_special_values(rtk, ora):
    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    n = 4096
    rays, max_t = segments(flat, n, seed=4)
    i = np.arange(n)
    max_t[i % 8 == 0] = np.nan
    max_t[i % 8 == 1] = np.inf
    max_t[i % 8 == 2] = -1.0
    max_t[i % 8 == 3] = 0.0
    max_t[i % 8 == 4] = -0.0
    rays[i % 29 == 5, 3:] = 0.0                     # zero direction
    rays[i % 31 == 6, 1] = np.nan                   # NaN origin component
    rays[i % 37 == 7, 4] = np.inf                   # inf direction component
    rays[i % 41 == 9, 5] = -np.inf
    rays[i % 43 == 1, 0] = np.inf                   # inf origin component
    want, steps, entered = _check(rtk, acc, oacc, flat, rays, max_t, what="special")
    dead = (i % 8 == 0) | ((i % 8 >= 2) & (i % 8 <= 4))
    assert not want[dead].any() and not steps[dead].any() and not entered[dead].any()
    print("+inf: occluded", (want[i % 8 == 1] == 1).sum(), "of", (i % 8 == 1).sum())
    assert (want[i % 8 == 1] == 1).sum() >= 100
    # only the dead ones: nothing may be counted
    got, n_int = acc.occluded(rays[dead], max_t[dead], count=True)
    assert not got.any() and n_int == 0


# ---- 5. ragged sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100_003])
def test_ragged_sizes(rtk, ora, n):
    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    rays, max_t = segments(flat, max(n, 1), seed=5)
    want, _, _ = _check(rtk, acc, oacc, flat, rays[:n], max_t[:n], what=f"n={n}")
    assert want.shape == (n,)


# ---- 6. the step limit, and a zero bias
def test_step_limit_with_a_negative_bias(rtk, ora):
    """A negative bias steps back in front of the transmissive surface it just crossed and hits it again: the reference would
    loop until max_t is used up; the kernel answers RTK_OCC_STEP_LIMIT after RTK_OCCLUDED_MAX_STEPS closest-hit queries."""
    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    rays, max_t = segments(flat, N_SEG, seed=1)
    rays, max_t = rays[:4096], max_t[:4096]
    want, steps, entered = _check(rtk, acc, oacc, flat, rays, max_t, bias=-1e-4, what="bias -1e-4")
    limit = want == rtk.OCC_STEP_LIMIT
    print("ran to the limit:", limit.sum(), "of", len(want))
    assert limit.sum() >= 100
    assert (steps[limit] == rtk.OCCLUDED_MAX_STEPS).all() and not entered[limit].any()
    got, n_int = acc.occluded(rays[limit], max_t[limit], shadow_bias=-1e-4, count=True)
    assert (got == rtk.OCC_STEP_LIMIT).all() and n_int == int(limit.sum()) * rtk.OCCLUDED_MAX_STEPS


def test_zero_bias(rtk, ora):
    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    rays, max_t = segments(flat, N_SEG, seed=1)
    want, steps, _ = _check(rtk, acc, oacc, flat, rays, max_t, bias=0.0, what="bias 0")
    assert not (want == 2).any() and (steps > 0).sum() >= 500 and steps.max() < 64


# ---- 7. RTK_TRAVERSAL_FAST on a scene without transmissive materials: the answer depends on t only
def test_fast_traversal_without_glass_gives_the_same_bytes(rtk, ora):
    acc, oacc, flat = _pair(rtk, ora, SCENE5)
    fast = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5), traversal=rtk.TRAVERSAL_FAST)
    rays, max_t = segments(flat, N_SEG, seed=1)
    assert not (flat.mat_kind == 2).any()
    for mode in _modes(rtk).values():
        want, n_want = acc.occluded(rays, max_t, trace_mode=mode, count=True)
        got, n_got = fast.occluded(rays, max_t, trace_mode=mode, count=True)
        assert np.array_equal(got, want) and n_got == n_want == int((0.0 < max_t).sum())
    _check(rtk, fast, oacc, flat, rays, max_t, what="fast")


# ---- 8. another tree
def test_other_tree_parameters(rtk, ora):
    md, ml, eps = 13, 4, 1e-9                         # test_gpu_tree_params: TREES["d13_l4"] (node array too large for LDS), EPS["1e-9"]
    flat = ora.load_crtscene(SCENE8)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8), max_depth=md, max_leaf_size=ml, eps=eps)
    oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD, eps=eps, max_depth=md, max_leaf=ml)
    assert acc.tree_info().n_nodes * 32 > 48 * 1024
    rays, max_t = segments(flat, N_SEG, seed=1)
    want, steps, _ = _check(rtk, acc, oacc, flat, rays, max_t, what="d13_l4 eps 1e-9")
    assert (steps > 0).sum() >= 500 and ((steps > 0) & (want == 1)).sum() >= 100


# ---- 9. the device variant
def test_device_variant_streams_and_graph(rtk, ora):
    import torch

    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    rays, max_t = segments(flat, N_SEG, seed=9)
    want, _ = occluded_ref(oacc, flat, rays, max_t, BIAS)
    half = N_SEG // 2 + 1                              # odd offsets: no alignment demand on d_out beyond a byte
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_rays = torch.from_numpy(rays).to("cuda")
    d_max_t = torch.from_numpy(max_t).to("cuda")
    out1 = torch.full((N_SEG + 3,), 77, dtype=torch.uint8, device="cuda")
    out2 = torch.full((N_SEG + 3,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    acc.occluded_device(d_rays.data_ptr(), d_max_t.data_ptr(), N_SEG, out1.data_ptr() + 1, BIAS, rtk.TRACE_AUTO, s1.cuda_stream)
    acc.occluded_device(d_rays.data_ptr() + 24 * half, d_max_t.data_ptr() + 4 * half, N_SEG - half, out2.data_ptr() + 1 + half,
                        BIAS, rtk.TRACE_WAVE, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    o1, o2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert np.array_equal(o1[1:N_SEG + 1], want) and o1[0] == 77 and (o1[N_SEG + 1:] == 77).all()
    assert np.array_equal(o2[1 + half:N_SEG + 1], want[half:]) and (o2[:1 + half] == 77).all() and (o2[N_SEG + 1:] == 77).all()
    # recorded in a graph on one stream and replayed once
    out3 = torch.full((N_SEG,), 77, dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        acc.occluded_device(d_rays.data_ptr(), d_max_t.data_ptr(), N_SEG, out3.data_ptr(), BIAS, rtk.TRACE_AUTO,
                            torch.cuda.current_stream().cuda_stream)
    out3.fill_(77)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out3.cpu().numpy(), want)


# ---- 10. the frame is not disturbed
def test_frames_before_and_after_a_batch_are_the_same(rtk, ora):
    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    cfg = rtk.RenderConfig(width=480, height=270, max_ray_depth=10, collect_stats=1)
    rgb0, cn0 = acc.render_frame(cfg)
    rays, max_t = segments(flat, N_SEG, seed=10)
    got, n_int = acc.occluded(rays, max_t, count=True)
    assert n_int >= N_SEG // 2
    rgb1, cn1 = acc.render_frame(cfg)
    assert np.array_equal(rgb0.view(np.uint32), rgb1.view(np.uint32)) and cn0 == cn1
    want, _ = occluded_ref(oacc, flat, rays, max_t, BIAS)
    assert np.array_equal(got, want)


# ---- 11. bad arguments
def test_bad_arguments_leave_the_accel_working(rtk, ora):
    import torch

    acc, oacc, flat = _pair(rtk, ora, SCENE8)
    rays, max_t = segments(flat, 1000, seed=11)
    want, _ = occluded_ref(oacc, flat, rays, max_t, BIAS)
    d_rays, d_max_t = torch.from_numpy(rays).to("cuda"), torch.from_numpy(max_t).to("cuda")
    d_out = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    bad = [dict(trace_mode=m) for m in (rtk.TRACE_GROUP4, rtk.TRACE_GROUP8, rtk.TRACE_GROUP16, rtk.TRACE_STREAM, rtk.TRACE_TWOPASS,
                                        rtk.TRACE_REPACK, -1)]
    bad += [dict(shadow_bias=float("nan")), dict(shadow_bias=float("-inf"))]
    for kw in bad:
        with pytest.raises(rtk.RtkError) as e:
            acc.occluded(rays, max_t, **kw)
        assert e.value.code == rtk.RTK_ERR_INVALID, kw
        with pytest.raises(rtk.RtkError) as e:
            acc.occluded_device(d_rays.data_ptr(), d_max_t.data_ptr(), 1000, d_out.data_ptr(), **kw)
        assert e.value.code == rtk.RTK_ERR_INVALID, kw
    for ptrs in ((0, d_max_t.data_ptr(), d_out.data_ptr()), (d_rays.data_ptr(), 0, d_out.data_ptr()), (d_rays.data_ptr(), d_max_t.data_ptr(), 0)):
        with pytest.raises(rtk.RtkError) as e:
            acc.occluded_device(ptrs[0], ptrs[1], 1000, ptrs[2])
        assert e.value.code == rtk.RTK_ERR_INVALID
    acc.occluded_device(0, 0, 0, 0)
    assert np.array_equal(acc.occluded(rays, max_t), want)
    acc.occluded_device(d_rays.data_ptr(), d_max_t.data_ptr(), 1000, d_out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
