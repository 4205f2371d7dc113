"""GPU parity away from the defaults the rest of the suite builds with: other kd-tree shapes (max_depth, max_leaf_size), other
eps values and other scene scales, each against the oracle built with the same three values.

On the test scenes the default tree (8 / 64) has at most 188 nodes and 87 leaves, so the hierarchical wave walk (more leaves
than the leaf list holds), node arrays that do not fit in LDS, a root that is a leaf, leaves below the bundle-culling minimum
and whole accels without bundle culling never run elsewhere.  Every tree case here asserts that it reaches the branch it
is named for, also without a GPU (test_tree_cases_reach_their_branches).

The last part is the empty-leaf case of the per-lane walk: RTK_TRAVERSAL_FAST's opaque-only occlusion tree keeps every node
and gives leaves that held only transmissive triangles a count of 0; walked per lane (the streaming pipeline's deep levels),
such a leaf must be stepped over, not end the walk."""
import dataclasses
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import CONFIG_SCENES, SCENE5
from test_gpu_parity import FRAME_MODES, MODES, _bits, _boundary_rays, _mixed_rays
from test_random_scenes import _rtk_scene, _same_frame

# Limits of the product that pick a branch.  Keep in step with the sources they cite.
K_LIST_MAX_LEAVES = 512            # trace.hip.hpp kListMaxLeaves: trees with more leaves keep the hierarchical wave walk
K_MAX_NODE_LDS_BYTES = 48 * 1024   # kernels.hpp kMaxNodeLdsBytes: larger node arrays are read from global memory, not LDS
DEV_NODE_BYTES = 32                # sizeof(DevNode), rtk_internal.hpp
K_BUNDLE_MIN_TRIS = 4              # trace.hip.hpp kBundleMinTris: smaller leaves are tested triangle by triangle
K_BUNDLE_LIMIT = 1.0e9             # trace.hip.hpp kBundleLimit: an accel with a larger v0 / e1 / e2 coordinate never bundle-culls (api.hip coords_small)
PASS_TRIS = 64                     # triangles per pass of the wave's leaf loop

FLT_MIN = 1.17549435e-38           # the smallest eps rtk_accel_build accepts

TREES = {                          # name: (max_depth, max_leaf_size)
    "root_leaf": (0, 64),
    "d12_l8": (12, 8),
    "d13_l4": (13, 4),
    "d16_l1": (16, 1),
    "long_leaves": (8, 1000),
}
# the branches each (tree, scene) must reach; see _reached
CLAIMS = {
    "root_leaf": {s: {"root_leaf", "long_leaves"} for s in CONFIG_SCENES},
    "d12_l8": {"scene5": {"hier_walk"}, "scene8": set(), "hw15_scene2": set()},
    "d13_l4": {s: {"hier_walk", "global_nodes"} for s in CONFIG_SCENES},
    "d16_l1": {s: {"hier_walk", "global_nodes", "small_leaves"} for s in CONFIG_SCENES},
    "long_leaves": {s: {"long_leaves"} for s in CONFIG_SCENES},
}
DEPTH = {"scene5": 5, "scene8": 10, "hw15_scene2": 5}

EPS = {"flt_min": FLT_MIN, "1e-9": 1e-9, "1e-3": 1e-3, "0.25": 0.25}   # FLT_MIN: bundle_misses bounds 1/det by about 2^126
EPS_SCENES = ("scene5", "hw15_scene2")

SCALES = (1e-2, 1e3, 3e7, 6e7, 1e8)
SCALE_SCENES = ("scene5", "hw15_scene2")
BIAS = 1e-4                        # RenderConfig's default shadow / reflection / refraction bias


def _reached(acc):
    ti = acc.tree_info()
    _, link, _ = acc.tree_dump()
    leaf = (link[:, 0] < 0) & (link[:, 1] < 0)
    counts = link[leaf, 3]
    r = set()
    if ti.n_leaves > K_LIST_MAX_LEAVES:
        r.add("hier_walk")
    if ti.n_nodes * DEV_NODE_BYTES > K_MAX_NODE_LDS_BYTES:
        r.add("global_nodes")
    if ti.n_nodes == 1:
        r.add("root_leaf")
    if (counts < K_BUNDLE_MIN_TRIS).sum() * 4 >= ti.n_leaves and (counts == 1).any():
        r.add("small_leaves")                                                  # a quarter of the leaves or more, single triangles among them
    if ti.max_leaf_refs > 8 * PASS_TRIS:
        r.add("long_leaves")                                                   # more than eight 64-triangle passes (sliced leaves)
    return r


def _tree_pair(rtk, ora, scene, tree, **kw):
    md, ml = TREES[tree]
    path = CONFIG_SCENES[scene]
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path), max_depth=md, max_leaf_size=ml, **kw)
    assert CLAIMS[tree][scene] <= _reached(acc), (tree, scene, _reached(acc))
    oacc = ora.Accel(ora.Scene(ora.load_crtscene(path)), ora.ACCEL_KD_SIMD, max_depth=md, max_leaf=ml)
    return acc, oacc


@contextmanager
def _env(**kv):
    """Knobs are read once, when an accel is built: set them around the build only."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ray_sets(flat, seed, n=20_000):
    return np.concatenate([_mixed_rays(flat, n, seed), _boundary_rays(flat, n, seed + 1)])


def _assert_hits_equal(got, ref, what):
    assert np.array_equal(got["tri"], ref["tri"]), what
    assert np.array_equal(got["mesh"], ref["mesh"]), what
    for f in ("t", "u", "v"):
        assert np.array_equal(_bits(got[f]), _bits(ref[f])), (what, f)
    hit = ref["tri"] != 0xFFFFFFFF
    gn, rn = got["normal"][hit], ref["normal"][hit]
    assert np.array_equal(np.isnan(gn), np.isnan(rn)), what
    assert np.array_equal(_bits(np.nan_to_num(gn)), _bits(np.nan_to_num(rn))), what


def _frames_match(rtk, acc, oacc, w, h, spp, depth, diffuse=0, modes=tuple(FRAME_MODES), bias=BIAS):
    """Every frame twice: the second one runs in the cost-feedback block order."""
    ref, ocn = oacc.render(w, h, spp, depth, diffuse, shadow_bias=bias, reflection_bias=bias, refraction_bias=bias)
    assert np.isfinite(ref).any()
    for mode in modes:
        if mode == "twopass" and spp != 1:
            continue
        cfg = rtk.RenderConfig(width=w, height=h, spp=spp, max_ray_depth=depth, diffuse_rays=diffuse, trace_mode=FRAME_MODES[mode],
                               shadow_bias=bias, reflection_bias=bias, refraction_bias=bias)
        for rep in range(2):
            rgb, cn = acc.render_frame(cfg)
            assert cn["rays"] == ocn["rays"], (mode, rep)
            assert _same_frame(rgb, ref), (mode, rep, float(np.nanmax(np.abs(rgb - ref))))
    return ocn


# ---------------------------------------------------------------- tree shapes

@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("scene", list(CONFIG_SCENES))
def test_tree_cases_reach_their_branches(rtk, ora, scene, tree):
    """No GPU needed: the host build alone decides which branches a tree takes; the product's tree is the oracle's."""
    acc, oacc = _tree_pair(rtk, ora, scene, tree)
    ti = acc.tree_info()
    assert (ti.n_nodes, ti.n_leaf_refs) == (oacc.num_nodes, oacc.num_leaf_refs)


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("scene", list(CONFIG_SCENES))
def test_tree_intersect_matches_oracle(rtk, ora, scene, tree, cull):
    acc, oacc = _tree_pair(rtk, ora, scene, tree)
    rays = _ray_sets(oacc.scene.flat, seed=len(scene) * 7 + TREES[tree][0])
    ref = oacc.intersect(rays, cull)
    assert (ref["tri"] != 0xFFFFFFFF).sum() > 10_000
    for mode in MODES:
        _assert_hits_equal(acc.intersect(rays, cull, MODES[mode]), ref, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,tree", [("scene5", "d13_l4"), ("hw15_scene2", "d16_l1")])
def test_large_shuffled_batch_on_deep_trees(rtk, ora, scene, tree):
    """2^18 camera rays in random order on a tree past both the leaf-list and the LDS limit: AUTO (which probes and sorts) and
    REPACK give WAVE's bytes, and a sample is the oracle's."""
    acc, oacc = _tree_pair(rtk, ora, scene, tree)
    n = 1 << 18
    cam = acc.camera_rays(rtk.RenderConfig(width=512, height=512), 0).reshape(-1, 6)
    assert cam.shape[0] == n
    rays = np.ascontiguousarray(cam[np.random.default_rng(3).permutation(n)], dtype=np.float32)
    ref = acc.intersect(rays, True, MODES["wave"])
    assert (ref["tri"] != 0xFFFFFFFF).sum() > n // 8
    for mode in ("auto", "repack"):
        assert acc.intersect(rays, True, MODES[mode]).tobytes() == ref.tobytes(), mode
    k = 30_000
    _assert_hits_equal(ref[:k], oacc.intersect(rays[:k], True), "oracle sample")


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("scene", list(CONFIG_SCENES))
def test_tree_frames_match_oracle(rtk, ora, scene, tree):
    acc, oacc = _tree_pair(rtk, ora, scene, tree)
    _frames_match(rtk, acc, oacc, 256, 144, 1, DEPTH[scene])


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_tree_gi_frames_match_oracle(rtk, ora, tree):
    acc, oacc = _tree_pair(rtk, ora, "hw15_scene2", tree)
    _frames_match(rtk, acc, oacc, 96, 96, 4, 5, diffuse=1)


@pytest.mark.gpu
def test_tree_work_counters_match_oracle(rtk, ora):
    """collect_stats=1 on a tree past the leaf-list limit: the per-ray work of the reference algorithm, in every frame mode."""
    acc, oacc = _tree_pair(rtk, ora, "scene5", "d13_l4")
    md, ml = TREES["d13_l4"]
    _, ocn = ora.Accel(oacc.scene, ora.ACCEL_KD_SIMD, max_depth=md, max_leaf=ml, W=16).render(320, 184, 1, 5, 0)
    for mode in FRAME_MODES.values():
        _, cn = acc.render_frame(rtk.RenderConfig(width=320, height=184, max_ray_depth=5, trace_mode=mode, collect_stats=True))
        for k in ("rays", "hits", "nodes", "boxpass", "leaves", "tris"):
            assert cn[k] == ocn[k], (mode, k)
        assert cn["packets16"] == ocn["packets"], mode


# ---------------------------------------------------------------- eps

@pytest.mark.gpu
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("eps", list(EPS))
@pytest.mark.parametrize("scene", EPS_SCENES)
def test_eps_intersect_matches_oracle(rtk, ora, scene, eps, cull):
    path = CONFIG_SCENES[scene]
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path), eps=EPS[eps])
    osc = ora.Scene(ora.load_crtscene(path))
    oacc = ora.Accel(osc, ora.ACCEL_KD_SIMD, eps=EPS[eps])
    rays = _ray_sets(osc.flat, seed=31 + len(scene))
    ref = oacc.intersect(rays, cull)
    assert (ref["tri"] != 0xFFFFFFFF).sum() > 10_000
    if EPS[eps] >= 1e-3:                                                       # the value decides something on these rays
        base = ora.Accel(osc, ora.ACCEL_KD_SIMD).intersect(rays, cull)
        assert (base["tri"] != ref["tri"]).sum() > 100
    for mode in MODES:
        _assert_hits_equal(acc.intersect(rays, cull, MODES[mode]), ref, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("eps", list(EPS))
@pytest.mark.parametrize("scene", EPS_SCENES)
def test_eps_frames_match_oracle(rtk, ora, scene, eps):
    path = CONFIG_SCENES[scene]
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path), eps=EPS[eps])
    oacc = ora.Accel(ora.Scene(ora.load_crtscene(path)), ora.ACCEL_KD_SIMD, eps=EPS[eps])
    _frames_match(rtk, acc, oacc, 200, 112, 1, DEPTH[scene], modes=("group4", "stream", "lane"))


# ---------------------------------------------------------------- scene scale

def _scaled(flat, s):
    """Vertices, camera and lights times s; intensities times s^2, so that a light lights its surroundings as before."""
    return dataclasses.replace(
        flat, vertices=(flat.vertices.astype(np.float64) * s).astype(np.float32),
        cam_pos=(flat.cam_pos.astype(np.float64) * s).astype(np.float32),
        light_pos=(flat.light_pos.astype(np.float64) * s).astype(np.float32),
        light_intensity=(flat.light_intensity.astype(np.float64) * s * s).astype(np.float32))


def _leaf_coord_max(flat):
    """Largest |coordinate| of any triangle's v0, e1 = v1 - v0, e2 = v2 - v0: what api.hip compares with kBundleLimit."""
    starts = np.concatenate([[0], np.cumsum(flat.mesh_nverts)[:-1]])
    g = flat.indices.astype(np.int64) + starts[np.repeat(np.arange(len(flat.mesh_ntris)), flat.mesh_ntris)][:, None]
    v0, v1, v2 = (flat.vertices[g[:, k]] for k in range(3))
    return float(max(np.abs(v0).max(), np.abs(v1 - v0).max(), np.abs(v2 - v0).max()))


def _scaled_rays(flat, s, seed):
    """The ray sets of the unscaled scene with origins times s and directions of length 1e-3, 1 and 1e3 in turn."""
    rays = _ray_sets(flat, seed).astype(np.float64)
    d = rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    d *= np.array([1e-3, 1.0, 1e3])[np.arange(len(d)) % 3][:, None]
    return np.ascontiguousarray(np.concatenate([rays[:, :3] * s, d], axis=1).astype(np.float32))


def _scaled_pair(rtk, ora, scene, s):
    flat = _scaled(ora.load_crtscene(CONFIG_SCENES[scene]), s)
    return rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat)), ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD), flat


def test_scales_straddle_the_bundle_limit(ora):
    """No GPU needed: on scene5, 3e7 keeps every leaf coordinate under kBundleLimit (bundle culling on), 6e7 and 1e8 do not (off)."""
    flat = ora.load_crtscene(SCENE5)
    assert 0.8 * K_BUNDLE_LIMIT < _leaf_coord_max(_scaled(flat, 3e7)) < K_BUNDLE_LIMIT
    assert K_BUNDLE_LIMIT < _leaf_coord_max(_scaled(flat, 6e7)) < _leaf_coord_max(_scaled(flat, 1e8))


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("scene", SCALE_SCENES)
def test_scaled_intersect_matches_oracle(rtk, ora, scene, s, cull):
    unit = ora.load_crtscene(CONFIG_SCENES[scene])
    acc, oacc, _ = _scaled_pair(rtk, ora, scene, s)
    seed = 47 + len(scene)
    rays = _scaled_rays(unit, s, seed)
    ref = oacc.intersect(rays, cull)
    assert (ref["tri"] != 0xFFFFFFFF).sum() > 5_000
    if s == 1e-2:                                                              # determinants near eps: the hit set is not scale 1's
        base = ora.Accel(ora.Scene(unit), ora.ACCEL_KD_SIMD).intersect(_scaled_rays(unit, 1.0, seed), cull)
        assert (base["tri"] != ref["tri"]).sum() > 100
    for mode in MODES:
        _assert_hits_equal(acc.intersect(rays, cull, MODES[mode]), ref, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("scene", SCALE_SCENES)
def test_scaled_frames_match_oracle(rtk, ora, scene, s):
    acc, oacc, _ = _scaled_pair(rtk, ora, scene, s)
    _frames_match(rtk, acc, oacc, 200, 112, 1, DEPTH[scene], modes=("group4", "stream", "wave"), bias=BIAS * s)


@pytest.mark.gpu
def test_frames_without_bundle_culling_match_oracle(rtk, ora):
    """RTK_BUNDLE_CULL=0 at build time: the non-bundled wave walk of the GROUP / WAVE frames, at scale 1."""
    flat = ora.load_crtscene(SCENE5)
    with _env(RTK_BUNDLE_CULL=0):
        acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    _frames_match(rtk, acc, ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD), 320, 184, 1, 5, modes=("group4", "stream", "wave"))


# ---------------------------------------------------------------- empty leaves in the per-lane walk

def _layered_scene(ora, seed=5):
    """An opaque floor, an opaque blocker above it, a dense soup of glass triangles above the blocker and a light above all.
    The scene box's y midpoint (the depth-1 split; depth 0 splits x) lies between blocker and soup, and the upper half is
    walked first (child1 before child0), so on a shadow ray from under the blocker the glass-only leaves come first."""
    rng = np.random.default_rng(seed)
    floor = np.array([[-6, -2, -6], [6, -2, -6], [6, -2, 6], [-6, -2, 6]], np.float32)
    blocker = np.array([[-2.5, 0.5, -2.5], [2.5, 0.5, -2.5], [2.5, 0.5, 2.5], [-2.5, 0.5, 2.5]], np.float32)
    k = 1500
    centres = rng.uniform([-6, 3.5, -6], [6, 5.5, 6], size=(k, 1, 3))
    soup = (centres + rng.uniform(-0.35, 0.35, size=(k, 3, 3))).reshape(-1, 3).astype(np.float32)
    quad = np.array([[0, 2, 1], [0, 3, 2]], np.uint32)
    c, s_ = np.cos(0.35), np.sin(0.35)
    return ora.FlatScene(
        mesh_material=np.array([0, 1, 2], np.int32), mesh_nverts=np.array([4, 4, 3 * k], np.int32),
        mesh_ntris=np.array([2, 2, k], np.int32), vertices=np.concatenate([floor, blocker, soup]),
        indices=np.concatenate([quad, quad, np.arange(3 * k, dtype=np.uint32).reshape(k, 3)]),
        mat_kind=np.array([ora.MAT_DIFFUSE, ora.MAT_DIFFUSE, ora.MAT_REFRACTIVE], np.int32),
        mat_albedo=np.array([[0.8, 0.8, 0.8], [0.7, 0.3, 0.2], [0.9, 0.95, 1.0]], np.float32),
        mat_ior=np.array([1.0, 1.0, 1.5], np.float32), mat_smooth=np.zeros(3, np.int32),
        light_pos=np.array([[0.3, 9.0, 0.4]], np.float32), light_intensity=np.array([3000.0], np.float32),
        cam_pos=np.array([0.0, 2.5, 11.0], np.float32), cam_mat=np.array([1, 0, 0, 0, c, -s_, 0, s_, c], np.float32),
        background=np.array([0.1, 0.3, 0.2], np.float32), width=320, height=240, bucket_size=64)


def test_layered_scene_puts_glass_only_leaves_first(rtk, ora):
    """No GPU needed: the depth-1 split lies between blocker and soup, and the first leaves in traversal order hold only glass."""
    flat = _layered_scene(ora)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    box, link, refs = acc.tree_dump()
    lo, hi = box[0, 1], box[0, 4]
    assert 0.5 < lo + (hi - lo) / 2 < 3.5
    glass_first = 4                                                            # global triangle ids 0-3 are floor and blocker
    order, stack = [], [0]                                                     # flatten's order: node, child1 subtree, child0 subtree
    while stack:
        n = stack.pop()
        if link[n, 0] < 0 and link[n, 1] < 0:
            order.append(refs[link[n, 2]:link[n, 2] + link[n, 3]])
        for c in (link[n, 0], link[n, 1]):
            if c >= 0:
                stack.append(c)
    assert (order[0] >= glass_first).all() and (order[1] >= glass_first).all()
    assert sum(int((leaf >= glass_first).all()) for leaf in order) >= len(order) // 3


@pytest.mark.gpu
@pytest.mark.parametrize("deep_mode", [1, 0], ids=["lane", "auto"])
def test_fast_occlusion_steps_over_glass_only_leaves(rtk, ora, deep_mode):
    """RTK_TRAVERSAL_FAST with every level of the streaming pipeline "deep" (per-lane walk, directly or through AUTO's hand-over):
    a leaf left empty in the opaque-only occlusion tree must not end a shadow ray's walk before the blocker under it."""
    import torch

    flat = _layered_scene(ora)
    sc = _rtk_scene(rtk, flat)
    w, h = flat.width, flat.height
    st = torch.cuda.current_stream().cuda_stream

    def frame(acc):
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        acc.render_frame_device(rtk.RenderConfig(width=w, height=h, max_ray_depth=5, trace_mode=FRAME_MODES["stream"]), out.data_ptr(), st)
        torch.cuda.synchronize()
        return out

    ref = frame(rtk.KdTreeSimdAccel(sc))
    ora_ref, _ = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(w, h, 1, 5, 0)
    assert _same_frame(ref.cpu().numpy(), ora_ref)
    with _env(RTK_STREAM_DEEP_LEVEL=0, RTK_STREAM_DEEP_MODE=deep_mode):
        fast = frame(rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST))
    differing = int((fast != ref).any(dim=2).sum())
    print(f"deep mode {deep_mode}: {differing} of {w * h} pixels differ from the parity frame")
    assert differing <= w * h // 10_000, differing
