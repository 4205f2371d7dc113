"""rtk_accel_update_geometry: new triangle lists on a live accel (csrc/topology.hip makes the topology tables on the device,
csrc/build.hip the tree), against the CPU oracle built from the same vertices, indices and counts.  "Equal" is bit-equal
throughout (update_checks.py): the tree dump, every field of every hit record, every frame and its ray count.

Every case states what it is about as an assertion on the oracle or on the inputs, so it cannot pass beside its point."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import SCENE5, SCENE8, SCENES
from update_checks import (DEPTH, H, W, _bits, _check_frames, _check_hit_records, _check_hits, _check_tree, _rays, _rtk_scene,
                           _same_frame)

pytestmark = pytest.mark.gpu

HW12_4 = os.path.join(SCENES, "hw12", "scene4.crtscene")
MISS = 0xFFFFFFFF
RAYS = dict(n_cam=(64, 48), n_aimed=800)          # the reduced ray set of test_gpu_update_regimes.py
N_RAYS = 64 * 48 + 800


# ---------------------------------------------------------------- scenes and their triangle lists

def _lists(flat):
    """The triangle list of every mesh."""
    return np.split(flat.indices, np.cumsum(flat.mesh_ntris)[:-1])


def _with_lists(flat, lists, vertices=None):
    """`flat` with other triangle lists (and vertices): what the oracle is built from and what update_geometry is given."""
    lists = [np.asarray(t, np.uint32).reshape(-1, 3) for t in lists]
    return dataclasses.replace(flat, vertices=np.ascontiguousarray(flat.vertices if vertices is None else vertices, np.float32),
                               indices=np.ascontiguousarray(np.concatenate(lists), np.uint32),
                               mesh_ntris=np.array([len(t) for t in lists], np.int32))


def _dragon(flat):
    return int(np.argmax(flat.mesh_ntris))


def _cut(flat, k, mesh=None):
    """The big mesh cut to its first k triangles; the others stay."""
    m = _dragon(flat) if mesh is None else mesh
    lists = _lists(flat)
    lists[m] = lists[m][:k]
    return _with_lists(flat, lists)


def _oracle_of(ora, flat, **tree):
    return ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD, **tree)


def _update(acc, new):
    acc.update_geometry(new.vertices, new.indices, new.mesh_ntris)


def _same_dump(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check(rtk, ora, acc, new, seed, what, min_hits=500, small=False, **tree):
    """Tree (with n_triangles), hit records and frames of `acc` against the oracle of `new`."""
    oacc = _oracle_of(ora, new, **tree)
    dump = _check_tree(acc, oacc, what)
    assert acc.tree_info().n_triangles == int(new.mesh_ntris.sum()) == oacc.num_triangles, what
    if int(new.mesh_ntris.sum()) == 0:                                         # nothing to aim at: the camera rays alone
        rays = np.ascontiguousarray(oacc.camera_rays(64, 48).reshape(-1, 6))
        assert (oacc.intersect(rays, False)["tri"] == MISS).all()
        _check_hit_records(rtk, acc, oacc, rays, what, min_hits=0)
    elif small:
        _check_hits(rtk, acc, oacc, new, seed, what, n_rays=N_RAYS, min_hits=min_hits, **RAYS)
    else:
        _check_hits(rtk, acc, oacc, new, seed, what, min_hits=min_hits)
    _check_frames(rtk, acc, oacc, what)
    return dump, oacc


def _pool(p, seed, lift):
    """p vertices: a bumpy g x g height field over [-4, 4]^2 with g = floor(sqrt(p)), vertex i * g + j at grid point (i, j),
    and what is left over scattered above it."""
    rng = np.random.default_rng(seed)
    g = int(np.sqrt(p))
    xs, zs = np.meshgrid(np.linspace(-4, 4, g), np.linspace(-4, 4, g), indexing="ij")
    grid = np.stack([xs, 0.3 * rng.normal(size=xs.shape) - 1.0 + lift, zs], axis=-1).reshape(-1, 3)
    rest = rng.uniform(-3, 3, size=(p - g * g, 3)) + np.array([0.0, 4.0, 0.0])
    return np.concatenate([grid, rest])


def _soup(ora, n_pool, lists, seed=3, materials=(0, 0), kinds=None, lift=1.5):
    """Two meshes over pools of `n_pool` (a number, or one per mesh) vertices each (_pool; the second `lift` above the first),
    with the given triangle lists."""
    pools = (n_pool, n_pool) if np.isscalar(n_pool) else n_pool
    v = [_pool(p, seed + m, lift * m) for m, p in enumerate(pools)]
    kinds = [ora.MAT_DIFFUSE, ora.MAT_DIFFUSE] if kinds is None else kinds
    c, s_ = np.cos(0.35), np.sin(0.35)
    flat = ora.FlatScene(
        mesh_material=np.asarray(materials, np.int32), mesh_nverts=np.asarray(pools, np.int32), mesh_ntris=np.zeros(2, np.int32),
        vertices=np.concatenate(v).astype(np.float32), indices=np.zeros((0, 3), np.uint32),
        mat_kind=np.asarray(kinds, np.int32), mat_albedo=np.array([[0.8, 0.7, 0.5], [0.3, 0.5, 0.9]], np.float32),
        mat_ior=np.array([1.0, 1.0], np.float32), mat_smooth=np.array([1, 1], np.int32),
        light_pos=np.array([[2, 6, 3]], np.float32), light_intensity=np.array([900], np.float32),
        cam_pos=np.array([0.0, 3.0, 9.0], np.float32), cam_mat=np.array([1, 0, 0, 0, c, -s_, 0, s_, c], np.float32),
        background=np.array([0.1, 0.3, 0.2], np.float32), width=96, height=64, bucket_size=64)
    return _with_lists(flat, lists)


def _random_lists(pools, counts, seed):
    """counts[m] triangles of mesh m's height field (_pool), drawn at random WITH repetition and in no order: a vertex is shared
    by several triangles whose positions in the list have nothing to do with the vertex's, and some triangles are there twice."""
    rng = np.random.default_rng(seed)
    out = []
    for p, n in zip(pools, counts):
        g = int(np.sqrt(p))
        if g < 2:
            out.append(np.zeros((n, 3), np.uint32))                             # (a pool without a cell: every corner is vertex 0)
            continue
        a = rng.integers(0, g - 1, size=n) * g + rng.integers(0, g - 1, size=n)
        lower = rng.integers(0, 2, size=n)[:, None] == 0
        out.append(np.where(lower, np.stack([a, a + 1, a + g], axis=1), np.stack([a + 1, a + g + 1, a + g], axis=1)).astype(np.uint32))
    return out


# ---------------------------------------------------------------- 1. the same topology

@pytest.mark.parametrize("variant", ["host", "device"])
def test_same_topology_gives_the_built_accel(rtk, ora, variant):
    """scene5's own arrays: the device-made tables are the host-made ones, so the accel is the oracle's and a fresh build's.  The
    device variant runs on a caller's stream and the frame behind it on another, with no host wait between."""
    import torch

    flat = ora.load_crtscene(SCENE5)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    fresh = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=DEPTH)
    want = fresh.render_frame(cfg)[0]
    if variant == "host":
        _update(acc, flat)
    else:
        d_v, d_i = torch.from_numpy(flat.vertices).cuda(), torch.from_numpy(flat.indices.view(np.int32)).cuda()
        d_rgb = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for rep in range(2):                                                    # the second time with everything allocated
            acc.update_geometry_device(d_v.data_ptr(), d_i.data_ptr(), flat.mesh_ntris, s1.cuda_stream)
            acc.render_frame_device(cfg, d_rgb.data_ptr(), s2.cuda_stream)
            s2.synchronize()
            assert _same_frame(d_rgb.cpu().numpy(), want), rep
            d_rgb.fill_(float("nan"))
            torch.cuda.synchronize()
    assert _same_dump(acc.tree_dump(), fresh.tree_dump())
    _check(rtk, ora, acc, flat, 11, variant)
    acc.update_vertices(flat.vertices)                                          # the vertices-only update works on the device-made tables
    assert _same_dump(acc.tree_dump(), fresh.tree_dump())
    assert _same_frame(acc.render_frame(cfg)[0], want)


# ---------------------------------------------------------------- 2. the reveal

@pytest.mark.parametrize("k", [0, 1, 10, 63, 64, 65, 4011, 4012])
def test_reveal_of_the_dragon(rtk, ora, k):
    """dragon_slow_load: the dragon of scene5 cut to its first k triangles, the floor stays.  The aimed rays go at the
    triangles there are."""
    flat = ora.load_crtscene(SCENE5)
    assert int(flat.mesh_ntris[_dragon(flat)]) == 4012
    new = _cut(flat, k)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    _update(acc, new)
    _, oacc = _check(rtk, ora, acc, new, 20 + k % 7, k)
    if k <= 65:
        assert oacc.num_nodes == {0: 1, 1: 1, 10: 1, 63: 5, 64: 5, 65: 7}[k]
    if k == 4012:
        assert _same_dump(acc.tree_dump(), rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5)).tree_dump())


# ---------------------------------------------------------------- 3. the order of the triangles

def test_order_of_the_triangles_matters(rtk, ora):
    """The dragon with its triangle list reversed: the same surface, so every t is equal, but the face normals are summed into
    the vertex normals in another order and float addition does not commute.  Stale or unordered incidence lists cannot pass."""
    flat = ora.load_crtscene(SCENE5)
    m = _dragon(flat)
    lists = _lists(flat)
    lists[m] = lists[m][::-1]
    new = _with_lists(flat, lists)
    a, b = ora.Scene(flat).vertex_normals(m), ora.Scene(new).vertex_normals(m)
    assert (_bits(a) != _bits(b)).any(axis=1).sum() >= 1
    o_old, o_new = _oracle_of(ora, flat), _oracle_of(ora, new)
    rays = np.ascontiguousarray(o_new.camera_rays(160, 120).reshape(-1, 6))
    h_old, h_new = o_old.intersect(rays, True), o_new.intersect(rays, True)
    assert np.array_equal(_bits(h_old["t"]), _bits(h_new["t"]))
    assert (_bits(h_old["normal"]) != _bits(h_new["normal"])).any(axis=1).sum() >= 1
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    _update(acc, new)
    _check(rtk, ora, acc, new, 31, "reversed")


# ---------------------------------------------------------------- 4. grow and shrink on one accel

def test_grow_and_shrink_on_one_accel(rtk, ora):
    """8 -> 20,000 -> 3 -> 0 -> 8,193 triangles over a pool of vertices: 20,000 outgrows every per-triangle buffer and the
    reference lists, 0 is the accel without triangles.  Then the vertices move under the last topology."""
    pool = 6000
    base = _soup(ora, pool, [np.zeros((0, 3)), np.zeros((0, 3))])
    start = _with_lists(base, _random_lists((pool, pool), (5, 3), 1))
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, start))
    assert acc.tree_info().n_triangles == 8
    new = None
    for i, counts in enumerate([(5, 3), (12000, 8000), (1, 2), (0, 0), (193, 8000)]):
        new = _with_lists(base, _random_lists((pool, pool), counts, 10 + i))
        _update(acc, new)
        assert acc.tree_info().n_triangles == sum(counts)
        _check(rtk, ora, acc, new, 40 + i, counts, min_hits=500 if sum(counts) > 100 else 0, small=True)
    moved = dataclasses.replace(new, vertices=(new.vertices * np.float32([1.0, 1.7, 0.8]) + np.float32([0.3, 0.0, 0.0])).astype(np.float32))
    acc.update_vertices(moved.vertices)
    _check(rtk, ora, acc, moved, 47, "moved", small=True)


# ---------------------------------------------------------------- 5. boundaries

@pytest.mark.parametrize("total", [63, 64, 65, 255, 256, 257, 8191, 8192])
def test_triangle_totals_at_the_block_and_chunk_boundaries(rtk, ora, total):
    """One thread per triangle in blocks of 256, waves of 64, and the build's trips of 8,192 references."""
    pool = 900
    base = _soup(ora, pool, [np.zeros((0, 3)), np.zeros((0, 3))])
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, _with_lists(base, _random_lists((pool, pool), (2, 2), 1))))
    new = _with_lists(base, _random_lists((pool, pool), (total - total // 3, total // 3), total))
    _update(acc, new)
    _check(rtk, ora, acc, new, total, total, min_hits=100, small=True)


@pytest.mark.parametrize("n_verts", [1, 255, 256, 257, 65536, 65537])
def test_vertex_totals_at_the_sort_keys_bit_boundaries(rtk, ora, n_verts):
    """The incidence sort takes as many key bits as the vertex count needs; a triangle uses the last vertex."""
    pools = (n_verts - n_verts // 2, n_verts // 2)
    lists = _random_lists(pools, (300 if pools[0] > 1 else 2, 200 if pools[1] else 0), n_verts)
    if pools[1]:
        lists[1][-1] = [pools[1] - 1, 0, pools[1] // 2]                         # the last vertex of all
    base = _soup(ora, pools, [np.zeros((0, 3)), np.zeros((0, 3))], seed=n_verts)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, _with_lists(base, [lists[0][:1], lists[1][:1]])))
    new = _with_lists(base, lists)
    assert int(new.indices[-1, 0]) + int(pools[0]) == n_verts - 1 or n_verts == 1
    _update(acc, new)
    if n_verts == 1:                                                            # a point root: the product's departure, so a fresh accel is the yardstick
        assert _same_dump(acc.tree_dump(), rtk.KdTreeSimdAccel(_rtk_scene(rtk, new)).tree_dump())
        assert acc.tree_info().n_triangles == 2
    else:
        _check(rtk, ora, acc, new, n_verts % 97, n_verts, min_hits=20, small=True)


def test_fan_duplicates_unused_vertices_and_an_empty_mesh_between(rtk, ora):
    """2,000 triangles on one vertex; [a, a, b] and [a, a, a]; a pool most of which nothing uses; and three meshes of which the
    middle one has no triangles (the per-triangle search in the prefix sums must skip it)."""
    n = 2000
    ang = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    rim = np.stack([3.4 * np.cos(ang), 0.3 * np.sin(5 * ang) - 1.0, 3.4 * np.sin(ang)], axis=1)
    fan_v = np.concatenate([[[0.0, 0.5, 0.0]], rim, np.random.default_rng(5).uniform(-9, 9, size=(500, 3))])      # 500 unused
    fan_t = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1)
    fan_t = np.concatenate([fan_t, [[3, 3, 7], [9, 9, 9], fan_t[0]]])
    mid_v = np.random.default_rng(6).uniform(-2, 2, size=(40, 3))
    quad_v = np.array([[-6, -2, -6], [6, -2, -6], [6, -2, 6], [-6, -2, 6]], np.float64)
    quad_t = np.array([[0, 2, 1], [0, 3, 2]])
    c, s_ = np.cos(0.35), np.sin(0.35)
    base = ora.FlatScene(
        mesh_material=np.array([0, 1, 1], np.int32), mesh_nverts=np.array([len(fan_v), len(mid_v), 4], np.int32),
        mesh_ntris=np.array([1, 1, 1], np.int32), vertices=np.concatenate([fan_v, mid_v, quad_v]).astype(np.float32),
        indices=np.array([[0, 1, 2], [0, 1, 2], [0, 2, 1]], np.uint32),
        mat_kind=np.array([ora.MAT_DIFFUSE, ora.MAT_DIFFUSE], np.int32), mat_albedo=np.array([[0.8, 0.7, 0.5], [0.3, 0.5, 0.9]], np.float32),
        mat_ior=np.array([1.0, 1.0], np.float32), mat_smooth=np.array([1, 1], np.int32),
        light_pos=np.array([[2, 6, 3]], np.float32), light_intensity=np.array([900], np.float32),
        cam_pos=np.array([0.0, 3.0, 9.0], np.float32), cam_mat=np.array([1, 0, 0, 0, c, -s_, 0, s_, c], np.float32),
        background=np.array([0.1, 0.3, 0.2], np.float32), width=96, height=64, bucket_size=64)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, base))
    new = _with_lists(base, [fan_t, np.zeros((0, 3)), quad_t])
    assert new.mesh_ntris.tolist() == [n + 3, 0, 2]
    _update(acc, new)
    _, oacc = _check(rtk, ora, acc, new, 51, "fan", small=True)
    rays = _rays(oacc, new, 52, **RAYS)
    assert set(np.unique(oacc.intersect(rays, False)["mesh"][oacc.intersect(rays, False)["tri"] != MISS]).tolist()) == {0, 2}


# ---------------------------------------------------------------- 6. triangles change mesh

def test_triangles_change_mesh(rtk, ora):
    """Two meshes of different materials over the same pool positions: twelve triangles whose split between the meshes moves
    from (5, 7) to (7, 5) to (0, 12).  `mesh` of every hit record (and the colours of the frames) follow."""
    pool = 36
    base = _soup(ora, pool, [np.zeros((0, 3)), np.zeros((0, 3))], materials=(0, 1), kinds=[ora.MAT_DIFFUSE, ora.MAT_REFLECTIVE])
    v = base.vertices.copy()
    v[pool:] = v[:pool]                                                         # the same positions under both meshes
    base = dataclasses.replace(base, vertices=v)
    g = 6
    cells = np.array([i * g + j for i in range(1, 4) for j in range(1, 5)])     # twelve different triangles of the 6 x 6 field
    tris = np.stack([cells, cells + 1, cells + g], axis=1).astype(np.uint32)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, _with_lists(base, [tris[:5], tris[5:]])))
    seen = []
    for i, a in enumerate((5, 7, 0)):
        new = _with_lists(base, [tris[:a], tris[a:]])
        _update(acc, new)
        _, oacc = _check(rtk, ora, acc, new, 60 + i, a, min_hits=100, small=True)
        rays = _rays(oacc, new, 60 + i, **RAYS)
        ref = oacc.intersect(rays, False)
        hit = ref["tri"] != MISS
        assert np.array_equal(ref["mesh"][hit], (ref["tri"][hit] >= a).astype(np.uint32))
        seen.append(ref["mesh"][hit].copy())
    assert set(seen[0].tolist()) == {0, 1} and set(seen[2].tolist()) == {1}


# ---------------------------------------------------------------- 7. textures

def test_textured_quads_follow_their_triangles(rtk, ora):
    """hw12/scene4, four textured quads (one a bitmap): each mesh's two triangles swapped leaves the frame as it was, which a
    stale per-triangle uv table does not reproduce; then only the second triangle of each."""
    flat = ora.load_crtscene(HW12_4)
    assert flat.mesh_ntris.tolist() == [2, 2, 2, 2] and flat.tex_kind is not None and len(flat.tex_kind) > 0
    swapped = _with_lists(flat, [t[::-1] for t in _lists(flat)])
    thinned = _with_lists(flat, [t[1:] for t in _lists(flat)])
    f0 = _oracle_of(ora, flat).render(W, H, 1, DEPTH, 0)[0]
    f1 = _oracle_of(ora, swapped).render(W, H, 1, DEPTH, 0)[0]
    f2 = _oracle_of(ora, thinned).render(W, H, 1, DEPTH, 0)[0]
    assert _same_frame(f0, f1)
    assert (_bits(f0) != _bits(f2)).any(axis=2).sum() >= 600                           # (639 of 6,144 on the oracle)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(HW12_4))
    for name, new in (("swapped", swapped), ("thinned", thinned), ("back", flat)):
        _update(acc, new)
        _check(rtk, ora, acc, new, 70, name, min_hits=100, small=True)


# ---------------------------------------------------------------- 8. RTK_TRAVERSAL_FAST with a transmissive mesh

@pytest.mark.parametrize("k", [1000, 0])
def test_fast_traversal_with_a_transmissive_mesh(rtk, ora, k):
    """hw11/scene8 under RTK_TRAVERSAL_FAST: the refractive dragon cut to k triangles.  Ties keep FAST off the oracle, so its
    yardstick is a fresh FAST accel of the same arrays (tree dump, hits, occlusion bytes, frames); the parity mode is compared
    with the oracle."""
    flat = ora.load_crtscene(SCENE8)
    m = _dragon(flat)
    assert flat.mat_kind[flat.mesh_material[m]] == ora.MAT_REFRACTIVE
    new = _cut(flat, k)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8), traversal=rtk.TRAVERSAL_FAST)
    acc.render_frame(rtk.RenderConfig(width=W, height=H, max_ray_depth=DEPTH))  # the old geometry has been on the device and rendered
    _update(acc, new)
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, new), traversal=rtk.TRAVERSAL_FAST)
    oacc = _oracle_of(ora, new)
    _check_tree(acc, oacc, k)
    assert _same_dump(acc.tree_dump(), fresh.tree_dump())
    for mode in (rtk.TRACE_AUTO, rtk.TRACE_GROUP4, rtk.TRACE_STREAM):
        cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=10, trace_mode=mode)
        for rep in range(2):
            got, cn = acc.render_frame(cfg)
            want, wn = fresh.render_frame(cfg)
            assert _same_frame(got, want), (mode, rep)
            assert mode == rtk.TRACE_AUTO or cn["rays"] == wn["rays"], (mode, rep)      # (test_gpu_update.py: AUTO's trial may be a frame apart)
    rays = _rays(oacc, new, 9)
    max_t = np.random.default_rng(2).uniform(0.5, 40.0, size=rays.shape[0]).astype(np.float32)
    for mode in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_AUTO):
        assert acc.occluded(rays, max_t, trace_mode=mode).tobytes() == fresh.occluded(rays, max_t, trace_mode=mode).tobytes(), mode
        for cull in (False, True):
            g, w = acc.intersect(rays, cull, mode), fresh.intersect(rays, cull, mode)
            assert g.tobytes() == w.tobytes(), (mode, cull)
    par = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    _update(par, new)
    _check_tree(par, oacc, ("parity", k))
    _check_hits(rtk, par, oacc, new, 9, ("parity", k))
    ref, ocn = oacc.render(W, H, 1, 10, 0)
    got, cn = par.render_frame(rtk.RenderConfig(width=W, height=H, max_ray_depth=10))
    assert _same_frame(got, ref) and cn["rays"] == ocn["rays"]


# ---------------------------------------------------------------- 9. refused

def test_refused_updates_change_nothing(rtk, ora):
    """The device variant learns of an index outside its own mesh and of a non-finite vertex from the flags it reads back; the
    host variant finds a negative count, triangles on a mesh without vertices and index 0xFFFFFFFF before it touches the device.
    The bad device index equals mesh 0's vertex count with mesh 1 behind it: inside the concatenated vertex array."""
    import torch

    pool = 50
    lists = _random_lists((pool, pool), (30, 40), 4)
    base = _soup(ora, pool, lists)
    c, s_ = np.cos(0.35), np.sin(0.35)
    flat = dataclasses.replace(base, mesh_material=np.array([0, 1, 0], np.int32), mesh_nverts=np.array([pool, pool, 0], np.int32),
                               mesh_ntris=np.array([30, 40, 0], np.int32))      # a third mesh without vertices
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    start = _with_lists(flat, [lists[0][:20], lists[1][:25], np.zeros((0, 3))])
    _update(acc, start)
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=DEPTH)
    before, frame = acc.tree_dump(), acc.render_frame(cfg)[0]
    stream = torch.cuda.current_stream().cuda_stream

    def refused(call):
        with pytest.raises(rtk.RtkError) as e:
            call()
        assert e.value.code == rtk.RTK_ERR_INVALID
        assert _same_dump(before, acc.tree_dump()) and acc.tree_info().n_triangles == 45
        assert _same_frame(acc.render_frame(cfg)[0], frame)

    bad_i = flat.indices.copy()
    bad_i[29, 2] = pool                                                         # mesh 0's last triangle: one past its own vertices
    d_v, d_i = torch.from_numpy(flat.vertices).cuda(), torch.from_numpy(bad_i.view(np.int32)).cuda()
    torch.cuda.synchronize()
    refused(lambda: acc.update_geometry_device(d_v.data_ptr(), d_i.data_ptr(), flat.mesh_ntris, stream))
    bad_v = flat.vertices.copy()
    bad_v[-1, 2] = np.inf
    d_bv, d_gi = torch.from_numpy(bad_v).cuda(), torch.from_numpy(flat.indices.view(np.int32)).cuda()
    torch.cuda.synchronize()
    refused(lambda: acc.update_geometry_device(d_bv.data_ptr(), d_gi.data_ptr(), flat.mesh_ntris, stream))
    refused(lambda: acc.update_geometry(flat.vertices, bad_i, flat.mesh_ntris))
    refused(lambda: acc.update_geometry(bad_v, flat.indices, flat.mesh_ntris))
    refused(lambda: acc.update_geometry(flat.vertices, flat.indices, np.array([30, -1, 0], np.int32)))
    refused(lambda: acc.update_geometry(flat.vertices, np.concatenate([flat.indices, [[0, 0, 0]]]).astype(np.uint32), np.array([30, 40, 1], np.int32)))
    huge = flat.indices.copy()
    huge[0, 0] = 0xFFFFFFFF
    refused(lambda: acc.update_geometry(flat.vertices, huge, flat.mesh_ntris))
    _update(acc, flat)                                                          # and the accel stays usable
    _check(rtk, ora, acc, flat, 81, "after the refusals", min_hits=100, small=True)
    acc.update_geometry_device(d_v.data_ptr(), d_gi.data_ptr(), flat.mesh_ntris, stream)
    _check_tree(acc, _oracle_of(ora, flat), "device variant after the refusals")
