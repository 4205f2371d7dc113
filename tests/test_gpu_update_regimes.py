"""rtk_accel_update_vertices in the regimes test_gpu_update.py does not reach: levels of the device build wider than one trip
of the workgroup, both capacity retries, lists that end exactly on a chunk, an update that moves the scene across the
bundle-culling limit, signed zeros among the extremes of the root box, vertices no triangle uses, one vertex with thousands
of triangles, roots without extent, the accel without triangles.

Every case states its regime as an assertion on the CPU oracle's tree of the same vertices (or on the inputs), so that it
cannot pass without entering the regime: if a constant of the product moves, the precondition fails and says so.  The
constants below are the product's; keep them in step with the sources they cite."""
import dataclasses

import numpy as np
import pytest

from conftest import SCENE5
from test_gpu_tree_params import K_BUNDLE_LIMIT, _leaf_coord_max, _scaled_rays
from update_checks import (_bits, _check_frames, _check_hit_records, _check_hits, _check_tree, _oracle, _rays, _rtk_scene)

pytestmark = pytest.mark.gpu

K_TREE_THREADS = 1024              # build.hip kTreeThreads: nodes of a level per trip of k_build_tree's child loop
K_CHUNK = 8192                     # build.hip kChunk: references per trip of sweep_level
RAYS = dict(n_cam=(64, 48), n_aimed=800)
N_RAYS = 64 * 48 + 800
MISS = 0xFFFFFFFF


def _first_caps(n_nodes, n_tris, max_depth):
    """(cap_nodes, cap_refs) of an accel's FIRST update, from the tree it holds then: csrc/update_plan.hpp, BuildCaps, the first
    request() of one made without kept capacities (tests/cpp/update_plan_check.cpp pins the same numbers on the host).  Later
    updates keep what the last one ended with."""
    max_nodes = (1 << (max_depth + 1)) - 1
    want_nodes = min(max(1024, 4 * n_nodes), max_nodes)
    want_refs = max(4096, 2 * n_tris * (min(max_depth, 12) + 2), n_tris)
    return want_nodes, want_refs


# ---------------------------------------------------------------- scenes

def _flat(ora, meshes, cam_pos=(0.0, 3.0, 9.0), tilt=0.35, smooth=1, light=(2, 6, 3)):
    """meshes: [(vertices [n, 3], triangles [m, 3] mesh-local)], all of one diffuse material."""
    c, s_ = np.cos(tilt), np.sin(tilt)
    return ora.FlatScene(
        mesh_material=np.zeros(len(meshes), np.int32), mesh_nverts=np.array([len(v) for v, _ in meshes], np.int32),
        mesh_ntris=np.array([len(t) for _, t in meshes], np.int32),
        vertices=np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes]),
        indices=np.concatenate([np.asarray(t, np.uint32).reshape(-1, 3) for _, t in meshes]),
        mat_kind=np.array([ora.MAT_DIFFUSE], np.int32), mat_albedo=np.array([[0.8, 0.7, 0.5]], np.float32),
        mat_ior=np.array([1.0], np.float32), mat_smooth=np.array([smooth], np.int32),
        light_pos=np.array([light], np.float32), light_intensity=np.array([900], np.float32),
        cam_pos=np.array(cam_pos, np.float32), cam_mat=np.array([1, 0, 0, 0, c, -s_, 0, s_, c], np.float32),
        background=np.array([0.1, 0.3, 0.2], np.float32), width=96, height=64, bucket_size=64)


def _field(ora, g, amp, n_tris=None):
    """The height field of test_levels_longer_than_one_trip_of_the_build: g x g vertices on [-5, 5]^2, two triangles per cell;
    n_tris cuts the triangle list and keeps every vertex."""
    rng = np.random.default_rng(8)
    xs, zs = np.meshgrid(np.linspace(-5, 5, g), np.linspace(-5, 5, g), indexing="ij")
    v = np.stack([xs, amp * rng.normal(size=xs.shape) - 1.0, zs], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(g - 1), np.arange(g - 1), indexing="ij")
    a = (i * g + j).reshape(-1)
    t = np.stack([np.stack([a, a + 1, a + g], axis=1), np.stack([a + 1, a + g + 1, a + g], axis=1)], axis=1).reshape(-1, 3)
    return _flat(ora, [(v, t if n_tris is None else t[:n_tris])])


def _soup(ora, k):
    v = np.random.default_rng(3).uniform(-3, 3, size=(3 * k, 3)).astype(np.float32)
    return _flat(ora, [(v, np.arange(3 * k).reshape(k, 3))], cam_pos=(0.0, 3.0, 11.0))


def _bent(v):
    return (v * np.float32([1.0, 1.7, 0.8]) + np.float32([0.3, 0.0, 0.0])).astype(np.float32)


def _clustered(v, s, centre=None):
    """`v` shrunk by `s` about `centre` (default: the middle of its bounding box), except its first and last vertex: they stay
    where they are and with them, all but exactly, the root box."""
    w = v.astype(np.float64)
    c = (w.min(axis=0) + w.max(axis=0)) / 2 if centre is None else np.asarray(centre, np.float64)
    out = (c + (w - c) * s).astype(np.float32)
    out[0], out[-1] = v[0], v[-1]
    return out


def _node_depths(link):
    """Depth of every node of a dump, from its child links."""
    depth = np.full(link.shape[0], -1, np.int64)
    depth[0] = 0
    stack = [0]
    while stack:
        n = stack.pop()
        for c in link[n, :2]:
            if c >= 0:
                depth[c] = depth[n] + 1
                stack.append(int(c))
    assert (depth >= 0).all()
    return depth


def _widest_splitting_level(oacc):
    """Nodes in the widest level of the oracle's tree that has a node with children: k_build_tree walks such a level in trips
    of K_TREE_THREADS nodes and creates children in each."""
    _, link, _ = oacc.dump()
    depth = _node_depths(link)
    inner = link[:, 2] < 0
    return max(int((depth == d).sum()) for d in np.unique(depth[inner]))


def _check_state(rtk, ora, acc, flat, v, seed, what, max_depth=8, max_leaf=64, min_hits=500):
    """tree, hit records (the reduced ray set, both culls, three engines) and frames of `acc` against the oracle of `v`."""
    oacc, moved = _oracle(ora, flat, v, max_depth=max_depth, max_leaf=max_leaf)
    dump = _check_tree(acc, oacc, what)
    _check_hits(rtk, acc, oacc, moved, seed, what, n_rays=N_RAYS, min_hits=min_hits, **RAYS)
    _check_frames(rtk, acc, oacc, what)
    return dump, oacc


def _same_dump(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. levels wider than one workgroup

WIDE = [(64, 12, 4, 1), (40, 13, 1, 2)]      # g, max_depth, max_leaf, whole trips the widest splitting level exceeds


def _assert_wide(oacc, trips):
    """The widest level has more than 2,048 nodes, the widest level that still splits more than `trips` trips of 1,024.
    (On the 64 x 64 field at 12 / 4 the oracle gives 2,670 and 1,439: the widest level is the last one, which cannot split,
    so the child loop creates children in a second trip there, and in a third only in the other set: 4,854 and 2,601.)"""
    _, link, _ = oacc.dump()
    depth = _node_depths(link)
    assert max(int((depth == d).sum()) for d in np.unique(depth)) > 2 * K_TREE_THREADS
    assert _widest_splitting_level(oacc) > trips * K_TREE_THREADS


@pytest.mark.parametrize("g,max_depth,max_leaf,trips", WIDE)
def test_levels_wider_than_one_trip_of_the_child_loop(rtk, ora, g, max_depth, max_leaf, trips):
    """k_build_tree creates a level's children in trips of 1,024 nodes and carries next_id, next_ref and the overflow flag
    from trip to trip."""
    flat = _field(ora, g, 0.3)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=max_depth, max_leaf_size=max_leaf)
    built = acc.tree_dump()
    for i, (name, v) in enumerate((("same", flat.vertices), ("bent", _bent(flat.vertices)))):
        _assert_wide(_oracle(ora, flat, v, max_depth=max_depth, max_leaf=max_leaf)[0], trips)
        acc.update_vertices(v)
        dump, _ = _check_state(rtk, ora, acc, flat, v, 31 + i, (g, name), max_depth, max_leaf)
        if i == 0:
            assert _same_dump(built, dump)                                      # the device build of the unmoved scene is the host build


def test_wide_levels_under_fast_traversal(rtk, ora):
    """The eight front-to-back leaf orders of RTK_TRAVERSAL_FAST on a tree of several thousand nodes built on the device: the
    tree is the oracle's, occluded / intersect are those of a fresh FAST accel of the moved scene (FAST is not the parity mode)."""
    g, max_depth, max_leaf, trips = WIDE[0]
    flat = _field(ora, g, 0.3)
    v = _bent(flat.vertices)
    oacc, moved = _oracle(ora, flat, v, max_depth=max_depth, max_leaf=max_leaf)
    _assert_wide(oacc, trips)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=max_depth, max_leaf_size=max_leaf, traversal=rtk.TRAVERSAL_FAST)
    acc.update_vertices(v)
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, moved), max_depth=max_depth, max_leaf_size=max_leaf, traversal=rtk.TRAVERSAL_FAST)
    _check_tree(acc, oacc, "fast")
    rays = _rays(oacc, moved, 9, **RAYS)
    max_t = np.random.default_rng(2).uniform(0.5, 40.0, size=rays.shape[0]).astype(np.float32)
    assert (oacc.intersect(rays, True)["tri"] != MISS).sum() > 500
    for mode in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_AUTO):
        assert acc.occluded(rays, max_t, trace_mode=mode).tobytes() == fresh.occluded(rays, max_t, trace_mode=mode).tobytes(), mode
        for cull in (False, True):
            assert np.array_equal(_bits(acc.intersect(rays, cull, mode)["t"]), _bits(fresh.intersect(rays, cull, mode)["t"])), (mode, cull)


# ---------------------------------------------------------------- 2. the node table is outgrown

def test_node_table_retry_and_growth_after_it(rtk, ora):
    """An accel of a tight cluster holds a tree of a few nodes, so its first update starts with the smallest node table; the
    spread field needs several times that (kBuildNodeOverflow, need_nodes, a new up_table / up_table_host).  That first update
    comes through update_vertices_device on a caller's stream, so the retry loop runs there.  Then back to the cluster (the
    fresh build's dump, byte for byte) and out again with every buffer already grown."""
    import torch

    max_depth, max_leaf = 12, 4
    spread = _field(ora, 64, 0.3)
    cluster = _clustered(spread.vertices, 1e-4, centre=(1.3, -1.0, 2.1))
    flat = dataclasses.replace(spread, vertices=cluster)
    o_cluster, _ = _oracle(ora, flat, cluster, max_depth=max_depth, max_leaf=max_leaf)
    o_spread, _ = _oracle(ora, flat, spread.vertices, max_depth=max_depth, max_leaf=max_leaf)
    cap_nodes, _ = _first_caps(o_cluster.num_nodes, o_cluster.num_triangles, max_depth)
    assert 4 * o_cluster.num_nodes < 1024 and cap_nodes == 1024
    assert o_spread.num_nodes > cap_nodes                                       # the first update cannot fit: it must retry

    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=max_depth, max_leaf_size=max_leaf)
    built = acc.tree_dump()
    d_v = torch.from_numpy(spread.vertices).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    acc.update_vertices_device(d_v.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    out, _ = _check_state(rtk, ora, acc, flat, spread.vertices, 41, "spread", max_depth, max_leaf)
    acc.update_vertices(cluster)
    # (the cluster's triangles are 1e-5 across, under what eps = 1e-6 lets a ray hit: what is hit are the slivers to the two
    # vertices that stayed, by a few dozen rays)
    back, _ = _check_state(rtk, ora, acc, flat, cluster, 42, "cluster", max_depth, max_leaf, min_hits=20)
    assert _same_dump(built, back)
    acc.update_vertices(spread.vertices)
    again, _ = _check_state(rtk, ora, acc, flat, spread.vertices, 43, "spread again", max_depth, max_leaf)
    assert _same_dump(out, again)


# ---------------------------------------------------------------- 3. the reference lists are outgrown

@pytest.mark.parametrize("k,max_depth,max_leaf,nodes_too", [(300, 8, 64, False), (150, 10, 16, True)])
def test_reference_list_retry(rtk, ora, k, max_depth, max_leaf, nodes_too):
    """A soup of long triangles puts every triangle into many leaves: the lists of the target tree are several times the first
    capacity (kBuildRefOverflow, need_refs, new up_ref_id / up_ref_node), in the second set together with the node table.  The
    accel starts from the soup shrunk to 1 % about its centre, whose tree fits both first capacities: it is the update that
    overflows.  The way back gives the fresh build's dump byte for byte."""
    full = _soup(ora, k)
    start = _clustered(full.vertices, 0.01)
    flat = dataclasses.replace(full, vertices=start)
    o_start, _ = _oracle(ora, flat, start, max_depth=max_depth, max_leaf=max_leaf)
    o_full, _ = _oracle(ora, flat, full.vertices, max_depth=max_depth, max_leaf=max_leaf)
    cap_nodes, cap_refs = _first_caps(o_start.num_nodes, k, max_depth)
    assert o_full.num_leaf_refs > cap_refs                                      # every leaf's list lies in the table: it cannot fit
    assert o_start.num_leaf_refs <= cap_refs and o_start.num_nodes <= cap_nodes
    assert (o_full.num_nodes > cap_nodes) == nodes_too

    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=max_depth, max_leaf_size=max_leaf)
    built = acc.tree_dump()
    acc.update_vertices(full.vertices)
    _check_state(rtk, ora, acc, flat, full.vertices, 51, "full", max_depth, max_leaf)
    acc.update_vertices(start)
    back, _ = _check_state(rtk, ora, acc, flat, start, 52, "start", max_depth, max_leaf, min_hits=100)
    assert _same_dump(built, back)


# ---------------------------------------------------------------- 4. lists that end on a chunk

@pytest.mark.parametrize("n_tris", [K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK])
def test_chunk_exact_lists(rtk, ora, n_tris):
    """sweep_level walks a level's references in chunks of 8,192 and carries the open node's counts over a chunk's end.  With
    exactly 8,192 (16,384) triangles the root's last reference is also its chunk's last: the node's counts are closed and the
    carry is written by the same reference, and no chunk follows.  All 10,000 vertices stay, so thousands are in no triangle."""
    max_depth, max_leaf = 9, 48
    flat = _field(ora, 100, 0.3, n_tris=n_tris)
    assert flat.indices.shape[0] == n_tris and (n_tris % K_CHUNK == 0) == (n_tris in (K_CHUNK, 2 * K_CHUNK))
    assert np.unique(flat.indices).size < flat.vertices.shape[0] - 1000
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=max_depth, max_leaf_size=max_leaf)
    for i, (name, v) in enumerate((("same", flat.vertices), ("bent", _bent(flat.vertices)))):
        acc.update_vertices(v)
        _, oacc = _check_state(rtk, ora, acc, flat, v, 61 + i, (n_tris, name), max_depth, max_leaf)
        assert oacc.num_triangles == n_tris and oacc.num_nodes > 1


# ---------------------------------------------------------------- 5. coords_small follows the vertices

def _scaled_vertices(flat, s):
    return (flat.vertices.astype(np.float64) * s).astype(np.float32)


def _check_scaled_state(rtk, ora, acc, flat, unit, s, what):
    """`acc` holds the scene `flat` (its camera and lights, which an update does not move) with unit's vertices times s: the
    oracle of that scene, rays as test_gpu_tree_params.py scales them."""
    oacc, moved = _oracle(ora, flat, _scaled_vertices(unit, s))
    _check_tree(acc, oacc, what)
    _check_hit_records(rtk, acc, oacc, _scaled_rays(unit, s, 47), what, min_hits=5000)
    _check_frames(rtk, acc, oacc, what)


def test_an_update_across_the_bundle_limit_switches_bundle_culling(rtk, ora):
    """coords_small (api_update.hip) is recomputed by every update from kBuildCoordsBig: above kBundleLimit the interval arithmetic of
    bundle culling may overflow and must be off, below it is on again.  Up across the limit, down to just under it, down to
    the scene as loaded; and an accel BUILT above the limit comes down.  (What this pins are the results on both sides of the
    limit.  The flag alone is not observable here: a library with coords_small forced on passed this test)"""
    unit = ora.load_crtscene(SCENE5)
    big, close = dataclasses.replace(unit, vertices=_scaled_vertices(unit, 6e7)), dataclasses.replace(unit, vertices=_scaled_vertices(unit, 3e7))
    assert _leaf_coord_max(big) > K_BUNDLE_LIMIT
    assert 0.8 * K_BUNDLE_LIMIT < _leaf_coord_max(close) < K_BUNDLE_LIMIT
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, unit))
    for s in (6e7, 3e7, 1.0):
        acc.update_vertices(_scaled_vertices(unit, s))
        _check_scaled_state(rtk, ora, acc, unit, unit, s, ("from 1", s))
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, big))
    acc.update_vertices(unit.vertices)
    _check_scaled_state(rtk, ora, acc, big, unit, 1.0, ("from 6e7", 1.0))


# ---------------------------------------------------------------- 6. signed zeros among the extremes

def _zero_scene(ora):
    """Two meshes in x >= 0, y <= 0, z >= 0.  The least x, the greatest y and the least z of the scene are 0 and are attained
    twice within one triangle, in a later triangle of the same mesh, and in the second mesh.  -> (flat, holders): holders[axis]
    = the (vertex, axis) slots that hold such a zero, in the order the reference's boxes meet them."""
    rng = np.random.default_rng(6)
    a = np.array([[0, -1, 1], [0, -2, 2], [1, -1, 3],   [1, 0, 1], [2, 0, 2], [1, -1, 2],   [1, -1, 0], [2, -2, 0], [1, -2, 1],
                  [0, -3, 1], [2, -3, 2], [2, -2, 1],   [3, 0, 1], [3, -1, 2], [4, -1, 1],  [3, -1, 0], [4, -1, 1], [3, -2, 1]], np.float32)
    k = 200
    fill = rng.uniform([1.0, -4.5, 1.0], [5.5, -1.0, 4.5], size=(k, 1, 3)) + rng.uniform(-0.8, 0.8, size=(k, 3, 3))
    b = np.concatenate([np.array([[0, -4, 3], [1, -4, 4], [1, -5, 3],   [5, 0, 3], [5, -1, 4], [6, -1, 3],   [5, -3, 0], [6, -3, 1], [5, -4, 1]]),
                        fill.reshape(-1, 3)]).astype(np.float32)
    flat = _flat(ora, [(a, np.arange(len(a)).reshape(-1, 3)), (b, np.arange(len(b)).reshape(-1, 3))], cam_pos=(3.0, -1.0, 11.0),
                 tilt=0.1, smooth=0, light=(3, 4, 7))
    v = flat.vertices
    assert v[:, 0].min() == 0 and v[:, 1].max() == 0 and v[:, 2].min() == 0
    holders = [[(int(i), ax) for i in np.flatnonzero(v[:, ax] == 0)] for ax in range(3)]
    assert [len(h) for h in holders] == [4, 4, 4]
    return flat, holders


def _with_signs(v, holders, negative):
    """negative(rank): whether the rank-th holder of an axis carries -0 (the others +0)."""
    out = v.copy()
    for slots in holders:
        for rank, (i, ax) in enumerate(slots):
            out[i, ax] = np.float32(-0.0) if negative(rank) else np.float32(0.0)
    return out


def test_signed_zeros_keep_the_first_of_equals(rtk, ora):
    """box_grow keeps the first of equal extremes and -0 == +0, so which zero's bits the root box carries depends on the
    order of the triangles; the device reduces (value, triangle) keys in any order and must end with the same bits."""
    flat, holders = _zero_scene(ora)
    orderings = [("-0 first", lambda r: r == 0), ("+0 first", lambda r: r != 0),
                 ("-0 second in its triangle", lambda r: r == 1), ("-0 in the second mesh only", lambda r: r == 3)]
    roots = {}
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    for i, (name, negative) in enumerate(orderings):
        v = _with_signs(flat.vertices, holders, negative)
        assert np.array_equal(v, flat.vertices) and np.signbit(v).sum() > np.signbit(flat.vertices).sum()
        acc.update_vertices(v)
        (box, _, _), oacc = _check_state(rtk, ora, acc, flat, v, 71 + i, name, min_hits=300)
        roots[name] = _bits(oacc.dump()[0][0]).copy()
        assert np.array_equal(_bits(box[0]), roots[name]), name
    differ = roots["-0 first"] ^ roots["+0 first"]
    assert (differ[[0, 4, 2]] == 0x80000000).all() and (differ[[1, 3, 5]] == 0).all()     # min.x, max.y, min.z: the sign alone
    assert np.array_equal(roots["+0 first"], roots["-0 second in its triangle"])
    assert np.array_equal(roots["+0 first"], roots["-0 in the second mesh only"])


# ---------------------------------------------------------------- 7. unused vertices, one vertex with 2,000 triangles

def test_unused_vertices_and_a_fan(rtk, ora):
    """A fan of 2,000 smooth-shaded triangles around one apex: the apex normal is a serial sum of 2,000 face normals in
    triangle order (k_build_normals), compared by bits through the hits' interpolated normals.  Three vertices belong to no
    triangle, one of them far outside: they must stay out of the root box (and their NaN normals out of every result)."""
    n = 2000
    rng = np.random.default_rng(7)
    ang = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    rim = np.stack([3 * np.cos(ang), -1.0 + 0.2 * rng.normal(size=n), 3 * np.sin(ang)], axis=1)
    v = np.concatenate([[[0.0, 0.5, 0.0]], rim, [[0.5, 0.2, 0.5], [-4.0, 2.0, 1.0], [100.0, 100.0, 100.0]]]).astype(np.float32)
    t = np.stack([np.zeros(n, np.int64), 1 + (np.arange(n) + 1) % n, 1 + np.arange(n)], axis=1)         # (faces up)
    flat = _flat(ora, [(v, t)], smooth=1)
    assert np.unique(t).size == len(v) - 3 and (t == 0).sum() == n
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    for i, scale in enumerate((0.0, 0.05)):
        w = (v + rng.normal(scale=scale, size=v.shape)).astype(np.float32) if scale else v
        acc.update_vertices(w)
        (box, _, _), oacc = _check_state(rtk, ora, acc, flat, w, 81 + i, scale)
        obox = oacc.dump()[0][0]
        assert (w[-1] > obox[3:]).all() and not (w[-2] <= obox[3:]).all()       # neither outside vertex is in the oracle's root
        # rays at the triangles close to the apex, where all 2,000 meet
        k = 256
        tri = rng.integers(0, n, size=k)
        bary = rng.dirichlet([1, 1, 1], size=k) * 0.04
        target = w[0].astype(np.float64) + bary[:, 1:2] * (w[t[tri, 1]] - w[0]) + bary[:, 2:3] * (w[t[tri, 2]] - w[0])
        origin = target + np.array([0.0, 6.0, 0.0]) + rng.normal(scale=1.5, size=(k, 3))
        rays = np.concatenate([origin, target - origin], axis=1).astype(np.float32)
        ref = oacc.intersect(rays, True)
        at = rays[:, :3] + ref["t"][:, None] * rays[:, 3:]
        assert ((ref["tri"] != MISS) & (np.linalg.norm(at - w[0], axis=1) < 0.25)).sum() >= 200      # (a rim point is 3.4 away)
        _check_hit_records(rtk, acc, oacc, rays, ("apex", scale), min_hits=200)


# ---------------------------------------------------------------- 8. roots without extent

def test_root_with_extent_in_one_axis(rtk, ora):
    """Every vertex on the line y = z = 0: the split's axis hand-over (aabb3.hpp:43-60) runs twice at every level.  Nothing
    can be hit (every triangle has no area), so the hit records are compared with a floor of no hits."""
    flat = _soup(ora, 100)
    x = np.random.default_rng(9).permutation(300).astype(np.float32) * np.float32(0.02) - np.float32(3.0)
    line = np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)
    oacc, moved = _oracle(ora, flat, line, max_leaf=16)
    obox = oacc.dump()[0][0]
    assert ((obox[3:] - obox[:3]) == 0).tolist() == [False, True, True] and oacc.num_nodes > 1
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_leaf_size=16)
    acc.update_vertices(line)
    _check_tree(acc, oacc, "line")
    rays = _rays(oacc, moved, 91, **RAYS)
    assert (oacc.intersect(rays, False)["tri"] == MISS).all()
    _check_hit_records(rtk, acc, oacc, rays, "line", min_hits=0)


def test_point_root_is_a_leaf(rtk, ora):
    """Every vertex at one point.  The CPU oracle is NOT the yardstick here: the reference's aabb3::split gives up its axis
    hand-over after three steps and goes on splitting a point box down to max_depth (8,191 nodes at depth 12), where the
    product makes the root a leaf on purpose (kdtree.cpp split_box, build.hip k_build_tree).  So the updated accel is
    compared with a fresh product accel of the moved arrays: the same dump, one leaf of all triangles, and no ray hits."""
    flat = _soup(ora, 100)
    point = np.tile(np.float32([0.5, -0.25, 1.0]), (300, 1))
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=12, max_leaf_size=16)
    assert acc.tree_info().n_nodes > 1
    acc.update_vertices(point)
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, dataclasses.replace(flat, vertices=point)), max_depth=12, max_leaf_size=16)
    assert _same_dump(acc.tree_dump(), fresh.tree_dump())
    for a in (acc, fresh):
        ti = a.tree_info()
        assert (ti.n_nodes, ti.n_leaves, ti.n_leaf_refs) == (1, 1, 100)
    rng = np.random.default_rng(10)
    origin = point[0] + rng.normal(size=(2000, 3)) * rng.uniform(0.5, 10.0, size=(2000, 1))
    rays = np.concatenate([origin, point[0] - origin], axis=1).astype(np.float32)          # straight at the point
    for cull in (False, True):
        for mode in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_AUTO):
            for a in (acc, fresh):
                assert (a.intersect(rays, cull, mode)["tri"] == MISS).all(), (cull, mode)


# ---------------------------------------------------------------- 9. no triangles

def test_empty_accel_can_be_updated(rtk):
    """The zero-triangle scene of test_empty_and_tiny_scenes_build: an update with no vertices succeeds and changes nothing."""
    common = dict(mat_kind=np.array([0], np.int32), mat_albedo=np.ones((1, 3), np.float32), mat_ior=np.ones(1, np.float32),
                  mat_smooth=np.zeros(1, np.int32), light_pos=np.zeros((1, 3), np.float32),
                  light_intensity=np.ones(1, np.float32), cam_pos=np.zeros(3, np.float32),
                  cam_mat=np.eye(3, dtype=np.float32).ravel(), background=np.array([0.25, 0.5, 0.75], np.float32), width=8, height=8)
    empty = rtk.Scene.from_arrays(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3), np.float32),
                                  np.zeros((0, 3), np.uint32), **common)
    acc = rtk.KdTreeSimdAccel(empty)
    cfg = rtk.RenderConfig(width=8, height=8, max_ray_depth=3)
    before, cn = acc.render_frame(cfg)
    assert (before == np.float32([0.25, 0.5, 0.75])).all()
    for rep in range(2):
        acc.update_vertices(np.zeros((0, 3), np.float32))
        ti = acc.tree_info()
        assert (ti.n_nodes, ti.n_leaves, ti.n_leaf_refs) == (1, 1, 0)
        after, cn2 = acc.render_frame(cfg)
        assert after.tobytes() == before.tobytes() and cn2["rays"] == cn["rays"]
