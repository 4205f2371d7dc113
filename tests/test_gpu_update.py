"""rtk_accel_update_vertices: the accel after the scene's vertices moved, rebuilt on the device (csrc/build.hip), against the CPU
oracle built from the moved vertices.  "Equal" is bit-equal throughout: the tree dump, every field of every hit record, every
frame and its ray count.  The deformations make the tree grow and shrink (scene5: 188 nodes as loaded, fewer when twisted, 35
when the dragon is shrunk), so buffers of the accel are outgrown and under-filled within one test."""
import numpy as np
import pytest

from conftest import SCENE2, SCENE5, SCENE8
from update_checks import (DEPTH, H, W, _bits, _check_all, _check_frames, _check_hits, _check_tree, _oracle, _rays, _rtk_scene,
                           _same_frame)

pytestmark = pytest.mark.gpu

FIXTURES = {"scene5": SCENE5, "scene8": SCENE8, "hw15_scene2": SCENE2}


# ---------------------------------------------------------------- deformations

def _big_mesh(flat):
    """Vertex range of the mesh with the most triangles (the dragon of the fixture scenes)."""
    m = int(np.argmax(flat.mesh_ntris))
    start = int(np.sum(flat.mesh_nverts[:m]))
    return start, start + int(flat.mesh_nverts[m])


def _twist(flat, angle):
    """The big mesh twisted about the vertical axis through its centre (by `angle` radians from bottom to top) and stretched
    upwards by 1 + 0.4 * angle."""
    a, b = _big_mesh(flat)
    v = flat.vertices.astype(np.float64).copy()
    p = v[a:b]
    c = (p.min(axis=0) + p.max(axis=0)) / 2
    hgt = max(p[:, 1].max() - p[:, 1].min(), 1e-9)
    th = angle * (p[:, 1] - p[:, 1].min()) / hgt
    x, z = p[:, 0] - c[0], p[:, 2] - c[2]
    q = p.copy()
    q[:, 0] = c[0] + np.cos(th) * x - np.sin(th) * z
    q[:, 2] = c[2] + np.sin(th) * x + np.cos(th) * z
    q[:, 1] = p[:, 1].min() + (p[:, 1] - p[:, 1].min()) * (1.0 + 0.4 * angle)
    v[a:b] = q
    return v.astype(np.float32)


def _shrink(flat, s=0.05):
    a, b = _big_mesh(flat)
    v = flat.vertices.astype(np.float64).copy()
    c = (v[a:b].min(axis=0) + v[a:b].max(axis=0)) / 2
    v[a:b] = c + (v[a:b] - c) * s
    return v.astype(np.float32)


# ---------------------------------------------------------------- 1. fixture scenes

@pytest.mark.parametrize("scene", list(FIXTURES))
def test_fixture_scene_follows_its_vertices(rtk, ora, scene):
    path = FIXTURES[scene]
    flat = ora.load_crtscene(path)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    built = acc.tree_dump()
    steps = [("v0", flat.vertices), ("twist0.5", _twist(flat, 0.5)), ("twist1.0", _twist(flat, 1.0)), ("shrink", _shrink(flat)),
             ("back", flat.vertices)]
    sizes, first = [], None
    for i, (name, v) in enumerate(steps):
        acc.update_vertices(v)
        dump = _check_all(rtk, ora, acc, flat, v, seed=11 + i, what=(scene, name))
        sizes.append((dump[0].shape[0], dump[2].shape[0]))
        if first is None:
            first = dump
    # the device build of the unmoved scene is the host build, and the way back ends where it began
    for a, b, c in zip(built, first, dump):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert len(set(sizes)) >= 3, sizes                                          # the tree did change size, both ways
    assert min(s[0] for s in sizes) < sizes[0][0]


@pytest.mark.parametrize("max_depth,max_leaf", [(10, 16), (0, 64)])
def test_other_tree_parameters(rtk, ora, max_depth, max_leaf):
    flat = ora.load_crtscene(SCENE5)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5), max_depth=max_depth, max_leaf_size=max_leaf)
    v = _twist(flat, 1.0)
    acc.update_vertices(v)
    box, _, _ = _check_all(rtk, ora, acc, flat, v, seed=5, what=(max_depth, max_leaf), max_depth=max_depth, max_leaf=max_leaf)
    assert (box.shape[0] == 1) == (max_depth == 0)


# ---------------------------------------------------------------- 2. generated scenes

def _make_scene(ora, seed):
    """The soup of test_random_scenes.py: a bumpy height field, a triangle soup with zero-area, point and duplicated triangles and
    a repeated vertex index, axis-aligned quads whose planes are box planes."""
    rng = np.random.default_rng(seed)
    verts, idx, nverts, ntris, mesh_mat = [], [], [], [], []

    def add_mesh(v, t, m):
        verts.append(np.asarray(v, np.float32).reshape(-1, 3)); idx.append(np.asarray(t, np.uint32).reshape(-1, 3))
        nverts.append(len(verts[-1])); ntris.append(len(idx[-1])); mesh_mat.append(m)

    n_mat = 5
    g = int(rng.integers(6, 24))
    xs, zs = np.meshgrid(np.linspace(-4, 4, g), np.linspace(-4, 4, g), indexing="ij")
    ys = 0.4 * rng.normal(size=xs.shape) - 1.0
    v = np.stack([xs, ys, zs], axis=-1).reshape(-1, 3)
    t = []
    for i in range(g - 1):
        for j in range(g - 1):
            a = i * g + j
            t += [[a, a + 1, a + g], [a + 1, a + g + 1, a + g]]
    add_mesh(v, t, int(rng.integers(0, n_mat)))
    k = int(rng.integers(20, 300))
    v = rng.uniform(-3, 3, size=(3 * k, 3)) * np.array([1.0, 0.6, 1.0]) + np.array([0, 1.0, 0])
    t = np.arange(3 * k).reshape(k, 3).tolist()
    t += [[0, 0, 1], [2, 2, 2], t[0]]                                       # degenerate, point, duplicate
    add_mesh(v, t, int(rng.integers(0, n_mat)))
    add_mesh([[-6, -2, -6], [6, -2, -6], [6, -2, 6], [-6, -2, 6]], [[0, 2, 1], [0, 3, 2]], int(rng.integers(0, n_mat)))
    add_mesh([[-6, -2, -6], [6, -2, -6], [6, 5, -6], [-6, 5, -6]], [[0, 1, 2], [0, 2, 3]], int(rng.integers(0, n_mat)))
    kinds = np.array([ora.MAT_DIFFUSE, ora.MAT_REFLECTIVE, ora.MAT_REFRACTIVE if seed % 2 else ora.MAT_DIFFUSE, ora.MAT_CONSTANT,
                      ora.MAT_DIFFUSE], np.int32)
    n_l = int(rng.integers(1, 6))
    lights = rng.uniform(-5, 5, size=(n_l, 3)) + np.array([0, 6, 0])
    c, s_ = np.cos(0.35), np.sin(0.35)
    return ora.FlatScene(
        mesh_material=np.asarray(mesh_mat, np.int32), mesh_nverts=np.asarray(nverts, np.int32), mesh_ntris=np.asarray(ntris, np.int32),
        vertices=np.concatenate(verts).astype(np.float32), indices=np.concatenate(idx).astype(np.uint32),
        mat_kind=kinds, mat_albedo=rng.uniform(0.1, 1.0, size=(n_mat, 3)).astype(np.float32),
        mat_ior=np.full(n_mat, 1.5, np.float32), mat_smooth=rng.integers(0, 2, size=n_mat).astype(np.int32),
        light_pos=lights.astype(np.float32), light_intensity=rng.uniform(100, 2000, size=n_l).astype(np.float32),
        cam_pos=np.array([0.0 if seed % 4 else 0.5, 3.0, 11.0], np.float32),
        cam_mat=np.array([1, 0, 0, 0, c, -s_, 0, s_, c], np.float32), background=np.array([0.1, 0.3, 0.2], np.float32),
        width=96, height=64, bucket_size=int(rng.choice([16, 24, 64])))


@pytest.mark.parametrize("seed", range(4))
def test_generated_scene_follows_its_vertices(rtk, ora, seed):
    flat = _make_scene(ora, 40 + seed)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat))
    built = acc.tree_dump()
    rng = np.random.default_rng(seed)
    jitter = (flat.vertices + rng.normal(scale=0.3, size=flat.vertices.shape)).astype(np.float32)
    level = flat.vertices.copy()
    a = int(flat.mesh_nverts[0])
    level[a:a + int(flat.mesh_nverts[1]), 1] = np.float32(0.75)                 # the soup flattened: every box of it has no extent in y
    if seed % 2:
        level[:, 1] = np.float32(-2.0)                                          # everything: the ROOT box has no extent in y
    dump = None
    for name, v in (("jitter", jitter), ("level", level), ("back", flat.vertices)):
        acc.update_vertices(v)
        oacc, moved = _oracle(ora, flat, v)
        dump = _check_tree(acc, oacc, (seed, name))
        _check_hits(rtk, acc, oacc, moved, seed, (seed, name))
        _check_frames(rtk, acc, oacc, (seed, name), gi=1 if seed == 1 else 0, spp=1 + seed % 2)
    for x, y in zip(built, dump):
        assert x.tobytes() == y.tobytes()


def test_levels_longer_than_one_trip_of_the_build(rtk, ora):
    """The device build walks a level's references in chunks of 8,192 (csrc/build.hip, kChunk) and carries a node's counts from
    chunk to chunk: 19,602 triangles put the root's list (and the next levels' lists) across three chunks, with nodes that end
    anywhere inside them."""
    g = 100
    rng = np.random.default_rng(8)
    xs, zs = np.meshgrid(np.linspace(-5, 5, g), np.linspace(-5, 5, g), indexing="ij")
    v = np.stack([xs, 0.3 * rng.normal(size=xs.shape) - 1.0, zs], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(g - 1), np.arange(g - 1), indexing="ij")
    a = (i * g + j).reshape(-1)
    t = np.stack([np.stack([a, a + 1, a + g], axis=1), np.stack([a + 1, a + g + 1, a + g], axis=1)], axis=1).reshape(-1, 3)
    c, s_ = np.cos(0.35), np.sin(0.35)
    flat = ora.FlatScene(
        mesh_material=np.array([0], np.int32), mesh_nverts=np.array([len(v)], np.int32), mesh_ntris=np.array([len(t)], np.int32),
        vertices=v, indices=t.astype(np.uint32), mat_kind=np.array([ora.MAT_DIFFUSE], np.int32),
        mat_albedo=np.array([[0.8, 0.7, 0.5]], np.float32), mat_ior=np.array([1.0], np.float32), mat_smooth=np.array([1], np.int32),
        light_pos=np.array([[2, 6, 3]], np.float32), light_intensity=np.array([900], np.float32),
        cam_pos=np.array([0.0, 3.0, 9.0], np.float32), cam_mat=np.array([1, 0, 0, 0, c, -s_, 0, s_, c], np.float32),
        background=np.array([0.1, 0.3, 0.2], np.float32), width=96, height=64, bucket_size=64)
    assert len(t) > 2 * 8192
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), max_depth=9, max_leaf_size=48)
    for name, w in (("same", flat.vertices), ("bent", (flat.vertices * np.float32([1.0, 1.7, 0.8]) + np.float32([0.3, 0.0, 0.0])).astype(np.float32))):
        acc.update_vertices(w)
        _check_all(rtk, ora, acc, flat, w, seed=21, what=name, max_depth=9, max_leaf=48)


# ---------------------------------------------------------------- 3. both entry points

def test_device_variant_on_a_stream_of_its_own(rtk, ora):
    """update_vertices_device from a torch tensor on a non-default stream gives the host variant's accel, and a radiance batch
    issued on ANOTHER stream right behind it sees the new geometry (the accel's own ordering, not the caller's)."""
    import torch

    flat = ora.load_crtscene(SCENE5)
    v = _twist(flat, 1.0)
    host = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    host.update_vertices(v)
    devv = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))                    # (never on the device before: goes there first)
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=DEPTH)
    rays = np.ascontiguousarray(host.camera_rays(cfg, 0).reshape(-1, 6))
    n = rays.shape[0]
    d_v = torch.from_numpy(v).cuda()
    d_rays = torch.from_numpy(rays).cuda()
    d_rgb = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    rcfg = rtk.RadianceConfig(max_ray_depth=DEPTH)
    for rep in range(2):                                                        # the second time with everything allocated
        devv.update_vertices_device(d_v.data_ptr(), s1.cuda_stream)
        devv.radiance_device(d_rays.data_ptr(), 0, n, d_rgb.data_ptr(), rcfg, s2.cuda_stream)
        s2.synchronize()
        for x, y in zip(host.tree_dump(), devv.tree_dump()):
            assert x.tobytes() == y.tobytes()
        want, _ = host.radiance(rays, cfg=rcfg)
        assert _same_frame(d_rgb.cpu().numpy(), want)
        oacc, _ = _oracle(ora, flat, v)
        ref, _ = oacc.render(W, H, 1, DEPTH, 0)
        assert _same_frame(d_rgb.cpu().numpy().reshape(H, W, 3) + np.float32(0.0), ref)          # (a frame adds its one sample to +0)
        d_rgb.fill_(float("nan"))
        torch.cuda.synchronize()
    _check_all(rtk, ora, devv, flat, v, seed=3, what="device variant")


# ---------------------------------------------------------------- 4. RTK_TRAVERSAL_FAST

@pytest.mark.parametrize("scene", ["scene8", "scene5"])
def test_fast_traversal_accels_follow_too(rtk, ora, scene):
    """FAST is not the parity mode, so the yardstick for its own results is a fresh FAST accel of the moved scene; on scene5,
    where nothing is transmissive, FAST frames are the oracle's as well."""
    path = FIXTURES[scene]
    flat = ora.load_crtscene(path)
    v = _twist(flat, 1.0)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path), traversal=rtk.TRAVERSAL_FAST)
    acc.render_frame(rtk.RenderConfig(width=W, height=H, max_ray_depth=DEPTH))  # the old geometry has been on the device and rendered
    acc.update_vertices(v)
    oacc, moved = _oracle(ora, flat, v)
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, moved), traversal=rtk.TRAVERSAL_FAST)
    _check_tree(acc, oacc, scene)
    depth = 10 if scene == "scene8" else DEPTH
    ref, ocn = oacc.render(W, H, 1, depth, 0)
    for mode in (rtk.TRACE_AUTO, rtk.TRACE_GROUP4, rtk.TRACE_STREAM):
        cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=depth, trace_mode=mode)
        for rep in range(2):
            got, cn = acc.render_frame(cfg)
            want, wn = fresh.render_frame(cfg)
            assert _same_frame(got, want), (mode, rep)
            # (`rays` is compared where both accels certainly ran the same engine: under FAST the opaque-only occlusion tree
            # answers in one query what the megakernel steps through, and RTK_TRACE_AUTO's trial may be one frame apart on
            # the two accels -- the fresh one allocates its queues on its first frame and times the pipeline a frame later)
            assert mode == rtk.TRACE_AUTO or cn["rays"] == wn["rays"], (mode, rep)
            if scene == "scene5":                                               # nothing transmissive: FAST frames are the oracle's, in every engine
                assert _same_frame(got, ref) and cn["rays"] == ocn["rays"], (mode, rep)
    rays = _rays(oacc, moved, 9)
    max_t = np.random.default_rng(2).uniform(0.5, 40.0, size=rays.shape[0]).astype(np.float32)
    for mode in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_AUTO):
        assert acc.occluded(rays, max_t, trace_mode=mode).tobytes() == fresh.occluded(rays, max_t, trace_mode=mode).tobytes(), mode
        for cull in (False, True):
            assert np.array_equal(_bits(acc.intersect(rays, cull, mode)["t"]), _bits(fresh.intersect(rays, cull, mode)["t"])), (mode, cull)


# ---------------------------------------------------------------- 5. errors

@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_vertices_are_refused_and_change_nothing(rtk, ora, bad):
    import torch

    flat = ora.load_crtscene(SCENE5)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    acc.update_vertices(_twist(flat, 0.5))
    cfg = rtk.RenderConfig(width=W, height=H, max_ray_depth=DEPTH)
    before, frame = acc.tree_dump(), acc.render_frame(cfg)[0]
    v = _twist(flat, 1.0)
    v[-1, 2] = bad                                                              # (the last vertex: found by the last thread)
    with pytest.raises(rtk.RtkError) as e:
        acc.update_vertices(v)
    assert e.value.code == rtk.RTK_ERR_INVALID
    d_v = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    with pytest.raises(rtk.RtkError) as e:
        acc.update_vertices_device(d_v.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert e.value.code == rtk.RTK_ERR_INVALID
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    for rep in range(2):
        assert _same_frame(acc.render_frame(cfg)[0], frame)
    oacc, _ = _oracle(ora, flat, _twist(flat, 0.5))
    assert _same_frame(frame, oacc.render(W, H, 1, DEPTH, 0)[0])
    acc.update_vertices(flat.vertices)                                          # and the accel stays usable
    _check_tree(acc, _oracle(ora, flat, flat.vertices)[0], "after the refusals")
