"""What the tests of rtk_accel_update_vertices share (test_gpu_update.py, test_gpu_update_regimes.py): an updated accel against
the CPU oracle built from the moved vertices.  "Equal" is bit-equal throughout: the tree dump, every field of every hit record,
every frame and its ray count."""
import dataclasses

import numpy as np

W, H, DEPTH = 96, 64, 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_frame(a, b):
    """Bit-identical, except that a NaN pixel only has to be a NaN on both sides (test_random_scenes.py: which payload a NaN
    carries through an addition is a property of the hardware, not of the algorithm)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(_bits(np.where(na, 0.0, a).astype(np.float32)), _bits(np.where(nb, 0.0, b).astype(np.float32)))


def _same_floats(a, b):
    """Bit-identical; NaN must meet NaN."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(np.nan_to_num(a)), _bits(np.nan_to_num(b)))


def _rtk_scene(rtk, f):
    return rtk.Scene.from_arrays(f.mesh_material, f.mesh_nverts, f.mesh_ntris, f.vertices, f.indices, f.mat_kind, f.mat_albedo,
                                 f.mat_ior, f.mat_smooth, f.light_pos, f.light_intensity, f.cam_pos, f.cam_mat, f.background,
                                 f.width, f.height, f.bucket_size, mat_texture=f.mat_texture, uvs=f.uvs, mesh_has_uvs=f.mesh_has_uvs,
                                 tex_kind=f.tex_kind, tex_color_a=f.tex_color_a, tex_color_b=f.tex_color_b, tex_param=f.tex_param,
                                 tex_pixels=f.tex_pixels, tex_bitmap=f.tex_bitmap)


# ---------------------------------------------------------------- rays

def _global_indices(flat):
    starts = np.concatenate([[0], np.cumsum(flat.mesh_nverts)[:-1]])
    tri_mesh = np.repeat(np.arange(len(flat.mesh_ntris)), flat.mesh_ntris)
    return flat.indices.astype(np.int64) + starts[tri_mesh][:, None]


def _rays(oacc, flat, seed, n_aimed=800, n_cam=(160, 120)):
    """Camera rays (n_cam: 160x120 = 19,200) plus rays aimed at vertices and edge midpoints of the moved triangles: 20,000."""
    cam = oacc.camera_rays(*n_cam).reshape(-1, 6)
    rng = np.random.default_rng(seed)
    g = _global_indices(flat)
    t = rng.integers(0, g.shape[0], size=n_aimed)
    v0, v1, v2 = (flat.vertices[g[t, k]].astype(np.float64) for k in range(3))
    kind = rng.integers(0, 4, size=n_aimed)
    target = np.select([(kind == 0)[:, None], (kind == 1)[:, None], (kind == 2)[:, None], (kind == 3)[:, None]],
                       [v0, (v0 + v1) / 2, (v0 + v2) / 2, (v1 + v2) / 2])
    origin = target + rng.normal(size=(n_aimed, 3)) * rng.uniform(0.5, 30.0, size=(n_aimed, 1))
    d = target - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 0.37, 4.0], size=(n_aimed, 1))
    aimed = np.concatenate([origin, d], axis=1)
    return np.ascontiguousarray(np.concatenate([cam, aimed]).astype(np.float32))


# ---------------------------------------------------------------- checks

def _oracle(ora, flat, v, max_depth=8, max_leaf=64):
    moved = dataclasses.replace(flat, vertices=np.ascontiguousarray(v, np.float32))
    return ora.Accel(ora.Scene(moved), ora.ACCEL_KD_SIMD, max_depth=max_depth, max_leaf=max_leaf), moved


def _check_tree(acc, oacc, what):
    box, link, refs = acc.tree_dump()
    obox, olink, orefs = oacc.dump()
    assert box.shape == obox.shape and np.array_equal(_bits(box), _bits(obox)), what
    assert np.array_equal(link, olink), what
    assert np.array_equal(refs, orefs), what
    ti = acc.tree_info()
    leaf = olink[:, 2] >= 0
    assert (ti.n_nodes, ti.n_leaf_refs, ti.n_triangles) == (oacc.num_nodes, oacc.num_leaf_refs, oacc.num_triangles), what
    assert (ti.n_leaves, ti.n_inner) == (int(leaf.sum()), int((~leaf).sum())), what
    assert ti.max_leaf_refs == int(olink[leaf, 3].max()), what
    return box, link, refs


def _check_hit_records(rtk, acc, oacc, rays, what, min_hits=500):
    """The closest hits of `rays` with and without culling, in the three batch engines, against the oracle's.  More than
    `min_hits` of the rays must hit; 0 asks for none (a scene nothing can hit)."""
    for cull in (False, True):
        ref = oacc.intersect(rays, cull)
        hit = ref["tri"] != 0xFFFFFFFF
        assert min_hits == 0 or hit.sum() > min_hits, what
        for mode in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_AUTO):
            got = acc.intersect(rays, cull, mode)
            w = (what, cull, mode)
            assert np.array_equal(got["tri"], ref["tri"]), w
            assert np.array_equal(got["mesh"], ref["mesh"]), w
            for f in ("t", "u", "v"):
                assert np.array_equal(_bits(got[f]), _bits(ref[f])), (w, f)
            assert _same_floats(got["normal"][hit], ref["normal"][hit]), w      # smooth-shaded normals: the device's vertex normals


def _check_hits(rtk, acc, oacc, moved, seed, what, n_rays=20_000, min_hits=500, **rays_kw):
    rays = _rays(oacc, moved, seed, **rays_kw)
    assert rays.shape[0] == n_rays
    _check_hit_records(rtk, acc, oacc, rays, what, min_hits)


def _check_frames(rtk, acc, oacc, what, modes=None, gi=0, spp=1):
    ref, ocn = oacc.render(W, H, spp, DEPTH, gi)
    assert np.isfinite(ref).any()
    for mode in modes or (rtk.TRACE_AUTO, rtk.TRACE_GROUP4, rtk.TRACE_STREAM):
        for rep in range(2):                                                    # the second frame runs in cost-feedback order
            rgb, cn = acc.render_frame(rtk.RenderConfig(width=W, height=H, spp=spp, max_ray_depth=DEPTH, diffuse_rays=gi, trace_mode=mode))
            assert cn["rays"] == ocn["rays"], (what, mode, rep)
            assert _same_frame(rgb, ref), (what, mode, rep)
    return ref


def _check_all(rtk, ora, acc, flat, v, seed, what, **tree):
    oacc, moved = _oracle(ora, flat, v, **tree)
    dump = _check_tree(acc, oacc, what)
    _check_hits(rtk, acc, oacc, moved, seed, what)
    _check_frames(rtk, acc, oacc, what)
    return dump
