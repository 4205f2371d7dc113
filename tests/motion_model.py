"""The numpy float32 model of rtk_render_motion (include/rtk.h spells the arithmetic out) and the fixtures the motion tests share:
the planes of the CPU oracle's first hits on hw09/scene5, hostile variants of them, and one mesh moved under a standing camera.
Whole-array expressions, every operation in float32 in the order the contract writes it: numpy does not contract a multiply and
an add, so the bits are those of the scalar C++ of csrc/motion_math.hpp built with -ffp-contract=off, and of the kernel.  The
projection is tests/temporal_model.py's."""
import dataclasses

import numpy as np

import temporal_model as tm
from conftest import SCENE5

F = np.float32
MISS = 0xFFFFFFFF
MISS_BITS = np.uint32(0x7FC00000)
FOV = 90.0                                                    # the oracle's and RenderConfig's default
SIZES = ((1, 1), (7, 5), (64, 64), (130, 70))                 # width x height
OUTPUTS = (("prev_position",), ("motion",), ("prev_position", "motion"))

# max |P' - position| over the oracle's hits on scene5 with the scene's own vertices, the largest over SIZES, as
# tests/test_motion_model.py measures it on the CPU: 3.433e-05 (depths of 17 to 46; the g-buffer's position is o + t * d, P' the
# barycentric sum).  The GPU tests allow four times that.
RECONSTRUCTION_ERR = 3.44e-05
POSITION_TOL = 4.0 * RECONSTRUCTION_ERR
# max |motion| over the same hits with the scene's own vertices and camera, measured likewise: 5.722e-05 px
MOTION_BOUND = 5.73e-05
# The moving-mesh chain: mesh 1 of scene5 (the object above the ground plane) translated by MOVE under the standing camera.  With
# prev_position handed to temporal as position, SHARE_WITH of the mesh's hit pixels must keep their history; with position itself
# at most SHARE_WITHOUT may.  The model alone gives 0.952 and 0.054 at 130 x 70, 0.929 and 0.064 at 64 x 64 (what is
# lost with prev_position has not been taken apart; supposed: silhouette pixels, and neighbouring facets whose smooth normals
# differ by more than normal_min_dot allows at these sizes).
MOVED_MESH = 1
MOVE = np.array((0.0, 1.0, 0.0), F)
SHARE_WITH, SHARE_WITHOUT = 0.9, 0.1


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def global_indices(flat):
    """[n_triangles, 3] global vertex ids from the scene's mesh-local indices: a mesh's vertices follow those of the meshes before it"""
    starts = np.concatenate([[0], np.cumsum(flat.mesh_nverts)[:-1]]).astype(np.int64)
    tri_mesh = np.repeat(np.arange(len(flat.mesh_ntris)), flat.mesh_ntris)
    return np.asarray(flat.indices, np.int64).reshape(-1, 3) + starts[tri_mesh][:, None]


def render_motion(tri, bary, index, prev_vertices, view=None, fov_degrees=FOV):
    """Steps 1-3 of rtk.h.  tri [h, w] uint32, bary [h, w, 2]; index [n_triangles, 3] global vertex ids; prev_vertices
    [n_vertices, 3]; view = (position[3], matrix[9]) or None (no motion).  -> dict prev_position [h, w, 3], motion [h, w, 2] or
    None, hit [h, w] bool, computed [h, w] bool (the pixels whose motion is arithmetic and not the miss bits)."""
    tri = np.asarray(tri, np.uint32)
    h, w = tri.shape
    index = np.asarray(index, np.int64).reshape(-1, 3)
    verts = np.asarray(prev_vertices, F).reshape(-1, 3)
    hit = tri < np.uint32(min(index.shape[0], MISS))                      # step 1: nothing is dereferenced with another id
    safe = np.where(hit, tri, 0).astype(np.int64)
    P = np.zeros((h, w, 3), F)
    if index.shape[0]:
        ids = index[safe]
        A, B, C = verts[ids[..., 0]], verts[ids[..., 1]], verts[ids[..., 2]]
        with np.errstate(all="ignore"):
            u, v = np.asarray(bary, F)[..., 0:1], np.asarray(bary, F)[..., 1:2]
            wgt = (F(1.0) - u) - v
            Pp = ((wgt * A) + (u * B)) + (v * C)
        P = np.where(hit[..., None], Pp, F(0.0)).astype(F)
    out = dict(prev_position=np.ascontiguousarray(P, F), motion=None, hit=hit, computed=np.zeros((h, w), bool))
    if view is not None:
        C0 = np.asarray(view[0], F).reshape(3)
        M = np.asarray(view[1], F).reshape(9)
        with np.errstate(all="ignore"):
            D = [P[..., k] - C0[k] for k in range(3)]
            cz = (M[6] * D[0] + M[7] * D[1]) + M[8] * D[2]                 # (tm.project's own expression: its test is inside `ok`)
            _, fx, fy = tm.project(P, view, w, h, fov_degrees)
            ys, xs = np.mgrid[0:h, 0:w]
            mx, my = fx - xs.astype(F), fy - ys.astype(F)
        computed = hit & (cz < F(0.0))
        m = np.stack([mx, my], axis=-1).astype(F)
        out["motion"] = np.where(computed[..., None], m.view(np.uint32), MISS_BITS).view(F)
        out["computed"] = computed
    return out


def assert_same(got, want, names=("prev_position", "motion"), what=""):
    """Every bit of the planes `names`; where the model's value is a NaN that arithmetic made (a non-finite barycentric that
    propagated), a NaN must meet a NaN: which payload and sign an invalid operation leaves is the hardware's.  The miss bits of
    `motion` are written, not computed, and must be met exactly."""
    for name in names:
        g, w_ = bits(got[name]), bits(want[name])
        assert g.shape == w_.shape, (what, name, g.shape, w_.shape)
        made = np.isnan(np.asarray(want[name], F))
        if name == "motion":
            made &= want["computed"][..., None]
        else:
            made &= want["hit"][..., None]
        assert np.array_equal(np.isnan(np.asarray(got[name], F))[made], made[made]), (what, name, "NaN")
        diff = (g != w_) & ~made
        assert not diff.any(), (what, name, int(diff.sum()))


# ---- the shared fixture: the oracle's first hits on scene5
_cache = {}


def scene5(ora):
    """(flat scene, oracle accel, global indices, view) of hw09/scene5, made once"""
    if "scene5" not in _cache:
        flat = ora.load_crtscene(SCENE5)
        oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
        view = (np.asarray(flat.cam_pos, F).reshape(3), np.asarray(flat.cam_mat, F).reshape(9))
        _cache["scene5"] = (flat, oacc, global_indices(flat), view)
    return _cache["scene5"]


def first_hits(oacc, w, h):
    """The g-buffer planes of the oracle's camera rays (sample 0 of spp 1: the pixel centres) and closest hits with culling"""
    rays = oacc.camera_rays(w, h).reshape(-1, 6)
    hits = oacc.intersect(rays, True)
    hit = (hits["tri"] != MISS).reshape(h, w)
    pos = (rays[:, 0:3] + (hits["t"][:, None] * rays[:, 3:6]).astype(F)).astype(F).reshape(h, w, 3)
    return dict(tri=np.ascontiguousarray(hits["tri"].reshape(h, w), np.uint32),
                bary=np.ascontiguousarray(np.stack([hits["u"], hits["v"]], axis=1).reshape(h, w, 2), F),
                position=np.where(hit[..., None], pos, F(0.0)).astype(F), depth=np.ascontiguousarray(hits["t"].reshape(h, w), F),
                normal=np.where(hit[..., None], hits["normal"].reshape(h, w, 3), F(0.0)).astype(F),
                mesh=np.ascontiguousarray(hits["mesh"].reshape(h, w), np.uint32), hit=hit)


def planes(ora, w, h):
    """first_hits of scene5 at w x h, shared and left unchanged"""
    if (w, h) not in _cache:
        _cache[(w, h)] = first_hits(scene5(ora)[1], w, h)
    return _cache[(w, h)]


def moved_vertices(flat, mesh=MOVED_MESH, d=MOVE):
    """the scene's vertices with those of `mesh` translated by d"""
    starts = np.concatenate([[0], np.cumsum(flat.mesh_nverts)]).astype(np.int64)
    v = np.array(flat.vertices, F).reshape(-1, 3)
    v[starts[mesh]:starts[mesh + 1]] = (v[starts[mesh]:starts[mesh + 1]] + np.asarray(d, F)).astype(F)
    return np.ascontiguousarray(v)


def moved_oracle(ora, flat, vertices):
    return ora.Accel(ora.Scene(dataclasses.replace(flat, vertices=np.ascontiguousarray(vertices, F))), ora.ACCEL_KD_SIMD)


def hostile_planes(base, n_triangles, seed=11):
    """(name, tri, bary) over a frame's planes: ids n_triangles, 0xFFFFFFFE and 0xFFFFFFFF scattered among the valid ones, and
    barycentrics holding NaN, +-inf and 1e30 on a fifth of the pixels, hits among them"""
    rng = np.random.default_rng(seed)
    h, w = base["tri"].shape
    n = w * h
    tri = base["tri"].copy().reshape(-1)
    pick = rng.permutation(n)[: max(n // 5, min(n, 3))]
    tri[pick] = np.array([n_triangles, 0xFFFFFFFE, MISS], np.uint32)[np.arange(pick.size) % 3]
    # ... and valid ids where the frame had none, so that garbage barycentrics meet real triangles
    more = rng.permutation(n)[: n // 5]
    tri[more] = rng.integers(0, n_triangles, more.size).astype(np.uint32)
    yield "ids", tri.reshape(h, w), base["bary"]
    bary = base["bary"].copy().reshape(-1)
    bad = rng.permutation(bary.size)[: max(bary.size // 5, min(bary.size, 2))]
    bary[bad] = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F)[np.arange(bad.size) % 5]
    yield "barycentrics", base["tri"], bary.reshape(h, w, 2)
    yield "both", tri.reshape(h, w), bary.reshape(h, w, 2)


def temporal_inputs(cur, position, prev, view):
    """The two frames of the moving-mesh chain as tm.accumulate takes them: the new frame's guides with `position` in the place of
    its own, and the previous frame as a history whose every length is 1, so that a pixel that keeps its history ends with
    length 2 exactly (sum_l and sum_w are then the same sums).  The colours play no part: constant."""
    h, w = cur["tri"].shape
    grey = np.full((h, w, 3), 0.5, F)
    c = dict(rgb=grey, noise=None, position=np.ascontiguousarray(position, F), normal=cur["normal"], depth=cur["depth"], mesh=cur["mesh"])
    p = dict(rgb=grey, noise=None, length=np.ones((h, w), F), position=prev["position"], normal=prev["normal"], depth=prev["depth"],
             mesh=prev["mesh"], view=view)
    return c, p


def kept_share(length, cur, mesh=MOVED_MESH):
    """the share of `mesh`'s hit pixels of the new frame that ended with length 2"""
    on = cur["hit"] & (cur["mesh"] == mesh)
    assert on.sum() >= 100
    return float((np.asarray(length)[on] == 2.0).mean())
