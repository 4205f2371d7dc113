"""tests/specular_model.py against geometry, on the CPU: what rtk_render_gbuffer_specular's contract promises for planar mirrors --
`position` and `normal` are the mirror image of the shaded point and of its normal -- holds for the model the GPU tests compare
with.  These tests run the model alone (over the CPU oracle's hits): they pass or fail with it, with or without the feature."""
import numpy as np

import material_scenes as ms
import specular_model as sm
from views_checks import with_camera

W, H = ms.SIZE
BIAS = 1e-4
_cache = {}


def _planes(ora, depth=5):
    if depth not in _cache:
        flat = ms.make_scene(ora, "ior15_075")
        _cache[depth] = sm.camera_planes(ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD), flat, W, H, depth, reflection_bias=BIAS)
    return _cache[depth]


# cameras as rtk_view: position, then the matrix
BEHIND_THE_QUADS = np.array([0, 3, -5.2, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)        # between the upper quads and the back mirror, facing it
AT_THE_RIGHT_MIRROR = np.array([6, 1, 5, 0, 0, 1, 0, 1, 0, -1, 0, 0], np.float32)       # between the side mirrors, turned to the right one


def _view(ora, cam):
    f = with_camera(ms.make_scene(ora, "ior15_075"), cam)
    return sm.camera_planes(ora.Accel(ora.Scene(f), ora.ACCEL_KD_SIMD), f, W, H, 5, reflection_bias=BIAS)


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _mirror_chain(m, *mirrors):
    """pixels whose chain is exactly these mirrors, in this order, and then a surface"""
    k = len(mirrors)
    sel = (m["bounces"] == k) & m["surface"] & (m["reflections"] == k)
    for i, mesh in enumerate(mirrors):
        sel &= m["chain_mesh"][:, i] == mesh
    return sel


def test_one_bounce_off_the_back_mirror_is_the_mirror_image(ora):
    """Single-bounce pixels on the back mirror (the plane z = -6): position is (x, y, -12 - z) of surface_position within
    reflection_bias + 64 ulp(L) -- one bias step along the ray and the handful of roundings in L and o + L d -- and normal is
    surface_normal with z negated, within 8 ulp of 1.  The scene's camera sees the back mirror in a gap between the quads; a camera
    behind the quads sees little else."""
    for cam, least in ((None, 16), (BEHIND_THE_QUADS, 500)):
        _check_back_mirror(ora, cam, least)


def _check_back_mirror(ora, cam, least):
    m = _planes(ora) if cam is None else _view(ora, cam)
    back = _mirror_chain(m, ms.MIRROR_BACK)
    assert back.sum() >= least, int(back.sum())
    sp, vp = m["surface_position"][back].astype(np.float64), m["position"][back].astype(np.float64)
    image = np.stack([sp[:, 0], sp[:, 1], -12.0 - sp[:, 2]], axis=1)
    bound = BIAS + 64 * _ulp(m["depth"][back])
    err = np.linalg.norm(vp - image, axis=1)
    print("back mirror pixels", int(back.sum()), "largest error", err.max(), "smallest bound", bound.min())
    assert (err <= bound).all(), (err.max(), bound.min())
    sn, vn = m["surface_normal"][back].astype(np.float64), m["normal"][back].astype(np.float64)
    assert np.abs(vn - sn * np.array([1.0, 1.0, -1.0])).max() <= 8 * float(np.spacing(np.float32(1.0)))
    assert len(np.unique(m["mesh"][back])) >= 3


def test_two_bounces_between_the_side_mirrors_are_the_double_image(ora):
    """Two reflections, off one side mirror (x = -8: x -> -16 - x; x = 8: x -> 16 - x) and then off the other: the image of the
    image, x + 32 seen right-then-left and x - 32 seen left-then-right, within 2 reflection_bias + 64 ulp(L); the normal is the
    surface normal again (x negated twice).  The scene's camera sees few such chains: a camera between the mirrors, turned
    towards the right one, sees many."""
    m = _view(ora, AT_THE_RIGHT_MIRROR)
    seen = 0
    for mirrors, shift in (((ms.MIRROR_RIGHT, ms.MIRROR_LEFT), 32.0), ((ms.MIRROR_LEFT, ms.MIRROR_RIGHT), -32.0)):
        sel = _mirror_chain(m, *mirrors)
        if not sel.any():
            continue
        seen += int(sel.sum())
        sp, vp = m["surface_position"][sel].astype(np.float64), m["position"][sel].astype(np.float64)
        image = np.stack([sp[:, 0] + shift, sp[:, 1], sp[:, 2]], axis=1)
        bound = 2 * BIAS + 64 * _ulp(m["depth"][sel])
        err = np.linalg.norm(vp - image, axis=1)
        print(mirrors, "pixels", int(sel.sum()), "largest error", err.max(), "smallest bound", bound.min())
        assert (err <= bound).all(), (err.max(), bound.min())
        sn, vn = m["surface_normal"][sel].astype(np.float64), m["normal"][sel].astype(np.float64)
        assert np.abs(vn - sn).max() <= 8 * float(np.spacing(np.float32(1.0)))
    assert seen >= 16, seen


def test_the_models_own_invariants(ora):
    """k == 0 pixels hold the first hit; NO SURFACE pixels hold the miss values; bounces never pass the limit; a frame's pixel is the
    albedo plane where the chain is mirrors alone and ends on the constant quad or on nothing (render.hpp:239-250, :302-303)."""
    flat = ms.make_scene(ora, "ior15_075")
    oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
    for depth in (1, 5, 16):
        m = _planes(ora, depth)
        assert m["bounces"].max() <= depth
        direct = (m["bounces"] == 0) & m["surface"]
        hits = oacc.intersect(m["camera_rays"], True)
        assert sm.same_bits(m["depth"][direct], hits["t"][direct]) and np.array_equal(m["tri"][direct], hits["tri"][direct])
        assert sm.same_bits(m["normal"][direct], np.ascontiguousarray(hits["normal"][direct]))
        assert sm.same_bits(m["position"][direct], m["surface_position"][direct])
        none = ~m["surface"]
        assert (m["depth"][none] == -1).all() and not m["position"][none].any() and (m["tri"][none] == sm.MISS).all()
        assert (m["albedo"][none] == flat.background).all()
        frame = oacc.render(W, H, 1, depth, 0)[0].reshape(-1, 3)
        pure = (m["refractions"] == 0) & (m["tirs"] == 0)
        sel = pure & (none | (m["end_kind"] == sm.CONSTANT))
        assert sel.sum() > 100 and frame[sel].tobytes() == m["albedo"][sel].tobytes()
