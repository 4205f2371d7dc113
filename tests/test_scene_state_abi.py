"""rtk_accel_{get,set}_lights / _materials / _background without a GPU: the symbols, the getters of a fresh accel, round trips by
their bits on an accel that has never touched a device, the tree left alone, the order of the argument checks, and a refused
rtk_accel_set_materials that leaves the table byte-identical."""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENE5, SCENES
from scene_state_checks import LEAF_SIZES, ONLY_A, ONLY_B, TREE, leaves_of, octant_scene
from update_checks import _rtk_scene

SCENE4_TEX = os.path.join(SCENES, "hw12", "scene4.crtscene")
SYMBOLS = ("rtk_accel_get_lights", "rtk_accel_set_lights", "rtk_accel_set_lights_device", "rtk_accel_get_materials",
           "rtk_accel_set_materials", "rtk_accel_get_background", "rtk_accel_set_background")


def _accel(rtk, path=SCENE5):
    sc = rtk.parse_scene_file(path)
    return sc, rtk.KdTreeSimdAccel(sc)


def _mat_bytes(acc):
    m = acc.materials()
    return b"".join(m[k].tobytes() for k in ("kind", "albedo", "ior", "smooth", "texture"))


def test_library_exports_the_scene_state_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    for name in ("lights", "set_lights", "set_lights_device", "materials", "set_materials", "background", "set_background"):
        assert hasattr(rtk.KdTreeSimdAccel, name)
    assert rtk.LIGHT_DTYPE.itemsize == 16 and rtk.MATERIAL_DTYPE.itemsize == 32


@pytest.mark.parametrize("path", [SCENE5, SCENE4_TEX], ids=["scene5", "hw12_scene4"])
def test_getters_are_the_scenes_on_a_fresh_accel(rtk, path):
    sc, acc = _accel(rtk, path)
    a = sc.arrays()
    pos, inten = acc.lights()
    assert pos.tobytes() == a["light_pos"].tobytes() and inten.tobytes() == a["light_intensity"].tobytes() and len(inten) > 0
    m = acc.materials()
    for k, key in (("kind", "mat_kind"), ("albedo", "mat_albedo"), ("ior", "mat_ior"), ("smooth", "mat_smooth"), ("texture", "mat_texture")):
        assert m[k].tobytes() == a[key].tobytes(), k
    assert acc.background().tobytes() == a["background"].tobytes()
    if path == SCENE4_TEX:
        assert (m["kind"] == rtk.MAT_TEXTURE).any() and (m["texture"][m["kind"] == rtk.MAT_TEXTURE] >= 0).all()


def test_round_trips_keep_the_bits_without_a_device(rtk):
    _, acc = _accel(rtk)
    before = acc.tree_dump()
    n0 = len(acc.lights()[1])
    # background: -0.0 and a denormal
    bg = np.array([-0.0, 3.0e-41, 0.75], np.float32)
    assert np.signbit(bg[0]) and 0 < bg[1] < np.finfo(np.float32).tiny
    acc.set_background(bg)
    assert acc.background().tobytes() == bg.tobytes()
    # lights: more than built with, -0.0, a denormal, NaN / inf / negative / zero intensities; then none; then one
    n = n0 + 5
    rng = np.random.default_rng(3)
    pos = rng.normal(size=(n, 3)).astype(np.float32)
    pos[0] = [-0.0, 3.0e-41, 1e30]
    inten = rng.uniform(1, 100, n).astype(np.float32)
    inten[:5] = [np.nan, np.inf, -3.5, 0.0, -0.0]
    acc.set_lights(pos, inten)
    p, i = acc.lights()
    assert p.tobytes() == pos.tobytes() and i.tobytes() == inten.tobytes() and np.isnan(i[0]) and np.signbit(i[4])
    acc.set_lights(np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
    p, i = acc.lights()
    assert p.shape == (0, 3) and i.shape == (0,)
    acc.set_lights(pos[:1], inten[:1])
    assert acc.lights()[0].tobytes() == pos[:1].tobytes()
    # a partial fetch: the count is the table's, the rows the first `cap`
    acc.set_lights(pos, inten)
    cnt = ctypes.c_int32(0)
    part = np.zeros(2, rtk.LIGHT_DTYPE)
    assert rtk.lib().rtk_accel_get_lights(acc._h, part.ctypes.data, 2, ctypes.byref(cnt)) == rtk.RTK_OK
    assert cnt.value == n and part["position"].tobytes() == pos[:2].tobytes()
    # materials: every kind but texture (the scene has no textures), `reserved` dropped, texture forced to -1
    m = acc.materials()
    k = len(m["kind"])
    kind = np.array([(j + 1) % 4 for j in range(k)], np.int32)
    albedo = rng.uniform(0, 1, (k, 3)).astype(np.float32)
    albedo[0] = [-0.0, 3.0e-41, np.nan]
    ior = rng.uniform(1, 2, k).astype(np.float32)
    smooth = np.array([j % 2 for j in range(k)], np.int32)
    acc.set_materials(kind, albedo, ior, smooth, texture=np.full(k, 7, np.int32))
    got = acc.materials()
    assert got["kind"].tobytes() == kind.tobytes() and got["albedo"].tobytes() == albedo.tobytes()
    assert got["ior"].tobytes() == ior.tobytes() and got["smooth"].tobytes() == smooth.tobytes()
    assert (got["texture"] == -1).all()
    tab = np.zeros(k, rtk.MATERIAL_DTYPE)
    tab["reserved"] = 99
    assert rtk.lib().rtk_accel_set_materials(acc._h, tab.ctypes.data, k) == rtk.RTK_OK
    back = np.full(k, 5, rtk.MATERIAL_DTYPE)
    assert rtk.lib().rtk_accel_get_materials(acc._h, back.ctypes.data) == rtk.RTK_OK
    assert (back["reserved"] == 0).all() and (back["texture"] == -1).all() and (back["kind"] == 0).all()
    # the tree depends on none of it
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    for bad in ((pos[:, :2], inten), (pos, inten[:-1]), (pos.reshape(-1), inten)):
        with pytest.raises(ValueError):
            acc.set_lights(*bad)
    with pytest.raises(ValueError):
        acc.set_background(bg[:2])
    with pytest.raises(ValueError):
        acc.set_materials(kind[:-1], albedo, ior, smooth)
    with pytest.raises(ValueError):
        acc.set_materials(kind, albedo[:, :2], ior, smooth)


def test_argument_errors_in_their_order(rtk):
    _, acc = _accel(rtk)
    L = rtk.lib()
    INV = rtk.RTK_ERR_INVALID
    lights = np.zeros(3, rtk.LIGHT_DTYPE)
    cnt = ctypes.c_int32(0)
    assert L.rtk_accel_get_lights(None, lights.ctypes.data, 3, ctypes.byref(cnt)) == INV
    assert L.rtk_accel_get_lights(acc._h, lights.ctypes.data, 3, None) == INV
    assert L.rtk_accel_get_lights(acc._h, None, 0, ctypes.byref(cnt)) == rtk.RTK_OK and cnt.value > 0
    for call in (lambda a, p, n: L.rtk_accel_set_lights(a, p, n), lambda a, p, n: L.rtk_accel_set_lights_device(a, p, n, None)):
        assert call(None, lights.ctypes.data, 3) == INV
        assert call(acc._h, lights.ctypes.data, -1) == INV
        assert call(acc._h, None, 3) == INV
    assert L.rtk_accel_set_lights(acc._h, None, 0) == rtk.RTK_OK            # n == 0 needs no pointer
    k = acc.scene.info.n_materials
    mats = np.zeros(k + 1, rtk.MATERIAL_DTYPE)
    mats["kind"] = 9                                                          # bad kinds behind a wrong n: the count is judged first
    assert L.rtk_accel_get_materials(None, mats.ctypes.data) == INV
    assert L.rtk_accel_get_materials(acc._h, None) == INV
    assert L.rtk_accel_set_materials(None, mats.ctypes.data, k) == INV
    assert L.rtk_accel_set_materials(acc._h, None, k) == INV
    for n in (k + 1, k - 1, 0, -1):
        assert L.rtk_accel_set_materials(acc._h, mats.ctypes.data, n) == INV
        assert b"number of materials" in L.rtk_last_error()
    assert L.rtk_accel_set_materials(acc._h, mats.ctypes.data, k) == INV
    assert b"type unknown" in L.rtk_last_error()
    bg = np.zeros(3, np.float32)
    assert L.rtk_accel_get_background(None, bg.ctypes.data) == INV
    assert L.rtk_accel_get_background(acc._h, None) == INV
    assert L.rtk_accel_set_background(None, bg.ctypes.data) == INV
    assert L.rtk_accel_set_background(acc._h, None) == INV


def test_a_refused_set_materials_changes_nothing(rtk):
    sc, acc = _accel(rtk, SCENE4_TEX)
    n_tex = sc.info.n_textures
    assert n_tex >= 2
    before = _mat_bytes(acc)
    m = acc.materials()
    k = len(m["kind"])
    tex_mat = int(np.flatnonzero(m["kind"] == rtk.MAT_TEXTURE)[0])

    def refused(**change):
        kw = {key: m[key].copy() for key in ("kind", "albedo", "ior", "smooth", "texture")}
        kw["albedo"][:] = 0.123                                               # would be visible had anything been written
        for key, (idx, val) in change.items():
            kw[key][idx] = val
        with pytest.raises(rtk.RtkError) as e:
            acc.set_materials(**kw)
        assert e.value.code == rtk.RTK_ERR_INVALID
        assert _mat_bytes(acc) == before

    refused(kind=(k - 1, 5))                                                  # the LAST row: everything before it was valid
    refused(kind=(k - 1, -1))
    refused(texture=(tex_mat, n_tex))
    refused(texture=(tex_mat, -1))
    tab = np.zeros(k, rtk.MATERIAL_DTYPE)
    assert rtk.lib().rtk_accel_set_materials(acc._h, tab.ctypes.data, k - 1) == rtk.RTK_ERR_INVALID
    assert _mat_bytes(acc) == before
    # a valid swap of texture indices, and a texture material that becomes diffuse and texture again
    tex = m["texture"].copy()
    tex[tex_mat] = (tex[tex_mat] + 1) % n_tex
    acc.set_materials(m["kind"], m["albedo"], m["ior"], m["smooth"], tex)
    assert acc.materials()["texture"][tex_mat] == tex[tex_mat]
    kind = m["kind"].copy()
    kind[tex_mat] = rtk.MAT_DIFFUSE
    acc.set_materials(kind, m["albedo"], m["ior"], m["smooth"], tex)
    assert acc.materials()["texture"][tex_mat] == -1
    acc.set_materials(m["kind"], m["albedo"], m["ior"], m["smooth"], m["texture"])
    assert _mat_bytes(acc) == before
    # a scene without textures cannot gain a texture material
    _, plain = _accel(rtk)
    pm = plain.materials()
    pbefore = _mat_bytes(plain)
    kind = pm["kind"].copy()
    kind[0] = rtk.MAT_TEXTURE
    with pytest.raises(rtk.RtkError) as e:
        plain.set_materials(kind, pm["albedo"], pm["ior"], pm["smooth"], np.zeros(len(kind), np.int32))
    assert e.value.code == rtk.RTK_ERR_INVALID and _mat_bytes(plain) == pbefore


def test_without_a_device_only_the_device_variant_needs_one(rtk):
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what the calls do then is tests/test_gpu_scene_state.py")
    _, acc = _accel(rtk)
    pos, inten = acc.lights()
    with pytest.raises(rtk.RtkError) as e:
        acc.set_lights_device(pos.ctypes.data, 1)                             # (never dereferenced: there is no device to copy on)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    acc.set_lights(pos[:1] + 1, inten[:1])                                    # the host setters never need one, and the refused call left it usable
    assert acc.lights()[0].tobytes() == (pos[:1] + 1).tobytes()
    m = acc.materials()
    kind = m["kind"].copy()
    kind[0] = rtk.MAT_REFRACTIVE
    acc.set_materials(kind, m["albedo"], m["ior"], m["smooth"])
    assert acc.materials()["kind"][0] == rtk.MAT_REFRACTIVE
    acc.set_background([0.1, 0.2, 0.3])
    with pytest.raises(rtk.RtkError) as e:
        acc.render_frame(rtk.RenderConfig(width=8, height=8))
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE


def test_octant_scene_has_the_leaves_it_promises(rtk, ora):
    flat, tri_octant, tri_owner = octant_scene(ora)
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), **TREE)
    _, link, refs = acc.tree_dump()
    leaves = leaves_of(link, refs)
    assert sorted(len(l) for l in leaves) == sorted(LEAF_SIZES)
    for l in leaves:
        o = set(tri_octant[l].tolist())
        assert len(o) == 1
        o = o.pop()
        assert len(l) == LEAF_SIZES[o]
        owners = set(tri_owner[l].tolist())
        assert owners == ({0} if o in (0, ONLY_A) else {1} if o == ONLY_B else {0, 1})
    assert {1, 63, 64, 65} <= {len(l) for l in leaves} and max(len(l) for l in leaves) > 128
