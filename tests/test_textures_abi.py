"""The textures and uvs of a live accel without a GPU: the nine symbols, rtk_texture's layout, the ABI version, rtk.h's wording, the
getters of a fresh accel and round trips through the Python bindings on accels that have never touched a device (the C-ABI's
refusals one by one: tests/cpp/textures_check.cpp)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, SCENE5, SCENES
from texture_checks import ALBEDO, BITMAP, CHECKER, Tex, check_table, dense_uvs, set_textures, textures_of, with_textures

SCENE4_TEX = os.path.join(SCENES, "hw12", "scene4.crtscene")
SYMBOLS = ("rtk_accel_get_textures", "rtk_accel_get_texture_pixels", "rtk_accel_set_textures", "rtk_accel_set_texture_pixels",
           "rtk_accel_set_texture_pixels_device", "rtk_accel_set_texture_frame_device", "rtk_accel_get_uvs", "rtk_accel_set_uvs",
           "rtk_accel_set_uvs_device")


def test_library_exports_the_texture_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    assert len(SYMBOLS) == 9
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS, name
    assert rtk.abi_version() == 4
    for name in ("textures", "set_textures", "texture_pixels", "set_texture_pixels", "set_texture_pixels_device",
                 "set_texture_frame_device", "uvs", "set_uvs", "set_uvs_device"):
        assert hasattr(rtk.KdTreeSimdAccel, name), name


def test_rtk_texture_is_40_bytes(rtk):
    class Texture(ctypes.Structure):                      # rtk.h, field by field
        _fields_ = [("kind", ctypes.c_int32), ("color_a", ctypes.c_float * 3), ("color_b", ctypes.c_float * 3), ("param", ctypes.c_float),
                    ("width", ctypes.c_int32), ("height", ctypes.c_int32)]
    assert ctypes.sizeof(Texture) == 40 == rtk.TEXTURE_DTYPE.itemsize
    want = dict(kind=0, color_a=4, color_b=16, param=28, width=32, height=36)
    for name, off in want.items():
        assert getattr(Texture, name).offset == off and rtk.TEXTURE_DTYPE.fields[name][1] == off, name
    # ... and the library writes its rows at that stride with the fields at those offsets
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE4_TEX))
    raw = np.full(40 * 4 + 8, 0xAB, np.uint8)
    n = ctypes.c_int32(0)
    assert rtk.lib().rtk_accel_get_textures(acc._h, raw.ctypes.data, 4, ctypes.byref(n)) == rtk.RTK_OK and n.value == 4
    assert (raw[160:] == 0xAB).all()
    rows = raw[:160].view(rtk.TEXTURE_DTYPE)
    tex = acc.scene.arrays()
    assert rows["kind"].tolist() == tex["tex_kind"].tolist()
    b = int(np.flatnonzero(rows["kind"] == BITMAP)[0])
    assert (rows["width"][b], rows["height"][b]) == tuple(tex["tex_bitmap"][b][1:])


def test_the_header_points_to_the_new_section():
    text = open(os.path.join(ROOT, "include", "rtk.h")).read()
    assert "cannot gain a texture material" not in text
    assert "textures and uvs of a live accel" in text
    for name in SYMBOLS:
        assert name + "(" in text, name


@pytest.mark.parametrize("path", [SCENE5, SCENE4_TEX], ids=["scene5", "hw12_scene4"])
def test_getters_are_the_scenes_on_a_fresh_accel(rtk, ora, path):
    flat = ora.load_crtscene(path)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    check_table(acc, flat)
    assert acc.uvs().tobytes() == dense_uvs(flat).tobytes()
    if path == SCENE5:
        assert len(acc.textures()["kind"]) == 0 and not acc.uvs().any()
    else:
        assert BITMAP in acc.textures()["kind"] and acc.uvs().any()


def test_round_trips_without_a_device(rtk, ora):
    flat = ora.load_crtscene(SCENE4_TEX)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE4_TEX))
    before = acc.tree_dump()
    rng = np.random.default_rng(5)
    own = textures_of(flat)
    texs = [Tex(BITMAP, pixels=rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)), Tex(BITMAP, pixels=rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)),
            Tex(CHECKER, (-0.0, 0.5, np.nan), (np.inf, 0.0, 1.0), 0.0), own[[t.kind for t in own].index(BITMAP)], Tex(ALBEDO, (0.1, 0.2, 0.3))]
    state = with_textures(flat, texs)
    set_textures(acc, state)
    check_table(acc, state)
    for shape in ((2, 7, 3), (64, 64, 3), (1, 1, 3), (5, 3, 3)):
        texs[1] = Tex(BITMAP, pixels=rng.integers(0, 256, shape, dtype=np.uint8))
        acc.set_texture_pixels(1, texs[1].pixels)
        check_table(acc, with_textures(flat, texs))
    with pytest.raises(rtk.RtkError) as e:
        acc.set_texture_pixels(2, texs[1].pixels)                              # a checker
    assert e.value.code == rtk.RTK_ERR_INVALID
    with pytest.raises(rtk.RtkError) as e:
        acc.set_textures([CHECKER])                                             # materials use textures 1..3
    assert e.value.code == rtk.RTK_ERR_INVALID
    check_table(acc, with_textures(flat, texs))
    uv = rng.uniform(-2, 2, acc.uvs().shape).astype(np.float32)
    uv[0] = [-0.0, np.nan]
    acc.set_uvs(uv)
    assert acc.uvs().tobytes() == uv.tobytes()
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    for bad in (uv[:-1], uv[:, :1], uv.reshape(-1)):
        with pytest.raises(ValueError):
            acc.set_uvs(bad)
    with pytest.raises(ValueError):
        acc.set_texture_pixels(1, np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        acc.set_textures([CHECKER, ALBEDO], color_a=np.zeros((1, 3)))


def test_without_a_device_only_the_device_variants_need_one(rtk):
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what the calls do then is tests/test_gpu_textures.py")
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE4_TEX))
    b = int(np.flatnonzero(acc.textures()["kind"] == BITMAP)[0])
    px, uv = acc.texture_pixels(b), acc.uvs()
    for call in (lambda: acc.set_texture_pixels_device(b, 2, 2, px.ctypes.data), lambda: acc.set_texture_frame_device(b, 2, 2, uv.ctypes.data),
                 lambda: acc.set_uvs_device(uv.ctypes.data)):                  # (never dereferenced: there is no device to copy on)
        with pytest.raises(rtk.RtkError) as e:
            call()
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    assert acc.texture_pixels(b).tobytes() == px.tobytes() and acc.uvs().tobytes() == uv.tobytes()
    acc.set_texture_pixels(b, px[:3, :5])                                       # the refused calls left it usable
    assert acc.texture_pixels(b).tobytes() == np.ascontiguousarray(px[:3, :5]).tobytes()
