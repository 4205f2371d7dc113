"""rtk_accel_get_camera / _set_camera and rtk_render_views[_device] without a GPU: the symbols, the camera of an accel that has
never touched a device, and the order of the argument checks (what a frame refuses, then the views' own, then n_views == 0,
then the missing device)."""
import ctypes

import numpy as np
import pytest

from conftest import SCENE5

SYMBOLS = ("rtk_accel_get_camera", "rtk_accel_set_camera", "rtk_render_views", "rtk_render_views_device")


def _accel(rtk):
    sc = rtk.parse_scene_file(SCENE5)
    return sc, rtk.KdTreeSimdAccel(sc)


def test_library_exports_the_view_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    for name in ("camera", "set_camera", "render_views", "render_views_device"):
        assert hasattr(rtk.KdTreeSimdAccel, name)


def test_get_camera_is_the_scenes(rtk):
    sc, acc = _accel(rtk)
    a = sc.arrays()
    pos, mat = acc.camera()
    assert pos.tobytes() == a["cam_pos"].tobytes() and mat.tobytes() == a["cam_mat"].tobytes()
    assert np.abs(mat).sum() > 0


def test_set_get_round_trip_keeps_the_bits_without_a_device(rtk):
    _, acc = _accel(rtk)
    before = acc.tree_dump()
    v = np.array([1.5, -0.0, 3.0e-41, -1.0, 0.0, -0.0, 0.25, 7.0, -2.5, 1e30, -1e-30, 0.1], np.float32)   # -0.0 and a denormal
    assert np.signbit(v[1]) and np.signbit(v[5])
    acc.set_camera(v[:3], v[3:])
    pos, mat = acc.camera()
    assert np.concatenate([pos, mat]).tobytes() == v.tobytes()
    w = -v
    acc.set_camera(w[:3], w[3:].reshape(3, 3))
    pos, mat = acc.camera()
    assert np.concatenate([pos, mat]).tobytes() == w.tobytes()
    for x, y in zip(before, acc.tree_dump()):                      # the tree does not depend on the camera
        assert x.tobytes() == y.tobytes()
    with pytest.raises(ValueError):
        acc.set_camera(v[:2], v[3:])


def test_null_camera_arguments(rtk):
    _, acc = _accel(rtk)
    L = rtk.lib()
    v = np.zeros(12, np.float32)
    assert L.rtk_accel_get_camera(None, v.ctypes.data) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_get_camera(acc._h, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_set_camera(None, v.ctypes.data) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_set_camera(acc._h, None) == rtk.RTK_ERR_INVALID


def test_view_argument_errors_in_their_order(rtk):
    _, acc = _accel(rtk)
    L = rtk.lib()
    views = np.zeros((2, 12), np.float32)
    out = np.zeros((2, 8, 8, 3), np.float32)
    V, O = views.ctypes.data, out.ctypes.data

    def host(p, v, n, o):
        return L.rtk_render_views(acc._h, ctypes.byref(p), v, n, o, None)

    def dev(p, v, n, o):
        return L.rtk_render_views_device(acc._h, ctypes.byref(p), v, n, o, None)

    ok = rtk.RenderConfig(width=8, height=8)
    for call in (host, dev):
        assert L.rtk_render_views(None, ctypes.byref(ok.to_c()), V, 2, O, None) == rtk.RTK_ERR_INVALID
        assert L.rtk_render_views_device(None, ctypes.byref(ok.to_c()), V, 2, O, None) == rtk.RTK_ERR_INVALID
        # what a frame refuses comes first, whatever the views are (n_views == 0 and NULL pointers included)
        for bad in (rtk.RenderConfig(width=8, height=8, spp=0), rtk.RenderConfig(width=70000, height=8),
                    rtk.RenderConfig(width=8, height=8, trace_mode=99), rtk.RenderConfig(width=8, height=8, max_ray_depth=17),
                    rtk.RenderConfig(width=8, height=8, spp=2, sample_begin=2)):
            assert call(bad.to_c(), V, 2, O) == rtk.RTK_ERR_INVALID
            assert call(bad.to_c(), None, 0, None) == rtk.RTK_ERR_INVALID
        # then the views' own
        assert call(ok.to_c(), V, -1, O) == rtk.RTK_ERR_INVALID
        assert call(rtk.RenderConfig(width=8, height=8, world_size=2).to_c(), V, 2, O) == rtk.RTK_ERR_INVALID
        assert call(rtk.RenderConfig(width=8, height=8, world_size=2).to_c(), V, 0, O) == rtk.RTK_ERR_INVALID   # before n_views == 0
        assert call(ok.to_c(), None, 2, O) == rtk.RTK_ERR_INVALID
        assert call(ok.to_c(), V, 2, None) == rtk.RTK_ERR_INVALID
        # then n_views == 0: nothing to do, device or not, pointers or not
        assert call(ok.to_c(), None, 0, None) == rtk.RTK_OK
        assert call(ok.to_c(), V, 0, O) == rtk.RTK_OK
    assert not out.any()
    rgb, cn = acc.render_views(ok, np.zeros((0, 12), np.float32))
    assert rgb.shape == (0, 8, 8, 3) and cn["rays"] == 0
    for bad in (views.astype(np.float64), views[:, :11], views.reshape(-1)):
        with pytest.raises(ValueError):
            acc.render_views(ok, bad)


def test_without_a_device_views_are_no_device_and_the_camera_still_moves(rtk):
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what a valid call does then is tests/test_gpu_views.py")
    _, acc = _accel(rtk)
    views = np.zeros((2, 12), np.float32)
    views[:, 3] = views[:, 7] = views[:, 11] = 1.0
    cfg = rtk.RenderConfig(width=8, height=8)
    with pytest.raises(rtk.RtkError) as e:
        acc.render_views(cfg, views)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    with pytest.raises(rtk.RtkError) as e:
        acc.render_views_device(cfg, views.ctypes.data, 2, views.ctypes.data)      # (never dereferenced: there is no device to launch on)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    acc.set_camera(views[0, :3] + 1, views[0, 3:])                                 # needs no device, and the refused calls left it usable
    assert acc.camera()[0].tolist() == [1.0, 1.0, 1.0]
