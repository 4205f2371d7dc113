"""rtk_accel_update_vertices / rtk_accel_update_vertices_device without a GPU: the symbols, the order of the checks (NULL first,
then the missing device -- there is no CPU path) and the Python wrapper's own checks."""
import ctypes

import numpy as np
import pytest

from conftest import SCENE5


def test_library_exports_the_update_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in ("rtk_accel_update_vertices", "rtk_accel_update_vertices_device"):
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4


def test_null_arguments_come_before_the_device(rtk):
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    v = np.zeros((acc.scene.info.n_vertices, 3), np.float32)
    L = rtk.lib()
    assert L.rtk_accel_update_vertices(None, v.ctypes.data) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_vertices(acc._h, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_vertices_device(None, v.ctypes.data, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_vertices_device(acc._h, None, None) == rtk.RTK_ERR_INVALID
    with pytest.raises(rtk.RtkError) as e:
        acc.update_vertices_device(0)
    assert e.value.code == rtk.RTK_ERR_INVALID


def test_the_wrapper_checks_shape_and_dtype(rtk):
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    n = acc.scene.info.n_vertices
    for bad in (np.zeros((n, 3), np.float64), np.zeros((n, 3), np.int32), np.zeros((n - 1, 3), np.float32),
                np.zeros((n, 4), np.float32), np.zeros((n * 3,), np.float32), np.zeros((3, n), np.float32)):
        with pytest.raises(ValueError):
            acc.update_vertices(bad)


def test_without_a_device_a_valid_call_is_no_device_and_changes_nothing(rtk):
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what a valid call does then is tests/test_gpu_update.py")
    sc = rtk.parse_scene_file(SCENE5)
    acc = rtk.KdTreeSimdAccel(sc)
    before = acc.tree_dump()
    v = np.ascontiguousarray(sc.arrays()["vertices"] * np.float32(1.5))
    with pytest.raises(rtk.RtkError) as e:
        acc.update_vertices(v)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    with pytest.raises(rtk.RtkError) as e:
        acc.update_vertices_device(v.ctypes.data)                    # (never dereferenced: there is no device to launch on)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    v[0, 0] = np.nan                                                 # the missing device is reported before the coordinates are looked at
    with pytest.raises(rtk.RtkError) as e:
        acc.update_vertices(v)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    ti = acc.tree_info()
    assert (ti.n_nodes, ti.n_leaf_refs) == (before[0].shape[0], before[2].shape[0])
