"""rtk_accel_update_geometry / rtk_accel_update_geometry_device without a GPU: the symbols, the order of the checks (NULL first,
then the missing device -- there is no CPU path) and that a refused call leaves the accel's tree as it was."""
import ctypes

import numpy as np
import pytest

from conftest import SCENE5


def _arrays(rtk):
    sc = rtk.parse_scene_file(SCENE5)
    a = sc.arrays()
    return sc, np.ascontiguousarray(a["vertices"]), np.ascontiguousarray(a["indices"]), np.ascontiguousarray(a["mesh_ntris"])


def test_library_exports_the_geometry_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in ("rtk_accel_update_geometry", "rtk_accel_update_geometry_device"):
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    assert hasattr(rtk.KdTreeSimdAccel, "update_geometry") and hasattr(rtk.KdTreeSimdAccel, "update_geometry_device")


def test_null_arguments_come_before_the_device(rtk):
    sc, v, idx, nt = _arrays(rtk)
    acc = rtk.KdTreeSimdAccel(sc)
    before = acc.tree_dump()
    L = rtk.lib()
    V, I, N = v.ctypes.data, idx.ctypes.data, nt.ctypes.data
    assert L.rtk_accel_update_geometry(None, V, I, N) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_geometry(acc._h, None, I, N) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_geometry(acc._h, V, I, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_geometry(acc._h, V, None, N) == rtk.RTK_ERR_INVALID          # NULL indices with a positive total
    assert L.rtk_accel_update_geometry_device(None, V, I, N, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_geometry_device(acc._h, None, I, N, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_geometry_device(acc._h, V, I, None, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_update_geometry_device(acc._h, V, None, N, None) == rtk.RTK_ERR_INVALID
    with pytest.raises(rtk.RtkError) as e:
        acc.update_geometry_device(0, 0, nt)
    assert e.value.code == rtk.RTK_ERR_INVALID
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    assert acc.tree_info().n_triangles == int(nt.sum())


def test_the_wrapper_checks_shape_and_dtype(rtk):
    sc, v, idx, nt = _arrays(rtk)
    acc = rtk.KdTreeSimdAccel(sc)
    for bad_v in (v.astype(np.float64), v[:-1], v.reshape(-1)):
        with pytest.raises(ValueError):
            acc.update_geometry(bad_v, idx, nt)
    for bad_i in (idx.astype(np.int64), idx[:-1], idx.reshape(-1), idx.astype(np.float32)):
        with pytest.raises(ValueError):
            acc.update_geometry(v, bad_i, nt)
    for bad_n in (nt[:-1], nt.astype(np.float32), np.concatenate([nt, nt])):
        with pytest.raises(ValueError):
            acc.update_geometry(v, idx, bad_n)


def test_without_a_device_a_valid_call_is_no_device_and_changes_nothing(rtk):
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what a valid call does then is tests/test_gpu_geometry.py")
    sc, v, idx, nt = _arrays(rtk)
    acc = rtk.KdTreeSimdAccel(sc)
    before = acc.tree_dump()
    half = (nt // 2).astype(np.int32)
    cut = np.ascontiguousarray(np.concatenate([m[:k] for m, k in zip(np.split(idx, np.cumsum(nt)[:-1]), half)]))
    with pytest.raises(rtk.RtkError) as e:
        acc.update_geometry(v, cut, half)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    with pytest.raises(rtk.RtkError) as e:
        acc.update_geometry_device(v.ctypes.data, cut.ctypes.data, half)    # (never dereferenced: there is no device to launch on)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    with pytest.raises(rtk.RtkError) as e:
        acc.update_geometry(v, np.zeros((0, 3), np.uint32), np.zeros_like(nt))          # no triangles, no indices
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    bad = cut.copy()
    bad[0, 0] = 0xFFFFFFFF                                             # the missing device is reported before the arrays are looked at
    with pytest.raises(rtk.RtkError) as e:
        acc.update_geometry(v, bad, half)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    ti = acc.tree_info()
    assert (ti.n_nodes, ti.n_leaf_refs, ti.n_triangles) == (before[0].shape[0], before[2].shape[0], int(nt.sum()))
