"""rtk_accel_radiance / rtk_accel_radiance_device without a GPU: the symbols, the parameter block on both sides of ctypes, the order
of the argument checks (bad arguments first, then the empty batch, then the missing device) and the Python wrapper's own checks."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENE5


def test_library_exports_the_radiance_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in ("rtk_accel_radiance", "rtk_accel_radiance_device"):
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4


def test_radiance_params_have_the_same_size_on_both_sides(rtk, tmp_path):
    assert ctypes.sizeof(rtk.RadianceParams) == 36
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtk.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(rtk_radiance_params), offsetof(rtk_radiance_params, shadow_bias), offsetof(rtk_radiance_params, trace_mode)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    P = rtk.RadianceParams
    assert [int(x) for x in out] == [ctypes.sizeof(P), P.shadow_bias.offset, P.trace_mode.offset]
    text = open(os.path.join(ROOT, "include", "rtk.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} rtk_radiance_params;", text).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", fields)
    assert names == [n for n, _ in P._fields_]


def _bad_configs(rtk):
    R = rtk.RadianceConfig
    bad = [R(trace_mode=m) for m in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_GROUP4, rtk.TRACE_GROUP8, rtk.TRACE_GROUP16,
                                     rtk.TRACE_TWOPASS, rtk.TRACE_REPACK, -1, 99)]
    bad += [R(max_ray_depth=-1), R(max_ray_depth=17), R(diffuse_rays=-1), R(sample=-1)]
    bad += [R(shadow_bias=float("nan")), R(reflection_bias=float("inf")), R(refraction_bias=float("-inf"))]
    return bad


def test_argument_checks_come_before_the_device(rtk):
    """Bad arguments are RTK_ERR_INVALID with or without a device, and before n == 0 is looked at; an empty batch is RTK_OK with or
    without a device; only then does a machine without a GPU answer RTK_ERR_NO_DEVICE."""
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    rays = np.zeros((4, 6), np.float32)
    rays[:, 5] = -1.0
    for cfg in _bad_configs(rtk):
        for r in (rays, rays[:0]):
            with pytest.raises(rtk.RtkError) as e:
                acc.radiance(r, cfg=cfg)
            assert e.value.code == rtk.RTK_ERR_INVALID, cfg
            with pytest.raises(rtk.RtkError) as e:
                acc.radiance_device(0, 0, len(r), 0, cfg=cfg)
            assert e.value.code == rtk.RTK_ERR_INVALID, cfg
    L, p = rtk.lib(), rtk.RadianceConfig().to_c()
    rgb = np.zeros((4, 3), np.float32)
    assert L.rtk_accel_radiance(None, rays.ctypes.data, None, 4, ctypes.byref(p), rgb.ctypes.data, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_radiance(acc._h, rays.ctypes.data, None, 4, None, rgb.ctypes.data, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_radiance(acc._h, None, None, 4, ctypes.byref(p), rgb.ctypes.data, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_radiance(acc._h, rays.ctypes.data, None, 4, ctypes.byref(p), None, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_radiance_device(acc._h, None, None, 4, ctypes.byref(p), rgb.ctypes.data, None) == rtk.RTK_ERR_INVALID
    assert L.rtk_accel_radiance_device(acc._h, rays.ctypes.data, None, (1 << 32) + 1, ctypes.byref(p), rgb.ctypes.data, None) == rtk.RTK_ERR_INVALID
    # the empty batch: nothing touched, no device needed
    got, cn = acc.radiance(rays[:0])
    assert got.shape == (0, 3) and cn["rays"] == 0 and cn["primary"] == 0
    acc.radiance_device(0, 0, 0, 0)
    assert L.rtk_accel_radiance(acc._h, None, None, 0, ctypes.byref(p), None, None) == rtk.RTK_OK
    if rtk.device_count() > 0:
        return                                         # (with a device: tests/test_gpu_radiance.py)
    with pytest.raises(rtk.RtkError) as e:
        acc.radiance(rays)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    with pytest.raises(rtk.RtkError) as e:
        acc.radiance(rays, ids=np.arange(4, dtype=np.uint32), cfg=rtk.RadianceConfig(diffuse_rays=2, cull=False, trace_mode=rtk.TRACE_STREAM))
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    with pytest.raises(rtk.RtkError) as e:
        acc.radiance_device(rays.ctypes.data, 0, 4, rgb.ctypes.data)      # (never dereferenced: there is no device to launch on)
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE


def test_the_wrapper_checks_its_arguments(rtk):
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    rays = np.zeros((4, 6), np.float32)
    with pytest.raises(ValueError):
        acc.radiance(rays, ids=np.arange(3, dtype=np.uint32))
    with pytest.raises(ValueError):
        acc.radiance(rays, ids=np.array([0, 1, 2, -1]))
    with pytest.raises(ValueError):
        acc.radiance(rays, ids=np.array([0, 1, 2, 1 << 32]))
    with pytest.raises(ValueError):
        acc.radiance(rays, ids=np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        acc.radiance(np.zeros((4, 5), np.float32))
    c = rtk.RadianceConfig()
    assert (c.max_ray_depth, c.diffuse_rays, c.seed, c.sample, c.cull, c.trace_mode) == (5, 0, 42, 0, True, rtk.TRACE_AUTO)
    p = rtk.RadianceConfig(cull=False, sample=3, shadow_bias=0.5).to_c()
    assert (p.cull, p.sample, p.shadow_bias) == (0, 3, 0.5)
