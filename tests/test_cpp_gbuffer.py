"""hip_accel::render_gbuffer (simd-raytracer_amd/hip_accel.hpp), the C++ door to rtk_render_gbuffer."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_views import CAMS, _scene

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
MISS = 0xFFFFFFFF


def _build_gbuffer_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "gbuffer_check")
    src = os.path.join(ROOT, "tests", "cpp", "gbuffer_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h"), os.path.join(PKG, "librtk_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_render_gbuffer_adapter_refusals_need_no_device(rtk):
    """A call without planes and a sample outside [0, spp) throw before any device is asked for; then the call needs one: without
    it the adapter reports "no usable HIP device", with it the program runs to its end (test_render_gbuffer_adapter_results)."""
    res = subprocess.run([_build_gbuffer_check()], capture_output=True, text=True)
    assert "refused 2" in res.stdout, res.stdout + res.stderr
    if rtk.device_count() > 0:
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
def test_render_gbuffer_adapter_results(rtk, ora):
    out = subprocess.run([_build_gbuffer_check()], capture_output=True, text=True, check=True).stdout
    assert "refused 2" in out and "shape 3 16 16" in out
    rows = re.findall(r"view (\d) pixel (\d+)((?: [0-9a-f]{8}){15})", out)
    assert len(rows) == 3 * 256, out
    got = np.array([[int(x, 16) for x in r[2].split()] for r in rows], np.uint32).reshape(3, 256, 15)
    hits = 0
    for v, (pos, mat) in enumerate(CAMS):
        flat = dataclasses.replace(_scene(ora), cam_pos=np.array(pos, np.float32), cam_mat=np.array(mat, np.float32))
        oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
        rays = oacc.camera_rays(16, 16).reshape(-1, 6)
        ref = oacc.intersect(rays, True)
        hit = ref["tri"] != MISS
        hits += int(hit.sum())
        u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)           # noqa: E731
        assert np.array_equal(got[v, :, 0], u32(ref["t"])), v
        assert np.array_equal(got[v, :, 1], ref["tri"]) and np.array_equal(got[v, :, 2], ref["mesh"]), v
        material = np.where(hit, flat.mesh_material[np.where(hit, ref["mesh"], 0)].astype(np.uint32), np.uint32(MISS))
        assert np.array_equal(got[v, :, 3], material), v
        position = (rays[:, 0:3] + (ref["t"][:, None] * rays[:, 3:6]).astype(np.float32)).astype(np.float32)
        assert np.array_equal(got[v, :, 4:7], u32(np.where(hit[:, None], position, np.float32(0)))), v
        assert np.array_equal(got[v, :, 7:10], u32(np.where(hit[:, None], ref["normal"], np.float32(0)))), v
        albedo = np.where(hit[:, None], flat.mat_albedo[np.where(hit, material, 0)], flat.background[None, :])
        assert np.array_equal(got[v, :, 10:13], u32(albedo)), v
        assert np.array_equal(got[v, :, 13], u32(ref["u"])) and np.array_equal(got[v, :, 14], u32(ref["v"])), v
        if v == 2:
            assert not hit.any()                                                   # the third camera looks away
    assert hits > 100
    assert "depth only same 768 others empty 1 own camera same 256 of 256 views 1" in out, out
