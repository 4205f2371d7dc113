"""hip_accel::set_lights / lights_now, set_materials / materials_now, set_background / background_now
(simd-raytracer_amd/hip_accel.hpp), the C++ door to rtk_accel_set_lights / _set_materials / _set_background."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_views import _scene

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def _build_scene_state_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "scene_state_check")
    src = os.path.join(ROOT, "tests", "cpp", "scene_state_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_setters_need_no_device_and_the_first_frame_throws_without_one(rtk):
    exe = _build_scene_state_check()
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what the program answers then is test_scene_state_results")
    res = subprocess.run([exe], capture_output=True, text=True)
    assert "round trip 1 refused 1" in res.stdout, res.stdout + res.stderr
    assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


def _states(ora):
    """The states of scene_state_check.cpp."""
    s0 = _scene(ora)
    s1 = dataclasses.replace(s0, light_pos=np.array([[2, 2.5, -1], [-1.5, 1, -3]], np.float32), light_intensity=np.array([90, -0.0], np.float32))
    s2 = dataclasses.replace(s1, mat_kind=np.array([ora.MAT_DIFFUSE, ora.MAT_REFRACTIVE], np.int32),
                             mat_albedo=np.array([[0.2, 0.7, 0.4], [0, 0, 0]], np.float32), mat_ior=np.array([1.0, 1.5], np.float32),
                             mat_smooth=np.array([1, 0], np.int32))
    s3 = dataclasses.replace(s2, background=np.array([-0.0, 0.125, 0.5], np.float32))
    return [s0, s1, s2, s3]


@pytest.mark.gpu
def test_scene_state_results(rtk, ora):
    out = subprocess.run([_build_scene_state_check()], capture_output=True, text=True, check=True).stdout
    assert "round trip 1 refused 1" in out
    rows = re.findall(r"state (\d) pixel (\d+) ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8})", out)
    assert len(rows) == 4 * 256, out
    got = np.array([[int(x, 16) for x in r[2:]] for r in rows], np.uint32).reshape(4, 256, 3)
    frames = []
    for k, flat in enumerate(_states(ora)):
        ref, ocn = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(16, 16, 1, 5, 0)
        assert np.array_equal(got[k], ref.reshape(-1, 3).view(np.uint32)), k
        assert f"state {k} rays {ocn['rays']}\n" in out, k
        frames.append(ref)
    for a, b in zip(frames, frames[1:]):
        assert not np.array_equal(a.view(np.uint32), b.view(np.uint32))
