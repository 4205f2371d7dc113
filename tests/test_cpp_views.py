"""hip_accel::set_camera / camera_now / render_views (simd-raytracer_amd/hip_accel.hpp), the C++ door to rtk_accel_set_camera and
rtk_render_views."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def _build_views_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "views_check")
    src = os.path.join(ROOT, "tests", "cpp", "views_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_set_camera_needs_no_device_and_render_views_throws_without_one(rtk):
    exe = _build_views_check()
    if rtk.device_count() > 0:
        pytest.skip("a device is present: what the program answers then is test_render_views_results")
    res = subprocess.run([exe], capture_output=True, text=True)
    assert "round trip 1" in res.stdout, res.stdout + res.stderr
    assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


CAMS = [([0, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0, 1]),
        ([1, 0.5, 0.25], [0.96, 0, 0.28, 0, 1, 0, -0.28, 0, 0.96]),
        ([0, 0, 0], [-1, 0, 0, 0, 1, 0, 0, 0, -1])]


def _scene(ora):
    """The scene of views_check.cpp."""
    return ora.FlatScene(
        mesh_material=np.array([0, 1], np.int32), mesh_nverts=np.array([4, 4], np.int32), mesh_ntris=np.array([2, 2], np.int32),
        vertices=np.array([[-3, -1, 0], [3, -1, 0], [3, -1, -6], [-3, -1, -6],
                           [-1.5, -1, -4], [1.5, -1, -4], [1.5, 1, -4], [-1.5, 1, -4]], np.float32),
        indices=np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3]], np.uint32),
        mat_kind=np.array([ora.MAT_DIFFUSE, ora.MAT_REFLECTIVE], np.int32),
        mat_albedo=np.array([[0.9, 0.6, 0.3], [1, 1, 1]], np.float32), mat_ior=np.array([1.0, 1.0], np.float32),
        mat_smooth=np.zeros(2, np.int32), light_pos=np.array([[0, 3, -2]], np.float32),
        light_intensity=np.array([150], np.float32), cam_pos=np.zeros(3, np.float32),
        cam_mat=np.eye(3, dtype=np.float32).reshape(-1), background=np.array([0.25, 0.5, 0.75], np.float32),
        width=16, height=16, bucket_size=64)


@pytest.mark.gpu
def test_render_views_results(rtk, ora):
    out = subprocess.run([_build_views_check()], capture_output=True, text=True, check=True).stdout
    assert "round trip 1" in out and "no views 0" in out
    rows = re.findall(r"view (\d) pixel (\d+) ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8})", out)
    assert len(rows) == 3 * 256, out
    got = np.array([[int(x, 16) for x in r[2:]] for r in rows], np.uint32).reshape(3, 256, 3)
    rays = 0
    frames = []
    for v, (pos, mat) in enumerate(CAMS):
        flat = dataclasses.replace(_scene(ora), cam_pos=np.array(pos, np.float32), cam_mat=np.array(mat, np.float32))
        ref, ocn = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(16, 16, 1, 5, 0)
        assert np.array_equal(got[v], ref.reshape(-1, 3).view(np.uint32)), v
        rays += ocn["rays"]
        frames.append(ref)
    assert not np.array_equal(frames[0], frames[1]) and len(np.unique(frames[2].reshape(-1, 3), axis=0)) == 1   # the third looks away
    assert f"same 768 rays {rays} of {rays} primary 768" in out
