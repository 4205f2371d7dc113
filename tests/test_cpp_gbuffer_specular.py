"""hip_accel::render_gbuffer_specular (simd-raytracer_amd/hip_accel.hpp), the C++ door to rtk_render_gbuffer_specular: it compiles
against the mock reference headers and forwards."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import specular_model as sm
from conftest import ROOT
from test_cpp_views import CAMS, _scene

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
# the columns of a printed pixel behind depth, tri, mesh, material, bounces
COLUMNS = (("position", 3), ("normal", 3), ("surface_position", 3), ("surface_normal", 3), ("albedo", 3), ("bary", 2), ("last_ray", 6))


def _build_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "gbuffer_specular_check")
    src = os.path.join(ROOT, "tests", "cpp", "gbuffer_specular_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h"), os.path.join(PKG, "librtk_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_adapter_refusals_need_no_device(rtk):
    """A call without planes and a sample outside [0, spp) throw before any device is asked for; then the call needs one: without
    it the adapter reports "no usable HIP device", with it the program runs to its end (test_adapter_results)."""
    res = subprocess.run([_build_check()], capture_output=True, text=True)
    assert "refused 2" in res.stdout, res.stdout + res.stderr
    if rtk.device_count() > 0:
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
def test_adapter_results(rtk, ora):
    out = subprocess.run([_build_check()], capture_output=True, text=True, check=True).stdout
    assert "refused 2" in out and "shape 3 16 16" in out
    rows = re.findall(r"view (\d) pixel (\d+)((?: [0-9a-f]{8}){28})", out)
    assert len(rows) == 3 * 256, out
    got = np.array([[int(x, 16) for x in r[2].split()] for r in rows], np.uint32).reshape(3, 256, 28)
    mirrored = 0
    for v, (pos, mat) in enumerate(CAMS):
        flat = dataclasses.replace(_scene(ora), cam_pos=np.array(pos, np.float32), cam_mat=np.array(mat, np.float32))
        m = sm.camera_planes(ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD), flat, 16, 16, 5)
        mirrored += int(((m["bounces"] > 0) & m["surface"]).sum())
        assert np.array_equal(got[v, :, 0], sm.u32(m["depth"])), v
        for col, name in ((1, "tri"), (2, "mesh"), (3, "material"), (4, "bounces")):
            assert np.array_equal(got[v, :, col], m[name]), (v, name)
        at = 5
        for name, comps in COLUMNS:
            assert np.array_equal(got[v, :, at:at + comps], sm.u32(m[name]).reshape(256, comps)), (v, name)
            at += comps
        if v == 2:
            assert not m["surface"].any()                                          # the third camera looks away
    assert mirrored >= 10                                                          # the floor, seen in the wall
    assert "two planes same 768 others empty 1 own camera same 256 of 256 views 1" in out, out
