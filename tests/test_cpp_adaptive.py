"""hip_accel::render_adaptive (simd-raytracer_amd/hip_accel.hpp), the C++ door to rtk_render_adaptive."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cpp_views import _scene

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def _build_adaptive_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "adaptive_check")
    src = os.path.join(ROOT, "tests", "cpp", "adaptive_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h"), os.path.join(PKG, "librtk_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_render_adaptive_adapter_refusals_need_no_device(rtk):
    """min_samples above spp and a negative threshold throw before any device is asked for; then the call needs one: without it the
    adapter reports "no usable HIP device", with it the program runs to its end (test_render_adaptive_adapter_results)."""
    res = subprocess.run([_build_adaptive_check()], capture_output=True, text=True)
    assert "refused 2" in res.stdout, res.stdout + res.stderr
    if rtk.device_count() > 0:
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
def test_render_adaptive_adapter_results(rtk, ora):
    """every pixel is the CPU oracle's pixel of the frame with spp = its sample count (16 x 16, depth 3, two GI rays)"""
    out = subprocess.run([_build_adaptive_check()], capture_output=True, text=True, check=True).stdout
    assert "refused 2" in out and "shape 16 16 samples 256 noise 256" in out
    rows = re.findall(r"pixel (\d+) (\d+) ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8})", out)
    assert len(rows) == 256, out
    samples = np.array([int(r[1]) for r in rows], np.uint32).reshape(16, 16)
    rgb = np.array([[int(x, 16) for x in r[2:5]] for r in rows], np.uint32).reshape(16, 16, 3)
    noise = np.array([int(r[5], 16) for r in rows], np.uint32).view(np.float32).reshape(16, 16)
    assert set(np.unique(samples).tolist()) <= {2, 3, 4}
    for y in (0, 8):
        for x in (0, 8):
            assert (samples[y:y + 8, x:x + 8] == samples[y, x]).all()
    oacc = ora.Accel(ora.Scene(_scene(ora)), ora.ACCEL_KD_SIMD)
    for n in np.unique(samples).tolist():
        ref, _ = oacc.render(16, 16, n, 3, 2)
        mask = samples == n
        assert np.array_equal(rgb[mask], ref.view(np.uint32)[mask]), n
    assert np.isfinite(noise).all() and (noise >= 0).all() and noise.max() > 0
    rays, primary = (int(x) for x in re.search(r"rays (\d+) primary (\d+)", out).groups())
    assert primary == int(samples.sum()) and rays > primary
