"""hip_accel::render_motion (simd-raytracer_amd/hip_accel.hpp), the C++ door to rtk_render_motion."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
# The scene's coordinates lie below 8, where one ulp of a float is 4.8e-7.  position is o + t * d (two roundings per component),
# prev_position the barycentric sum (six), the translation one more on either side: ten ulps bound their difference, 4.8e-6.
POSITION_TOL = 4.8e-6
# A pixel of the 16 x 16 frame spans 1 / 8 of the image plane at depth 1: the position error above, at a depth of at least 1,
# moves the projection by less than 8 * 4.8e-6 px; the projection's own seven roundings of values below 16 add 7 * 9.5e-7.
MOTION_TOL = 8 * 4.8e-6 + 7 * 9.5e-7


def _build_motion_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "motion_check")
    src = os.path.join(ROOT, "tests", "cpp", "motion_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h"), os.path.join(PKG, "librtk_hip.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_render_motion_adapter_refusals_need_no_device(rtk):
    """A g-buffer without tri and bary planes, a view it does not have and a wrong vertex count throw before any device is asked
    for; then the call needs one: without it the adapter reports "no usable HIP device", with it the program runs to its end."""
    res = subprocess.run([_build_motion_check()], capture_output=True, text=True)
    assert "refused 3" in res.stdout, res.stdout + res.stderr
    if rtk.device_count() > 0:
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
def test_render_motion_adapter_results(rtk):
    out = subprocess.run([_build_motion_check()], capture_output=True, text=True, check=True).stdout
    assert "refused 3" in out and "shape 16 16 planes 768 512 768 0" in out, out
    hits, misses, good = (int(x) for x in re.search(r"hits (\d+) misses (\d+) good misses (\d+)", out).groups())
    assert hits >= 64 and misses >= 16 and good == misses, out
    own_err, own_motion = (float(x) for x in re.search(r"own pose: position error (\S+) motion (\S+)", out).groups())
    back_err = float(re.search(r"moved back: position error (\S+)", out).group(1))
    print(out)
    assert own_err <= POSITION_TOL and back_err <= POSITION_TOL
    assert own_motion <= MOTION_TOL
