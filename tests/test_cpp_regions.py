"""The host side of rtk_render_regions that needs no GPU to be judged: csrc/regions_plan.hpp through its stand-alone check program
(plain and with the host sanitizers), and hip_accel::render_regions / render_regions_into (simd-raytracer_amd/hip_accel.hpp), the
C++ door to the call, which takes the reference's render_tile."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "regions_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(PKG, "csrc", "regions_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]


def _stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)


def _build_plan_check(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if _stale(exe, PLAN_DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), PLAN_SRC, "-o", exe])
    return exe


def _run_plan_check(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout + res.stderr
    for line in ("units ok", "packed ok", "launches ok", "validity ok", "large ok", "all ok"):
        assert line in res.stdout, res.stdout
    m = re.search(r"sweep (\d+) lists (\d+) overlapping ok", res.stdout)
    assert m and int(m.group(1)) == 2000 and 0 < int(m.group(2)) < 2000, res.stdout
    return res


def test_regions_plan_units_offsets_launches_and_sweep():
    """Unit counts and prefixes of ragged rectangles, packed offsets, the cut into launches at 150 units, and the sweep against
    the pairwise check on 2,000 seeded lists (regions_plan_check.cpp has the numbers)."""
    _run_plan_check(_build_plan_check("regions_plan_check", []))


def test_regions_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run_plan_check(_build_plan_check("regions_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr


def _build_regions_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "regions_check")
    src = os.path.join(ROOT, "tests", "cpp", "regions_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h"), os.path.join(PKG, "librtk_hip.so")]
    if _stale(exe, deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_render_regions_adapter_without_pixels_needs_no_device(rtk):
    """No tiles and tiles without pixels return at once, a tile past the frame is refused; with pixels the call needs a device:
    without one the adapter throws, with one the program runs to its end (test_render_regions_adapter_results reads the rest)."""
    res = subprocess.run([_build_regions_check()], capture_output=True, text=True)
    assert "no tiles 0 hollow 2 6 0" in res.stdout and "past the frame refused 1" in res.stdout, res.stdout + res.stderr
    if rtk.device_count() > 0:
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 3 and "exception rtk: no usable HIP device" in res.stdout, res.stdout + res.stderr


PACKED_TILES = [(1, 2, 12, 9), (8, 6, 16, 16), (15, 0, 16, 1), (4, 4, 4, 9), (0, 11, 16, 12)]      # regions_check.cpp's


def _scene(ora):
    """The scene of regions_check.cpp (and views_check.cpp)."""
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
def test_render_regions_adapter_results(rtk, ora):
    out = subprocess.run([_build_regions_check()], capture_output=True, text=True, check=True).stdout
    ref, ocn = ora.Accel(ora.Scene(_scene(ora)), ora.ACCEL_KD_SIMD).render(16, 16, 1, 5, 0)
    ref_bits = ref.reshape(-1, 3).view(np.uint32)
    assert len(np.unique(ref_bits, axis=0)) > 8                              # floor, mirror and background are in the picture
    shapes = re.findall(r"tile (\d) shape (\d+) (\d+)", out)
    assert [(int(h), int(w)) for _, h, w in shapes] == [(y1 - y0, x1 - x0 if y1 > y0 else 0) for x0, y0, x1, y1 in PACKED_TILES], out
    rows = re.findall(r"tile (\d) pixel (\d+) ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8})", out)
    want = [(t, y * 16 + x) for t, (x0, y0, x1, y1) in enumerate(PACKED_TILES) for y in range(y0, y1) for x in range(x0, x1)]
    assert [(int(r[0]), int(r[1])) for r in rows] == want
    for r in rows:
        assert [int(v, 16) for v in r[2:]] == ref_bits[int(r[1])].tolist(), r
    n = len(want)
    assert n == 174 and f"packed same {n} of {n} primary {n}" in out, out
    assert "in frame same 146 of 146 outside kept 110 of 110 primary 146" in out, out
    assert f"quarters rays {ocn['rays']} frame rays {ocn['rays']} primary 256" in out, out
