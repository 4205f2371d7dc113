"""tests/cpp/textures_check.cpp: the C-ABI's textures and uvs of a live accel, and hip_accel::set_textures / textures_now /
set_texture_pixels / set_uvs / uvs_now (simd-raytracer_amd/hip_accel.hpp), on accels that were never resident.  Everything the
program does is host work, so it runs here without a GPU; once as built, once under the address and undefined-behaviour
sanitizers (a stand-alone program over the library as it is: the sanitizers see the program and the adapter header)."""
import os
import subprocess

import pytest

from conftest import ROOT, SCENE5, SCENES

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SCENE4_TEX = os.path.join(SCENES, "hw12", "scene4.crtscene")


def _build(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    src = os.path.join(ROOT, "tests", "cpp", "textures_check.cpp")
    deps = [src, os.path.join(PKG, "hip_accel.hpp"), os.path.join(ROOT, "include", "rtk.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([
            "g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
            "-I" + os.path.join(ROOT, "include"), "-I" + PKG, src, "-o", exe, "-L" + PKG, "-lrtk_hip",
            "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def _run(exe, env=None):
    res = subprocess.run([exe, SCENE4_TEX, SCENE5], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and "FAILED" not in res.stdout and ", 0 failed" in res.stdout, res.stdout + res.stderr
    return res


def test_textures_check():
    res = _run(_build("textures_check"))
    assert int(res.stdout.split("textures_check: ")[1].split()[0]) > 150


def test_textures_check_under_sanitizers(rtk):
    if rtk.device_count() > 0:
        pytest.skip("sanitizer runs stay off machines with a GPU; the same program runs unsanitized in test_textures_check")
    exe = _build("textures_check_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    # (the leak check is off: what the HIP runtime keeps for the life of the process is not the program's)
    res = _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
