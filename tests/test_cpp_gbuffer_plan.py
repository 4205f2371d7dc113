"""The host plan of rtk_render_gbuffer that needs no GPU to be judged: csrc/gbuffer_plan.hpp through its stand-alone check program
(tests/cpp/gbuffer_plan_check.cpp), plain and with the host sanitizers."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "gbuffer_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(PKG, "csrc", "gbuffer_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]
LINES = ("masks ok", "refusals ok", "units ok", "elements ok", "grids ok", "launches ok", "large ok", "all ok")


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
    for line in LINES:
        assert line in res.stdout, res.stdout
    return res


def test_gbuffer_plan_refusals_units_grids_and_launches():
    """Plane masks, the refusals in the header's order, blocks and workgroups of 1x1, 8x8, 9x7 and 70x45 views, element counts past
    2^32, two-dimensional grids, and the cut into launches of whole views: at a lowered limit and for 70,000 views of 3840x2160."""
    _run_plan_check(_build_plan_check("gbuffer_plan_check", []))


def test_gbuffer_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run_plan_check(_build_plan_check("gbuffer_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
