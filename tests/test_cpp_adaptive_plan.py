"""The host plan of rtk_render_adaptive that needs no GPU to be judged: csrc/adaptive_plan.hpp through its stand-alone check program
(tests/cpp/adaptive_plan_check.cpp), plain and with the host sanitizers."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "adaptive_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(PKG, "csrc", "adaptive_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]
LINES = ("refusals ok", "checkpoints ok", "blocks ok", "chunks ok", "count ok", "all ok")


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


def test_adaptive_plan_refusals_checkpoints_blocks_and_chunks():
    """The refusals in the header's order; checkpoint schedules with a step that does not divide spp - min, min == spp, step > spp
    and sums past 2^31; the first round's block offsets of 70x36, 5x3 and other frames; chunk walks that cover every pixel of a
    round exactly once (2520 pixels by 1000, 2^31 by 2^20); the count word."""
    _run_plan_check(_build_plan_check("adaptive_plan_check", []))


def test_adaptive_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run_plan_check(_build_plan_check("adaptive_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
