"""The host half of rtk_render_frame_noise that needs no GPU to be judged: csrc/frame_noise_plan.hpp and csrc/frame_noise_math.hpp
through their stand-alone check program (tests/cpp/frame_noise_plan_check.cpp), plain and with the host sanitizers."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "frame_noise_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + [os.path.join(PKG, "csrc", h) for h in
                                                                  ("frame_noise_plan.hpp", "frame_noise_math.hpp", "adaptive_plan.hpp")]
LINES = ("refusals ok", "plan ok", "x < 0 by rounding", "math ok", "all ok")


def _stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)


def _build_plan_check(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if _stale(exe, PLAN_DEPS):
        # -ffp-contract=off: the statistic is compiled as the library compiles it
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), PLAN_SRC, "-o", exe])
    return exe


def _run_plan_check(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout + res.stderr
    for line in LINES:
        assert line in res.stdout, res.stdout
    return res


def test_frame_noise_plan_and_math():
    """The refusals in the header's order; 16 B of workspace per pixel, 64-bit safe; which batch starts and which ends the sums; the
    overflow redo as an adaptive call with one checkpoint; the statistic: a constant y gives exactly 0, a constant y whose x rounds
    below zero gives 0 and not NaN, a NaN stays one, and twenty sequences agree with a long-double recomputation."""
    _run_plan_check(_build_plan_check("frame_noise_plan_check", []))


def test_frame_noise_plan_and_math_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run_plan_check(_build_plan_check("frame_noise_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
