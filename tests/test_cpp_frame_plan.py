"""csrc/frame_plan.hpp, the launch decisions of a frame, through its stand-alone check program (plain and with the host
sanitizers): the engine trial of RTK_TRACE_AUTO, the first-frame prior, the re-sort cadence, the read-back workgroup count, the
capacity of the cost tables, eight waves for few blocks, the cut of a views call and the growth of the streaming workspace.
None of these changes a pixel, so no frame test sees them.  Needs no GPU."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "frame_plan_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "frame_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]


def _stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if _stale(exe, DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), SRC, "-o", exe])
    return exe


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout + res.stderr
    for line in ("trial ok", "order ok", "capacity ok", "geometry and views ok", "stream workspace ok", "all ok"):
        assert line in res.stdout, res.stdout
    return res


def test_frame_plan_trial_order_capacity_views_and_workspace():
    """The trial's frames 1-3 and both verdicts, a tie, events not ready for two frames, abandon on frame 1, a new signature from
    every state, trials off, a stats frame in between; the order for 40 frames at resort_every 16 and 1 (prior, sort at 2, 18,
    34), another shape at frame 5 and back, forget(), everything that suppresses the prior, table growth; the workgroup count 0
    until the read-back is seen and after the next sort; capacity at native below, above and beyond 2^24; views_launches at
    per_view <, =, > limit; the workspace growing one field at a time and its refusal bound (frame_plan_check.cpp has the numbers)."""
    _run(_build("frame_plan_check", []))


def test_frame_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run(_build("frame_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr and res.stderr == "", res.stderr
