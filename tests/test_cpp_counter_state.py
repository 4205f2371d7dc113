"""csrc/frame_plan.hpp CounterState, the host half of an accel's two counter blocks, through its stand-alone check program (plain
and with the host sanitizers): three frames on one stream (fill, none, none), a stream switch, every other user of the counters
between two frames, an error in the middle, a shape change, and 40 frames across the re-sorts at 18 and 34.  For each frame it
asserts which block is current, whether a fill is issued and whether the kernel is handed the other block.  Then the two sets of
launch lists of OrderState across the re-sorts at 18 and 34 (sorted behind frames 17 and 33), at resort_every 1, and behind a new
shape, forget() and a growth of the tables: which set a frame reads and which a sort writes.  Needs no GPU."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "counter_state_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "frame_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]
GROUPS = ("one stream ok", "stream switch ok", "interleaved ok", "error ok", "shapes and resorts ok", "list sets ok", "all ok")


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), SRC, "-o", exe])
    return exe


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout + res.stderr
    for line in GROUPS:
        assert line in res.stdout, res.stdout
    return res


def test_counter_state_sequences():
    """Every sequence of tests/cpp/counter_state_check.cpp, which has the expected block, fill and hand-over of each frame."""
    _run(_build("counter_state_check", []))


def test_counter_state_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run(_build("counter_state_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert res.stderr == "", res.stderr
