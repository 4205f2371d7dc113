"""stream_plan.hpp (csrc): how a STREAM frame's samples are cut into batches and a radiance call's rays into chunks, and how
many of them are in flight -- the arithmetic that sizes the streaming pipeline's queues.  Plain integer code, so it is tested
without a device: tests/cpp/stream_plan_check.cpp holds plans derived by hand and sweeps the rules' invariants (the node bound of
a launch, the memory budget of all lanes, every sample and every ray covered exactly once)."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "simd-raytracer_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def _stream_plan_check():
    """g++ and the one header: no HIP, no librtk_hip.so."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "stream_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "stream_plan_check.cpp")
    deps = [src, os.path.join(CSRC, "stream_plan.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, src, "-o", exe])
    return exe


def test_pins_and_invariants():
    res = subprocess.run([_stream_plan_check()], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.fullmatch(r"pins (\d+) ok\nframe plans (\d+) ok\nradiance plans (\d+) ok\n", res.stdout)
    assert m, res.stdout
    pins, frames, radiance = map(int, m.groups())
    # every pin ran, and the sweeps were the few thousand combinations they are meant to be
    assert pins == 14 and frames > 5000 and radiance > 3000
