"""csrc/batch_plan.hpp, the host's share of the ray repacking, through its stand-alone check program (plain and with the host
sanitizers): which batches are probed, forced into a sort or left alone at 2^18 and 2^32 rays, that a statistics call never
sorts, the wave strides of the probe and of the sort's own bounds pass, and what the verdict words make of the sorted walk --
strategy and unsorted key bits for 0..6 varying dimensions at the ends of every knob's range.  None of these changes a hit, so
no parity test sees them.  Needs no GPU."""
import os
import subprocess

import repack_model as rm
from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "batch_plan_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "batch_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]


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
    for line in ("thresholds ok", "stats ok", "strides ok", "verdict table ok", "all ok"):
        assert line in res.stdout, res.stdout
    return res


def test_batch_plan_thresholds_strides_and_verdict_table():
    _run(_build("batch_plan_check", []))


def test_batch_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run(_build("batch_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr and res.stderr == "", res.stderr


def test_the_models_strides_are_the_headers():
    """tests/repack_model.py restates the two stride formulas for the device tests; the check program pins these values too."""
    assert [rm.probe_stride(n) for n in (1, 1 << 18, 1 << 22, (1 << 22) + 1, 1 << 24)] == [16, 16, 16, 17, 64]
    assert [rm.sample_stride(n) for n in (1, 1 << 18, (1 << 18) + 1, 1 << 24)] == [1, 1, 2, 64]
    assert [rm.sort_from_bit(d) for d in range(7)] == [14, 14, 14, 6, 0, 0, 0]
