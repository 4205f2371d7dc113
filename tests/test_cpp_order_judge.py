"""csrc/order_judge.hpp, the rule by which a newly sorted launch order is kept or dropped after one frame, and what
csrc/frame_plan.hpp OrderState gained with it -- the re-sort interval that doubles up to a cap, the frames a judge goes behind, the
workgroup count that is pending again behind a judge -- through their stand-alone check program, plain and with the host
sanitizers.  None of this changes a pixel, so no frame test sees it.  Needs no GPU."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "order_judge_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "order_judge.hpp"), os.path.join(PKG, "csrc", "frame_plan.hpp"), os.path.join(ROOT, "include", "rtk.h")]


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
    for line in ("rule ok", "schedule ok", "count ok", "all ok"):
        assert line in res.stdout, res.stdout
    return res


def test_order_judge_rule_schedule_and_rearmed_count():
    """The rule: a challenger faster, equal, one tick slower, slower; no champion yet; a score of 0 on either side; the champion's
    score refreshed by a sort; both forced verdicts; the score from two clock readings.  The schedule with the cap at 64 (sorts at
    2, 18, 34, 66, 130, then every 64 frames; judges at all but the first), restarted by forget() and by another shape, at 128, 48,
    16 and 8, and with the cap at 0 or left out the sequences of frame_plan_check.cpp; restart_schedule() in mid-segment, right behind
    a sort, with the cap at 0 and on a fresh state.  The count: 0 from the judge on until the
    new read-back is seen, then the new word."""
    _run(_build("order_judge_check", []))


def test_order_judge_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run(_build("order_judge_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr and res.stderr == "", res.stderr
