"""The host half of rtk_render_frame_noise that needs no GPU to be judged: csrc/frame_noise_plan.hpp and csrc/frame_noise_math.hpp
through their stand-alone check program (tests/cpp/frame_noise_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "frame_noise_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + plan_check.csrc("frame_noise_plan.hpp", "frame_noise_math.hpp", "adaptive_plan.hpp")
FLAGS = ("-ffp-contract=off",)                 # the statistic is compiled as the library compiles it
LINES = ("refusals ok", "plan ok", "x < 0 by rounding", "math ok", "all ok")


def test_frame_noise_plan_and_math():
    """The refusals in the header's order; 16 B of workspace per pixel, 64-bit safe; which batch starts and which ends the sums; the
    overflow redo as an adaptive call with one checkpoint; the statistic: a constant y gives exactly 0, a constant y whose x rounds
    below zero gives 0 and not NaN, a NaN stays one, and twenty sequences agree with a long-double recomputation."""
    plan_check.run(plan_check.build("frame_noise_plan_check", PLAN_SRC, PLAN_DEPS, FLAGS), LINES)


def test_frame_noise_plan_and_math_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("frame_noise_plan_check_san", PLAN_SRC, PLAN_DEPS, FLAGS, plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
