"""The host plan of rtk_denoise_frame that needs no GPU to be judged: csrc/denoise_plan.hpp through its stand-alone check program
(tests/cpp/denoise_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "denoise_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + plan_check.csrc("denoise_plan.hpp")
LINES = ("refusals ok", "tiles ok", "steps ok", "knob ok", "workspace ok", "all ok")


def test_denoise_plan_refusals_tiles_steps_knob_and_workspace():
    """The refusals in the header's order; tiles that cover every pixel of every image exactly once and never span two images
    (37x19, 5x3, 1x1, 70x36 x 2, 130x70 x 3 and the largest shapes); halo, pitch and LDS bytes of every step; which steps are
    staged under RTK_DENOISE_LDS_MAX_STEP; a workspace of at most 64 B per pixel that is 64-bit safe at 2^31 pixels."""
    plan_check.run(plan_check.build("denoise_plan_check", PLAN_SRC, PLAN_DEPS), LINES)


def test_denoise_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("denoise_plan_check_san", PLAN_SRC, PLAN_DEPS, extra=plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
