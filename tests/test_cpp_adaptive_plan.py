"""The host plan of rtk_render_adaptive that needs no GPU to be judged: csrc/adaptive_plan.hpp through its stand-alone check program
(tests/cpp/adaptive_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "adaptive_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + plan_check.csrc("adaptive_plan.hpp")
LINES = ("refusals ok", "checkpoints ok", "blocks ok", "chunks ok", "count ok", "all ok")


def test_adaptive_plan_refusals_checkpoints_blocks_and_chunks():
    """The refusals in the header's order; checkpoint schedules with a step that does not divide spp - min, min == spp, step > spp
    and sums past 2^31; the first round's block offsets of 70x36, 5x3 and other frames; chunk walks that cover every pixel of a
    round exactly once (2520 pixels by 1000, 2^31 by 2^20); the count word."""
    plan_check.run(plan_check.build("adaptive_plan_check", PLAN_SRC, PLAN_DEPS), LINES)


def test_adaptive_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("adaptive_plan_check_san", PLAN_SRC, PLAN_DEPS, extra=plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
