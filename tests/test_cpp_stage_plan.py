"""The layout of the host variants' staging buffer that needs no GPU to be judged: csrc/stage_plan.hpp through its stand-alone check
program (tests/cpp/stage_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "stage_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + plan_check.csrc("stage_plan.hpp", "gbuffer_plan.hpp")
LINES = ("temporal ok", "gbuffer ok", "bytes ok", "empty ok", "grid ok", "large ok", "all ok")


def test_stage_plan_layouts_invariants_and_large_sums():
    """Layouts worked out by hand: the sixteen planes of a temporal call with the noise planes, the mesh planes and the whole history
    absent in turn; the g-buffer with each single plane and with all eight; byte planes of 1, 4, 5 and 257 bytes; a present plane
    of size zero; nothing present.  Over a grid of sizes and presence masks: no two present planes overlap, every offset is a
    multiple of the alignment, the total holds every plane, an absent plane is null and takes no room.  Exact sums at 2^31 pixels
    of 17 words; sums that leave 64 bits, or one plane too many, are refused and never wrapped."""
    plan_check.run(plan_check.build("stage_plan_check", PLAN_SRC, PLAN_DEPS), LINES)


def test_stage_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("stage_plan_check_san", PLAN_SRC, PLAN_DEPS, extra=plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
