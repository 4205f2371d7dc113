"""The host plan of rtk_render_gbuffer_specular that needs no GPU to be judged: csrc/gbuffer_specular_plan.hpp through its stand-alone
check program (tests/cpp/gbuffer_specular_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "gbuffer_specular_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + plan_check.csrc("gbuffer_specular_plan.hpp", "gbuffer_plan.hpp")
LINES = ("masks ok", "refusals ok", "elements ok", "all ok")


def test_gbuffer_specular_plan_masks_refusals_and_elements():
    """The twelve plane masks in the struct's order, the refusals in the header's order with "no plane" in rtk_render_gbuffer's place,
    and element counts up to the largest call (2^56 pixels of 24 bytes)."""
    plan_check.run(plan_check.build("gbuffer_specular_plan_check", PLAN_SRC, PLAN_DEPS), LINES)


def test_gbuffer_specular_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("gbuffer_specular_plan_check_san", PLAN_SRC, PLAN_DEPS, extra=plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
