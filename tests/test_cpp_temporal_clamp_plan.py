"""The host plan of rtk_temporal_accumulate_clamped that needs no GPU to be judged: csrc/temporal_clamp_plan.hpp through its
stand-alone check program (tests/cpp/temporal_clamp_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "temporal_clamp_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + \
    plan_check.csrc("temporal_clamp_plan.hpp", "temporal_plan.hpp", "temporal_math.hpp", "camera_plan.hpp", "denoise_plan.hpp")
FLAGS = ("-ffp-contract=off",)
LINES = ("ranges ok", "order ok", "lds 1: 324 pixels, 6480 bytes", "lds 2: 400 pixels, 8000 bytes", "lds 3: 484 pixels, 9680 bytes",
         "lds ok", "all ok")


def test_temporal_clamp_plan_ranges_order_aliasing_and_lds():
    """The ends of the ranges of radius, gamma and history_keep; the refusals in the header's order, from the parameters to the
    device variant's alignment; both aliasing refusals, which the plain call does not have; the LDS of a tile with its halo for
    every radius."""
    plan_check.run(plan_check.build("temporal_clamp_plan_check", PLAN_SRC, PLAN_DEPS, FLAGS), LINES)


def test_temporal_clamp_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("temporal_clamp_plan_check_san", PLAN_SRC, PLAN_DEPS, FLAGS, plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
