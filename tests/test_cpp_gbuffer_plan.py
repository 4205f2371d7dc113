"""The host plan of rtk_render_gbuffer that needs no GPU to be judged: csrc/gbuffer_plan.hpp through its stand-alone check program
(tests/cpp/gbuffer_plan_check.cpp), plain and with the host sanitizers."""
import os

import plan_check
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "gbuffer_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + plan_check.csrc("gbuffer_plan.hpp")
LINES = ("masks ok", "refusals ok", "units ok", "elements ok", "grids ok", "launches ok", "large ok", "all ok")


def test_gbuffer_plan_refusals_units_grids_and_launches():
    """Plane masks, the refusals in the header's order, blocks and workgroups of 1x1, 8x8, 9x7 and 70x45 views, element counts past
    2^32, two-dimensional grids, and the cut into launches of whole views: at a lowered limit and for 70,000 views of 3840x2160."""
    plan_check.run(plan_check.build("gbuffer_plan_check", PLAN_SRC, PLAN_DEPS), LINES)


def test_gbuffer_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("gbuffer_plan_check_san", PLAN_SRC, PLAN_DEPS, extra=plan_check.SANITIZE), LINES)
    plan_check.assert_sanitizers_quiet(res)
