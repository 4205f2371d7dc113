"""The host plan of rtk_render_motion that needs no GPU to be judged: csrc/motion_plan.hpp through its stand-alone check program
(tests/cpp/motion_plan_check.cpp), plain and with the host sanitizers, and its scalars against those that tests/ref_camera.py
makes camera rays from."""
import os
import re

import numpy as np

import plan_check
import temporal_model as tm
from conftest import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "motion_plan_check.cpp")
PLAN_DEPS = [PLAN_SRC, os.path.join(ROOT, "include", "rtk.h")] + \
    plan_check.csrc("motion_plan.hpp", "motion_math.hpp", "temporal_math.hpp", "camera_plan.hpp", "denoise_plan.hpp", "stage_plan.hpp")
FLAGS = ("-ffp-contract=off",)
LINES = ("refusals ok", "alignment ok", "scalars ok", "stage ok", "grid ok", "all ok")
SHAPES = ((1, 1, 90.0), (7, 5, 90.0), (64, 64, 90.0), (130, 70, 60.0), (1920, 1080, 73.5), (16384, 16384, 179.0), (3, 1000, 1.0))
ARGS = [str(v) for shape in SHAPES for v in shape]


def test_motion_plan_refusals_alignment_scalars_stage_and_grid():
    """The refusals in the header's order with the ends of every range; the alignment of every pointer of the device variant; the
    host variant's stage; tiles that give every pixel to one workgroup of a bounded grid, from 1x1 to 16384x16384.  The scalars
    the kernel gets are, bit for bit, those the camera rays of ref_camera.py are made from."""
    res = plan_check.run(plan_check.build("motion_plan_check", PLAN_SRC, PLAN_DEPS, FLAGS), LINES, ARGS)
    got = {(int(w), int(h)): tuple(int(x, 16) for x in words.split())
           for w, h, words in re.findall(r"scalars (\d+) (\d+): ([0-9a-f ]+)", res.stdout)}
    assert len(got) == len(SHAPES)
    for w, h, fov in SHAPES:
        want = tuple(int(np.float32(v).view(np.uint32)) for v in tm.scalars(w, h, fov))
        assert got[(w, h)] == want, (w, h, fov)


def test_motion_plan_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = plan_check.run(plan_check.build("motion_plan_check_san", PLAN_SRC, PLAN_DEPS, FLAGS, plan_check.SANITIZE), LINES, ARGS)
    plan_check.assert_sanitizers_quiet(res)
