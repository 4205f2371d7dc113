"""Occlusion queries that leave a bundle-culled leaf at the next 64-triangle pass once answered (trace.hip.hpp,
leaf_range_bundle, `exit_t`).  The shortcut only runs with RTK_SHADOW_EARLY_EXIT on (the default, read when an accel is
made); frames must be the same bits with it off, where every query is traced to its end."""
import os

import numpy as np
import pytest

from conftest import SCENE2, SCENE5


def _accel(rtk, path, early_exit):
    old = os.environ.get("RTK_SHADOW_EARLY_EXIT")
    os.environ["RTK_SHADOW_EARLY_EXIT"] = "1" if early_exit else "0"
    try:
        return rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    finally:
        if old is None:
            del os.environ["RTK_SHADOW_EARLY_EXIT"]
        else:
            os.environ["RTK_SHADOW_EARLY_EXIT"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("path,cfg", [
    (SCENE5, dict(width=1920, height=1080, spp=1, max_ray_depth=5)),                      # bench.py's config 2
    (SCENE2, dict(width=480, height=270, spp=1, max_ray_depth=10, diffuse_rays=1)),       # diffuse GI
])
def test_frames_equal_with_and_without_early_exit(rtk, path, cfg):
    frames = []
    for early_exit in (False, True):
        acc = _accel(rtk, path, early_exit)
        first, _ = acc.render_frame(rtk.RenderConfig(**cfg))
        second, _ = acc.render_frame(rtk.RenderConfig(**cfg))          # second frame: the cost-ordered launch
        frames.append((first, second))
    (a, a2), (b, b2) = frames
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a2.view(np.uint32), b2.view(np.uint32))
