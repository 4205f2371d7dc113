"""Wall time of three host variants of the C-ABI, staging included: render_gbuffer with all planes, render_frame_noise (2 spp) and
render_views with 4 views, hw09/scene5 at 1920x1080 on one accel.  Per call: the first call (the stage grows) and the median of
`repeats` further calls (the stage is reused).  Prints one JSON line; RTK_LIB_OVERRIDE chooses the library, so that two builds can
be timed in alternating processes.
usage: python tools/bench_host_stage.py [repeats]"""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rtk = importlib.import_module("simd-raytracer_amd")
    scene = rtk.parse_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "hw09", "scene5.crtscene"))
    acc = rtk.KdTreeSimdAccel(scene, device=0)
    cfg = rtk.RenderConfig(width=1920, height=1080, spp=1, max_ray_depth=5)
    pos, mat = acc.camera()
    views = np.stack([np.concatenate([pos + np.float32(0.01 * k), mat]) for k in range(4)]).astype(np.float32)
    acc.render_frame(cfg)                                   # the accel is resident and the device is warm before anything is timed
    calls = {"render_gbuffer": lambda: acc.render_gbuffer(cfg),
             "render_frame_noise": lambda: acc.render_frame_noise(rtk.RenderConfig(width=1920, height=1080, spp=2, max_ray_depth=5)),
             "render_views": lambda: acc.render_views(cfg, views)}
    out = {"lib": os.path.relpath(rtk.lib_path(), ROOT), "repeats": repeats}
    for name, call in calls.items():
        ms = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"first_ms": ms[0], "repeat_median_ms": statistics.median(ms[1:]), "repeat_ms": ms[1:]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
