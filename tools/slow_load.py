"""The reference's `dragon_slow_load` showcase (its README, Examples) through rtk_accel_update_geometry: the dragon of
hw09/scene5 revealed `--step` triangles per frame on ONE accel, every frame written as a PPM.  A demonstration, not a test.

Before rtk_accel_update_geometry every frame of this sequence was a new rtk_scene, a host build and a new accel.

    python tools/slow_load.py --out frames/ [--step 10] [--width 480 --height 270] [--every 1] [--limit 0]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE5 = os.path.join(ROOT, "tests", "golden", "scenes", "hw09", "scene5.crtscene")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory for frame_00000.ppm ...")
    ap.add_argument("--step", type=int, default=10, help="triangles revealed per frame")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--every", type=int, default=1, help="write every n-th frame")
    ap.add_argument("--limit", type=int, default=0, help="stop after this many frames (0: the whole dragon)")
    args = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("slow_load needs a HIP device: the rtk engine has no CPU path")
    scene = rtk.parse_scene_file(SCENE5)
    a = scene.arrays()
    lists = np.split(a["indices"], np.cumsum(a["mesh_ntris"])[:-1])
    dragon = int(np.argmax(a["mesh_ntris"]))
    n = len(lists[dragon])
    acc = rtk.KdTreeSimdAccel(scene)
    cfg = rtk.RenderConfig(width=args.width, height=args.height)
    os.makedirs(args.out, exist_ok=True)
    shown = list(range(0, n, max(1, args.step))) + [n]
    if args.limit > 0:
        shown = shown[: args.limit]
    t_update = t_frame = 0.0
    for f, k in enumerate(shown):
        cut = list(lists)
        cut[dragon] = lists[dragon][:k]
        t0 = time.perf_counter()
        acc.update_geometry(a["vertices"], np.ascontiguousarray(np.concatenate(cut)), np.array([len(t) for t in cut], np.int32))
        t1 = time.perf_counter()
        rgb, _ = acc.render_frame(cfg)
        t2 = time.perf_counter()
        t_update += t1 - t0
        t_frame += t2 - t1
        if f % max(1, args.every) == 0 or k == n:
            rtk.write_ppm(rgb, os.path.join(args.out, f"frame_{f:05d}.ppm"))
    print(f"{len(shown)} frames, {shown[-1]} of {n} triangles at the end: {1e3 * t_update / len(shown):.3f} ms per update, "
          f"{1e3 * t_frame / len(shown):.3f} ms per {args.width} x {args.height} frame (host variants, with their copies)")


if __name__ == "__main__":
    main()
