"""Times rtk_accel_set_lights / rtk_accel_set_materials against the only route the C-ABI offered before them to the same pixels.

Per change, alternating between two states, on hw09/scene5 (4,014 triangles, 1920x1080) and on the height field of
tools/bench_update.py (199,712 triangles, 1280x720):
  live     the setter on one accel, then a frame into a device buffer: host wall time from the call until the stream is idle
  rebuild  rtk_scene_create + rtk_accel_build of the changed scene + rtk_accel_destroy of the old accel, then the new accel's
           first frame (which pays its upload), timed the same way
for (a) a light that moves, (b) a material that changes colour (the set of refractive materials stays), (c) a material that turns
refractive and back (the set changes: other kernels, a new engine trial).  Both paths run alternately in one process after
warm-up, and the tool asserts that they give the same frame before it reports a time.
On an RTK_TRAVERSAL_FAST accel of hw11/scene8: rtk_accel_set_materials alone, with a wall turning refractive and back, which
re-makes the opaque-only occlusion tree on the device each time (call until idle device).
Launch order after a light move (rtk.h): frames 1, 2, 3 on scene5 at 1920x1080 after rtk_accel_set_lights with the cost-feedback order
kept (the default for an unchanged count) and forgotten (rtk_accel_set_camera with the same camera forgets it).
Prints one JSON line; --out also writes it to a file (profiles/scene_state_bench.json).

    python tools/bench_scene_state.py [--reps 15] [--warmup 3] [--out profiles/scene_state_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (code_hash: the hash bench.py stamps its results with)
from bench_update import height_field_arrays, scene5_arrays, spread  # noqa: E402

SCENE8 = os.path.join(ROOT, "tests", "golden", "scenes", "hw11", "scene8.crtscene")
REFRACTIVE, DIFFUSE = 2, 0


def make_scene(rtk, a):
    return rtk.Scene.from_arrays(a["mesh_material"], a["mesh_nverts"], a["mesh_ntris"], a["vertices"], a["indices"], a["mat_kind"],
                                 a["mat_albedo"], a["mat_ior"], a["mat_smooth"], a["light_pos"], a["light_intensity"], a["cam_pos"],
                                 a["cam_mat"], a["background"], a["width"], a["height"], a["bucket_size"])


def variants(a):
    """name -> (two states of the scene's arrays, the setter that takes a live accel to a state)"""
    def changed(**kw):
        b = dict(a)
        b.update(kw)
        return b

    moved = a["light_pos"].copy()
    moved[0] += np.array([-2.0, 1.0, 1.5], np.float32)
    m = int(a["mesh_material"][-1])                                  # the big mesh's material
    albedo = a["mat_albedo"].copy()
    albedo[m] = [0.2, 0.7, 0.4]
    kind, ior = a["mat_kind"].copy(), a["mat_ior"].copy()
    kind[m], ior[m] = REFRACTIVE, 1.5

    def lights(acc, s):
        acc.set_lights(s["light_pos"], s["light_intensity"])

    def materials(acc, s):
        acc.set_materials(s["mat_kind"], s["mat_albedo"], s["mat_ior"], s["mat_smooth"])

    return {"set_lights": ([a, changed(light_pos=moved)], lights),
            "set_materials, same refractive set": ([a, changed(mat_albedo=albedo)], materials),
            "set_materials, refractive set changes": ([a, changed(mat_kind=kind, mat_ior=ior)], materials)}


def measure(rtk, torch, stream, a, args):
    cfg = rtk.RenderConfig(width=a["width"], height=a["height"])
    out_l = torch.empty((a["height"], a["width"], 3), dtype=torch.float32, device="cuda")
    out_r = torch.empty_like(out_l)

    def frame(acc, out):
        acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)
        stream.synchronize()

    res = {"frame": [a["width"], a["height"]], "triangles": int(a["mesh_ntris"].sum())}
    for name, (states, setter) in variants(a).items():
        live = rtk.KdTreeSimdAccel(make_scene(rtk, states[0]))
        holder = {"acc": rtk.KdTreeSimdAccel(make_scene(rtk, states[0]))}

        def go_live(k):
            t0 = time.perf_counter()
            setter(live, states[k])
            frame(live, out_l)
            return (time.perf_counter() - t0) * 1e3

        def go_rebuild(k):
            t0 = time.perf_counter()
            new = rtk.KdTreeSimdAccel(make_scene(rtk, states[k]))
            old, holder["acc"] = holder["acc"], new
            del old
            frame(new, out_r)
            return (time.perf_counter() - t0) * 1e3

        frame(live, out_l); frame(holder["acc"], out_r)
        lv, rb = [], []
        for i in range(args.warmup + args.reps):                     # alternating: both see the same machine
            k = (i + 1) % 2
            x, y = go_live(k), go_rebuild(k)
            assert torch.equal(out_l, out_r), f"{name}: the live and the rebuilt accel render different frames"
            if i >= args.warmup:
                lv.append(x); rb.append(y)
        steady = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            frame(live, out_l)
            steady.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"live_call_and_frame": spread(lv), "rebuild_and_first_frame": spread(rb), "steady_frame": spread(steady),
                     "rebuild_over_live_median": round(spread(rb)["ms_median"] / spread(lv)["ms_median"], 2),
                     "every_live_run_faster_than_every_rebuild": max(lv) < min(rb)}
    return res


def regather(rtk, torch, args):
    sc = rtk.parse_scene_file(SCENE8)
    acc = rtk.KdTreeSimdAccel(sc, traversal=rtk.TRAVERSAL_FAST)
    m = acc.materials()
    wall = int(sc.arrays()["mesh_material"][0])
    kinds = [m["kind"].copy(), m["kind"].copy()]
    kinds[1][wall] = REFRACTIVE
    acc.render_frame(rtk.RenderConfig(width=64, height=64))          # resident, with the tree of the build
    ms = []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc.set_materials(kinds[(i + 1) % 2], m["albedo"], m["ior"], m["smooth"])
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    ti = acc.tree_info()
    return {"scene": "hw11/scene8, RTK_TRAVERSAL_FAST", "leaf_refs": int(ti.n_leaf_refs), "leaves": int(ti.n_leaves),
            "set_materials_with_regather_call_until_idle": spread(ms)}


def order_after_light_move(rtk, torch, stream, a, args):
    cfg = rtk.RenderConfig(width=1920, height=1080)
    out = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
    pos = [a["light_pos"].copy(), a["light_pos"].copy()]
    pos[1][0] += np.array([-6.0, 3.0, 5.0], np.float32)
    res = {}
    for name in ("order kept", "order forgotten"):
        acc = rtk.KdTreeSimdAccel(make_scene(rtk, a))
        cam = acc.camera()

        def frame():
            t0 = time.perf_counter()
            acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3

        f = [[], [], []]
        for i in range(args.warmup + args.reps):
            for _ in range(20):                                      # the order of the state before the move is learnt and settled
                frame()
            acc.set_lights(pos[(i + 1) % 2], a["light_intensity"])
            if name == "order forgotten":
                acc.set_camera(*cam)
            t = [frame() for _ in range(3)]
            if i >= args.warmup:
                for j in range(3):
                    f[j].append(t[j])
        res[name] = {f"frame_{j + 1}": spread(f[j]) for j in range(3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_scene_state needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    result = {"tool": "bench_scene_state", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "scenes": {}}
    with torch.cuda.stream(stream):
        s5 = scene5_arrays(rtk)
        result["scenes"]["hw09/scene5"] = measure(rtk, torch, stream, s5, args)
        result["scenes"]["height field"] = measure(rtk, torch, stream, height_field_arrays(), args)
        result["regather"] = regather(rtk, torch, args)
        result["launch_order_after_set_lights"] = order_after_light_move(rtk, torch, stream, s5, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
