"""Times rtk_render_regions_device against what a caller had before it.

hw09/scene5 at 1920 x 1080 (BASELINE config 2), RTK_TRACE_AUTO, device buffers, one process, 3 warm-up + 15 timed repetitions, the
variants alternating inside the repetition loop, host wall time from the first call to the idle stream; medians of the timed
repetitions, and every single run kept ("runs"):
  a  one centred 480 x 270 rectangle (PACKED)
       region        one rtk_render_regions_device call, steady state (the same list every repetition)
       frame         the whole frame through rtk_render_frame_device
       radiance      the same pixels the way they could be rendered before: rtk_camera_rays_device for the whole frame, the
                     rectangle's rays sliced out, rtk_accel_radiance_device with the frame's pixel indices
     with the rectangle's rtk_render_last_critical_path and the frame's
  b  64 disjoint 64 x 64 rectangles (an 8 x 8 lattice over the frame, IN_FRAME)
       one_call      one rtk_render_regions_device call
       loop          64 calls of one rectangle each, on one accel
       frame         the whole frame
     `every_one_call_run_faster`: max of one_call < min of loop
  c  the whole frame as one rectangle against rtk_render_frame_device
The tool asserts that every variant renders the frame's bits before it reports a time.

--steady W H (with --pkg-root DIR to load another checkout's package, e.g. the parent commit's): steady
rtk_render_frame_device calls alone -- and, where the package has regions, the whole frame as one rectangle; prints one JSON line.
Run it in alternating processes to compare two commits.

    python tools/bench_regions.py [--reps 15] [--warmup 3] [--out profiles/regions_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join("tests", "golden", "scenes", "hw09", "scene5.crtscene")
W, H = 1920, 1080


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "runs": [round(t, 4) for t in ms]}


def wall(stream, call):
    t0 = time.perf_counter()
    call()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(stream, variants, args, check=None):
    times = {n: [] for n in variants}
    for i in range(args.warmup + args.reps):
        for n, f in variants.items():
            t = wall(stream, f)
            if i >= args.warmup:
                times[n].append(t)
        if check is not None:
            check()
    return times


def same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def measure(rtk, torch, stream, args):
    scene = rtk.parse_scene_file(os.path.join(ROOT, SCENE))
    cfg = rtk.RenderConfig(width=W, height=H)
    s = stream.cuda_stream
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    acc_f = rtk.KdTreeSimdAccel(scene)

    def full():
        acc_f.render_frame_device(cfg, frame.data_ptr(), s)

    res = {}
    # ---- a: one centred 480 x 270 rectangle
    x0, y0 = (W - 480) // 2, (H - 270) // 2
    R = (x0, y0, x0 + 480, y0 + 270)
    acc_a, acc_r = rtk.KdTreeSimdAccel(scene), rtk.KdTreeSimdAccel(scene)
    out_a = torch.empty((270, 480, 3), dtype=torch.float32, device="cuda")
    out_r = torch.empty((270 * 480, 3), dtype=torch.float32, device="cuda")
    rays = torch.empty((H, W, 6), dtype=torch.float32, device="cuda")
    ys, xs = np.mgrid[R[1]:R[3], R[0]:R[2]]
    ids = torch.from_numpy((ys * W + xs).reshape(-1).astype(np.uint32).view(np.int32)).cuda()
    rcfg = rtk.RadianceConfig()

    def region():
        acc_a.render_regions_device(cfg, [R], rtk.REGIONS_PACKED, out_a.data_ptr(), s)

    def radiance():
        acc_r.camera_rays_device(cfg, rays.data_ptr(), 0, s)
        cut = rays[R[1]:R[3], R[0]:R[2]].contiguous()
        acc_r.radiance_device(cut.data_ptr(), ids.data_ptr(), 270 * 480, out_r.data_ptr(), rcfg, s)
        radiance.keep = cut                                        # (alive until the stream is idle)

    def check_a():
        want = frame[R[1]:R[3], R[0]:R[2]]
        assert same_bits(torch, out_a, want), "the rectangle and the frame's crop differ"
        assert same_bits(torch, out_r.view(270, 480, 3), want), "the radiance batch and the frame's crop differ"

    t = timed(stream, {"region": region, "frame": full, "radiance": radiance}, args, check_a)
    region(); stream.synchronize()
    crit_region = acc_a.last_critical_path_ms()
    full(); stream.synchronize()
    crit_frame = acc_f.last_critical_path_ms()
    res["a_one_480x270_rectangle"] = {
        "rect": list(R), **{n: spread(v) for n, v in t.items()},
        "region_over_frame": round(statistics.median(t["region"]) / statistics.median(t["frame"]), 3),
        "radiance_over_region": round(statistics.median(t["radiance"]) / statistics.median(t["region"]), 3),
        "critical_path_ms": {"region": round(crit_region, 4), "frame": round(crit_frame, 4)}}

    # ---- b: 64 disjoint 64 x 64 rectangles
    rects = [(32 + 236 * i, 20 + 130 * j, 32 + 236 * i + 64, 20 + 130 * j + 64) for j in range(8) for i in range(8)]
    acc_b, acc_l = rtk.KdTreeSimdAccel(scene), rtk.KdTreeSimdAccel(scene)
    out_b = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    out_l = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    singles = [np.array([r], np.int32) for r in rects]
    all_rects = np.array(rects, np.int32)

    def one_call():
        acc_b.render_regions_device(cfg, all_rects, rtk.REGIONS_IN_FRAME, out_b.data_ptr(), s)

    def loop():
        for r in singles:
            acc_l.render_regions_device(cfg, r, rtk.REGIONS_IN_FRAME, out_l.data_ptr(), s)

    def check_b():
        assert same_bits(torch, out_b, out_l), "one call and the loop of calls differ"
        for r in (rects[0], rects[27], rects[63]):
            assert same_bits(torch, out_b[r[1]:r[3], r[0]:r[2]], frame[r[1]:r[3], r[0]:r[2]]), "a rectangle and the frame's crop differ"

    t = timed(stream, {"one_call": one_call, "loop": loop, "frame": full}, args, check_b)
    res["b_64_rectangles_of_64x64"] = {
        **{n: spread(v) for n, v in t.items()},
        "loop_over_one_call": round(statistics.median(t["loop"]) / statistics.median(t["one_call"]), 3),
        "one_call_over_frame": round(statistics.median(t["one_call"]) / statistics.median(t["frame"]), 3),
        "every_one_call_run_faster": max(t["one_call"]) < min(t["loop"])}

    # ---- c: the whole frame as one rectangle
    acc_c = rtk.KdTreeSimdAccel(scene)
    out_c = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    whole = np.array([(0, 0, W, H)], np.int32)

    def as_region():
        acc_c.render_regions_device(cfg, whole, rtk.REGIONS_IN_FRAME, out_c.data_ptr(), s)

    def check_c():
        assert same_bits(torch, out_c, frame), "the whole-frame rectangle and the frame differ"

    t = timed(stream, {"region": as_region, "frame": full}, args, check_c)
    res["c_whole_frame_as_one_rectangle"] = {
        **{n: spread(v) for n, v in t.items()},
        "region_over_frame": round(statistics.median(t["region"]) / statistics.median(t["frame"]), 3)}
    return res


def steady(rtk, torch, stream, args):
    w, h = args.steady
    scene = rtk.parse_scene_file(os.path.join(ROOT, SCENE))
    acc = rtk.KdTreeSimdAccel(scene)
    cfg = rtk.RenderConfig(width=w, height=h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    variants = {"frame": lambda: acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)}
    if hasattr(acc, "render_regions_device"):
        acc2 = rtk.KdTreeSimdAccel(scene)
        whole = np.array([(0, 0, w, h)], np.int32)
        variants["region"] = lambda: acc2.render_regions_device(cfg, whole, rtk.REGIONS_IN_FRAME, out.data_ptr(), stream.cuda_stream)
    t = timed(stream, variants, args)
    return {"tool": "bench_regions --steady", "w": w, "h": h, **{n: spread(v) for n, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--steady", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--pkg-root", default=ROOT)
    args = ap.parse_args()
    import torch

    sys.path.insert(0, args.pkg_root)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_regions needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        if args.steady:
            result = steady(rtk, torch, stream, args)
        else:
            import bench  # (code_hash: the hash bench.py stamps its results with)
            result = {"tool": "bench_regions", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "scene": "hw09/scene5", "frame": [W, H], "trace_mode": "auto"}
            result.update(measure(rtk, torch, stream, args))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
