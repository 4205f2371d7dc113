"""Times rtk_render_gbuffer_device against the only other way to get such planes: per view rtk_accel_set_camera +
rtk_camera_rays_device + rtk_accel_intersect_device(cull = 1), all into preallocated device buffers (24 B of ray and 32 B of hit
per pixel; the caller would still have to split the hits into planes, which is not timed).  The albedo is outside the comparison:
the composite cannot produce it.

Shapes: hw09/scene5 as 1 view of 1920 x 1080, 16 views of 256 x 256 and 64 views of 128 x 128, and hw12/scene4 at 1920 x 1080.
Plane sets: all eight (60 B per pixel), depth only, depth + mesh.  The composite runs once with RTK_TRACE_AUTO and once with
RTK_TRACE_WAVE.  Every shape is warmed up first; then the sides alternate inside the repetition loop of one process and every
run is timed with device events on the call's stream.  The tool checks depth and mesh of the one call against the composite's
hits, bit for bit, before it reports a time.

`every_gbuffer_run_faster`: the slowest run of the one call is faster than the fastest run of the loop (against both trace
modes).  `gb_per_s`: bytes the call writes over its median time, beside the HBM peak of the MI355X (8 TB/s spec, about 6.3
achievable): information, not a claim.

    python tools/bench_gbuffer.py [--reps 15] [--warmup 3] [--out profiles/gbuffer_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SHAPES = [("hw09/scene5", 1920, 1080, 1), ("hw09/scene5", 256, 256, 16), ("hw09/scene5", 128, 128, 64), ("hw12/scene4", 1920, 1080, 1)]
PLANE_SETS = {"all": ("depth", "position", "normal", "albedo", "bary", "tri", "mesh", "material"), "depth": ("depth",),
              "depth_mesh": ("depth", "mesh")}
COMPS = dict(depth=1, position=3, normal=3, albedo=3, bary=2, tri=1, mesh=1, material=1)
HBM_PEAK_GB_S = 8000.0


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def timed(torch, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def measure_shape(rtk, torch, stream, shape, args):
    from bench_views import make_scene, orbit
    name, w, h, k = shape
    path = os.path.join(ROOT, "tests", "golden", "scenes", *name.split("/")) + ".crtscene"
    a = rtk.parse_scene_file(path).arrays()
    cams = np.stack([orbit(a, 360.0 * i / max(k, 4)) for i in range(k)])
    d_views = torch.from_numpy(cams).cuda()
    cfg = rtk.RenderConfig(width=w, height=h)
    acc_g = rtk.KdTreeSimdAccel(make_scene(rtk, a, cams[0]))
    acc_c = rtk.KdTreeSimdAccel(make_scene(rtk, a, cams[0]))
    n = w * h
    planes = {p: torch.empty(k * n * COMPS[p], dtype=torch.int32, device="cuda") for p in PLANE_SETS["all"]}
    d_rays = torch.empty(n * 6, dtype=torch.float32, device="cuda")
    d_hits = torch.empty(k * n * 8, dtype=torch.int32, device="cuda")
    s = stream.cuda_stream

    def gbuffer(names):
        return lambda: acc_g.render_gbuffer_device(cfg, {p: planes[p].data_ptr() for p in names}, 0, d_views.data_ptr(), k, s)

    def composite(mode):
        def run():
            for v in range(k):
                acc_c.set_camera(cams[v, :3], cams[v, 3:])
                acc_c.camera_rays_device(cfg, d_rays.data_ptr(), 0, s)
                acc_c.intersect_device(d_rays.data_ptr(), n, True, d_hits.data_ptr() + v * n * 32, mode, s)
        return run

    sides = {f"gbuffer_{key}": gbuffer(names) for key, names in PLANE_SETS.items()}
    sides["loop_auto"] = composite(rtk.TRACE_AUTO)
    sides["loop_wave"] = composite(rtk.TRACE_WAVE)
    times = {key: [] for key in sides}
    for i in range(args.warmup + args.reps):
        for key, call in sides.items():
            t = timed(torch, stream, call)
            if i >= args.warmup:
                times[key].append(t)
        if i == 0:          # the same answers on both sides, before any time counts
            hits = d_hits.view(k * n, 8)
            assert torch.equal(planes["depth"], hits[:, 0]) and torch.equal(planes["mesh"], hits[:, 4]) and torch.equal(planes["tri"], hits[:, 3]), \
                "the g-buffer call and the camera_rays + intersect loop disagree"
    res = {"scene": name, "w": w, "h": h, "k": k}
    for key, t in times.items():
        res[key] = spread(t)
    fastest_loop = min(min(times["loop_auto"]), min(times["loop_wave"]))
    for key, names in PLANE_SETS.items():
        g = res[f"gbuffer_{key}"]
        g["bytes_written"] = 4 * k * n * sum(COMPS[p] for p in names)
        g["gb_per_s"] = round(g["bytes_written"] / (g["ms_median"] * 1e-3) / 1e9, 1)
        g["fraction_of_hbm_peak"] = round(g["gb_per_s"] / HBM_PEAK_GB_S, 4)
        g["every_gbuffer_run_faster"] = max(times[f"gbuffer_{key}"]) < fastest_loop
    res["loop_bytes_written"] = k * n * (24 + 32)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_gbuffer needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        result = {"tool": "bench_gbuffer", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
                  "device": torch.cuda.get_device_name(0), "timing": "device events on the call's stream", "hbm_peak_gb_per_s": HBM_PEAK_GB_S,
                  "shapes": [measure_shape(rtk, torch, stream, s, args) for s in SHAPES]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
