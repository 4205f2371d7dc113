"""Times the batched radiance query (rtk_accel_radiance_device) against the frame path that shares its pipeline.

Workload: hw09/scene5 (max_ray_depth 5) and hw11/scene8 (max_ray_depth 10) at 1920x1080, one sample (device buffers).
  frame_stream       rtk_render_frame_device with RTK_TRACE_STREAM: the streaming pipeline fed by its built-in camera (the baseline:
                     it does not come from the code under test).  Timed twice per repetition (frame_stream, frame_stream_again)
                     so that the run-to-run spread of the baseline itself is on record next to the ratios.
  radiance_raster    rtk_camera_rays_device once, outside the timed window, then rtk_accel_radiance_device on those rays
  radiance_shuffled  the same rays in a seeded random order (ids shuffled with them).  Level 0 is not sorted (the optional
                     binning pass over the caller's rays is not built); the figure is recorded so that a later change has one.
All are timed with device events after warm-up, alternating; the tool asserts that radiance_raster equals the frame, and
radiance_shuffled the frame's pixels in shuffled order, on every bit before it reports a time.  Prints one JSON line; --out also
writes it to a file (profiles/radiance_bench.json).

    python tools/bench_radiance.py [--reps 15] [--warmup 3] [--out profiles/radiance_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (code_hash: the hash bench.py stamps its results with)

SCENES = {"hw09/scene5": (os.path.join(ROOT, "tests", "golden", "scenes", "hw09", "scene5.crtscene"), 5),
          "hw11/scene8": (os.path.join(ROOT, "tests", "golden", "scenes", "hw11", "scene8.crtscene"), 10)}
WIDTH, HEIGHT = 1920, 1080


def timed(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    stream.synchronize()
    return a.elapsed_time(b)


def spread(ms, n):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "rays_per_s": round(n / (med * 1e-3))}


def measure(rtk, torch, acc, stream, depth, args):
    n = WIDTH * HEIGHT
    fcfg = rtk.RenderConfig(width=WIDTH, height=HEIGHT, max_ray_depth=depth, trace_mode=rtk.TRACE_STREAM)
    rcfg = rtk.RadianceConfig(max_ray_depth=depth, cull=True, trace_mode=rtk.TRACE_STREAM)
    cam = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    acc.camera_rays_device(fcfg, cam.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(11)).cuda()
    shuf = cam[perm].contiguous()
    shuf_ids = perm.to(torch.int32).contiguous()
    frame = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    raster = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    shuffled = torch.empty((n, 3), dtype=torch.float32, device="cuda")

    def f_frame():
        acc.render_frame_device(fcfg, frame.data_ptr(), stream.cuda_stream)

    def f_raster():
        acc.radiance_device(cam.data_ptr(), 0, n, raster.data_ptr(), rcfg, stream.cuda_stream)

    def f_shuffled():
        acc.radiance_device(shuf.data_ptr(), shuf_ids.data_ptr(), n, shuffled.data_ptr(), rcfg, stream.cuda_stream)

    def check():
        stream.synchronize()
        assert torch.equal(raster.view(torch.int32), frame.view(torch.int32)), "radiance_raster and the frame differ"
        assert torch.equal(shuffled.view(torch.int32), frame[perm].view(torch.int32)), "radiance_shuffled and the frame differ"

    f_frame(); f_raster(); f_shuffled()
    check()
    frame_rays = acc.last_counters()["rays"]
    for _ in range(args.warmup):
        f_frame(); f_raster(); f_shuffled()
    stream.synchronize()
    ms = {"frame_stream": [], "radiance_raster": [], "frame_stream_again": [], "radiance_shuffled": []}
    for _ in range(args.reps):                                                 # alternating: all see the same machine
        ms["frame_stream"].append(timed(torch, stream, f_frame))
        ms["radiance_raster"].append(timed(torch, stream, f_raster))
        ms["frame_stream_again"].append(timed(torch, stream, f_frame))
        ms["radiance_shuffled"].append(timed(torch, stream, f_shuffled))
    check()
    out = {k: spread(v, n) for k, v in ms.items()}
    base = out["frame_stream"]["ms_median"]
    out.update(rays=n, max_ray_depth=depth, frame_intersections=frame_rays, level0_sort="not built",
               raster_over_frame=round(out["radiance_raster"]["ms_median"] / base, 3),
               frame_again_over_frame=round(out["frame_stream_again"]["ms_median"] / base, 3),
               shuffled_over_frame=round(out["radiance_shuffled"]["ms_median"] / base, 3))
    return out


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
        raise SystemExit("bench_radiance needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    result = {"tool": "bench_radiance", "code_hash": bench.code_hash(), "width": WIDTH, "height": HEIGHT, "spp": 1,
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "scenes": {}}
    with torch.cuda.stream(stream):
        for name, (path, depth) in SCENES.items():
            acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
            result["scenes"][name] = measure(rtk, torch, acc, stream, depth, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
