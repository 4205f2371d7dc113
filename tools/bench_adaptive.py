"""Times rtk_render_adaptive_device on hw15/scene2 at BASELINE config 4's shape (1920 x 1920, 128 spp ceiling, depth 5, one diffuse
GI ray) and says what the samples it saves cost in error.

  (a) rtk_render_frame_device, RTK_TRACE_STREAM, 128 spp: the plain frame, in progressive passes of 16 samples as bench.py renders
      config 4 (one call for all 128 samples asks for queues of 32 samples per lane, which this frame size does not get).
  (b) rtk_render_adaptive_device with min_samples = spp = 128: the same samples through the adaptive path (one round, no decision
      that stops anything), so b / a is the overhead of the path -- per sample and chunk a camera-ray kernel, one radiance batch,
      a counter fold and an accumulate kernel, where the frame traces several samples per launch on four lanes.
  (c) adaptive at min 16, step 16 with each of --thresholds: the time, the mean sample count and its histogram, the RMSE against a
      512-spp rtk_render_frame, and beside it the RMSE of a plain frame whose spp is the nearest integer to that mean (and that
      frame's time): what the same number of samples buys when every pixel gets the same share.

Every side is warmed up, then the sides alternate inside the repetition loop of one process; every run is timed with device events
on the call's stream (the adaptive call blocks the host once per round; the events bracket all of it).  Before any time counts the
tool checks that (b) has the bits of (a).

    python tools/bench_adaptive.py [--reps 15] [--warmup 2] [--out profiles/adaptive_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "hw15", "scene2.crtscene")
PASS = 16          # samples per progressive pass of a plain frame


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def timed(torch, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def rmse(torch, a, b):
    return float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.08, 0.04, 0.02])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_adaptive needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    w = h = args.size
    n = w * h
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE))
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    cfg = rtk.RenderConfig(spp=args.spp, **kw)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        d_frame = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_ref = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_rgb = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_samples = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_noise = torch.zeros(n, dtype=torch.float32, device="cuda")

        def frame(spp, out=d_frame):
            if spp <= PASS:
                cfgs = [rtk.RenderConfig(spp=spp, **kw)]
            else:
                cfgs = [rtk.RenderConfig(spp=spp, sample_begin=b, sample_count=min(PASS, spp - b), **kw) for b in range(0, spp, PASS)]

            def run():
                for c in cfgs:
                    acc.render_frame_device(c, out.data_ptr(), s)
            return run

        def adaptive(mn, step, thr):
            ad = rtk.AdaptiveConfig(min_samples=mn, step=step, threshold=thr, floor=0.01)
            return lambda: acc.render_adaptive_device(cfg, ad, d_rgb.data_ptr(), d_samples.data_ptr(), d_noise.data_ptr(), s)

        # the reference everything is judged against, and the sample counts the thresholds give
        frame(args.ref_spp, d_ref)()
        stream.synchronize()
        sides = {"a_frame": frame(args.spp), "b_adaptive_all_samples": adaptive(args.spp, 1, 0.0)}
        picks = []
        for thr in args.thresholds:
            adaptive(16, 16, thr)()
            stream.synchronize()
            cn = acc.last_counters()
            counts = d_samples.cpu().numpy()
            mean = float(counts.mean())
            hist = {int(k): int(v) for k, v in zip(*np.unique(counts, return_counts=True))}
            nearest = max(1, int(round(mean)))
            pick = {"threshold": thr, "mean_samples": round(mean, 3), "samples_histogram_pixels": hist, "rays": cn["rays"],
                    "primary": cn["primary"], "rmse_vs_ref": rmse(torch, d_rgb, d_ref), "plain_spp": nearest}
            frame(nearest)()
            stream.synchronize()
            pick["plain_rmse_vs_ref"] = rmse(torch, d_frame, d_ref)
            picks.append(pick)
            sides[f"c_adaptive_{thr:g}"] = adaptive(16, 16, thr)
            sides[f"c_plain_{nearest}spp_for_{thr:g}"] = frame(nearest)
        # (b) is (a), bit for bit, before any time counts
        sides["a_frame"]()
        sides["b_adaptive_all_samples"]()
        stream.synchronize()
        assert torch.equal(d_frame.view(torch.int32), d_rgb.view(torch.int32)), "adaptive with min_samples = spp is not the frame"
        frame_rmse = rmse(torch, d_frame, d_ref)
        times = {key: [] for key in sides}
        for i in range(args.warmup + args.reps):
            for key, call in sides.items():
                t = timed(torch, stream, call)
                if i >= args.warmup:
                    times[key].append(t)
    result = {"tool": "bench_adaptive", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "timing": "device events on the call's stream", "scene": "hw15/scene2",
              "w": w, "h": h, "spp": args.spp, "max_ray_depth": 5, "diffuse_rays": 1, "ref_spp": args.ref_spp, "plain_frames": "progressive passes of %d samples" % PASS,
              "frame_rmse_vs_ref": frame_rmse, "times": {key: spread(t) for key, t in times.items()}, "adaptive": picks}
    a, b = result["times"]["a_frame"]["ms_median"], result["times"]["b_adaptive_all_samples"]["ms_median"]
    result["overhead_b_over_a"] = round(b / a, 3)
    result["every_b_run_slower_than_every_a_run"] = min(times["b_adaptive_all_samples"]) > max(times["a_frame"])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
