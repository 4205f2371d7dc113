"""Measures rtk_render_frame_noise: what the noise plane costs beside a streamed frame, and against the call it replaces.

  sides    hw15/scene2 at 1920 x 1920, depth 5, one diffuse ray, 8 spp and 128 spp.  Three ways to the same pixels alternate inside
           the repetition loop of one process, each timed with device events on one stream:
             (a) frame      rtk_render_frame_device(RTK_TRACE_STREAM): rgb only
             (b) noise      rtk_render_frame_noise_device: rgb + noise (its host read-back of the overflow word lies inside the events)
             (c) adaptive   rtk_render_adaptive_device(min_samples = spp): rgb + noise, the only door before this call
           Medians of --reps after --warmup, min and max beside them, (b) - (a), and whether EVERY run of (b) beat EVERY run of (c).
  chain    (b) -> rtk_render_gbuffer_device -> rtk_denoise_frame_device at 8 spp, end to end in one pair of events, next to the same
           chain with (c) in front (the "denoised_8spp" row of tools/bench_denoise.py).

    python tools/bench_frame_noise.py [--reps 15] [--warmup 3] [--size 1920] [--out profiles/frame_noise_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "hw15", "scene2.crtscene")
PASS = 16                 # samples per progressive pass of a plain frame, as in tools/bench_denoise.py


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def timed(torch, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1920)
    ap.add_argument("--spp", type=int, nargs="+", default=[8, 128])
    ap.add_argument("--chain-spp", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_frame_noise needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    w = h = args.size
    n = w * h
    scene = rtk.parse_scene_file(SCENE)

    def make_accel(spp):
        # One call of more than PASS samples is planned with RTK_STREAM_BATCH = PASS / 4: four lanes of four samples, the queues of a
        # 16-sample pass (63 GB at this size), for the frame and for the new call alike.  The default plan would split the whole pass
        # over the lanes and ask for the full RTK_STREAM_MEM_GB budget (96 GB), which a shared device may not have.
        knob = {"RTK_STREAM_BATCH": str(PASS // 4)} if spp > PASS and "RTK_STREAM_BATCH" not in os.environ else {}
        os.environ.update(knob)                      # (the knobs are read when an accel is built)
        try:
            return rtk.KdTreeSimdAccel(scene), knob
        finally:
            for k in knob:
                del os.environ[k]

    acc, _ = make_accel(args.chain_spp)
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    dcfg = rtk.DenoiseConfig()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    result = {"tool": "bench_frame_noise", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "scene": "hw15/scene2", "w": w, "h": h, "max_ray_depth": 5, "diffuse_rays": 1,
              "timing": "device events around every call, sides alternating in one process", "spp": {}}
    with torch.cuda.stream(stream):
        f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")
        d_frame, d_rgb, d_argb, d_out, d_noise, d_anoise = f32(n * 3), f32(n * 3), f32(n * 3), f32(n * 3), f32(n), f32(n)
        gb = {k: f32(n * c) for k, c in (("depth", 1), ("position", 3), ("normal", 3), ("albedo", 3))}
        need = rtk.denoise_workspace_bytes(w, h, 1, dcfg)
        ws = f32(need // 4)

        def frame(spp):
            # (a frame of more than PASS samples in progressive passes, as tools/bench_denoise.py renders it)
            cfgs = ([rtk.RenderConfig(spp=spp, **kw)] if spp <= PASS else
                    [rtk.RenderConfig(spp=spp, sample_begin=b, sample_count=min(PASS, spp - b), **kw) for b in range(0, spp, PASS)])
            for c in cfgs:
                acc.render_frame_device(c, d_frame.data_ptr(), s)

        def frame_one_call(spp):
            acc.render_frame_device(rtk.RenderConfig(spp=spp, **kw), d_frame.data_ptr(), s)

        def noise(spp):
            acc.render_frame_noise_device(rtk.RenderConfig(spp=spp, **kw), d_rgb.data_ptr(), d_noise.data_ptr(), s)

        def adaptive(spp):
            acc.render_adaptive_device(rtk.RenderConfig(spp=spp, **kw), rtk.AdaptiveConfig(min_samples=spp, step=1, threshold=0.0, floor=1.0),
                                       d_argb.data_ptr(), 0, d_anoise.data_ptr(), s)

        def guides(spp):
            acc.render_gbuffer_device(rtk.RenderConfig(spp=spp, **kw), {k: t.data_ptr() for k, t in gb.items()}, sample=0, stream=s)

        def filt(rgb, nz):
            rtk.denoise_device(w, h, rgb.data_ptr(), gb["normal"].data_ptr(), gb["position"].data_ptr(), gb["depth"].data_ptr(), d_out.data_ptr(),
                               ws.data_ptr(), need, d_noise_ptr=nz.data_ptr(), d_albedo_ptr=gb["albedo"].data_ptr(), cfg=dcfg, stream=s)

        spp = args.chain_spp
        chains = {"b_noise_gbuffer_denoise": lambda: (noise(spp), guides(spp), filt(d_rgb, d_noise)),
                  "c_adaptive_gbuffer_denoise": lambda: (adaptive(spp), guides(spp), filt(d_argb, d_anoise)),
                  "a_plain_frame": lambda: frame_one_call(spp)}
        times = {k: [] for k in chains}
        for i in range(args.warmup + args.reps):
            for key, call in chains.items():
                t = timed(torch, stream, call)
                if i >= args.warmup:
                    times[key].append(t)
        result["chain"] = {"spp": spp, "denoise": dict(iterations=dcfg.iterations), "ms": {k: spread(v) for k, v in times.items()}}
        del acc

        for spp in args.spp:
            acc, knobs = make_accel(spp)
            sides = {"a_frame_stream_one_call": lambda: frame_one_call(spp), "b_frame_noise": lambda: noise(spp),
                     "c_adaptive_min_eq_spp": lambda: adaptive(spp)}
            if spp > PASS:
                sides["a_frame_stream_passes_of_16"] = lambda: frame(spp)
            times = {k: [] for k in sides}
            try:
                for i in range(args.warmup + args.reps):
                    for key, call in sides.items():
                        t = timed(torch, stream, call)
                        if i >= args.warmup:
                            times[key].append(t)
                stream.synchronize()
            except rtk.RtkError as e:                # (a device without room for the queues: say so and go on)
                result["spp"][str(spp)] = {"knobs": knobs, "error": str(e)}
                del acc
                continue
            row = {k: spread(v) for k, v in times.items()}
            row["knobs"] = knobs
            same_rgb = bool(torch.equal(d_rgb.view(torch.int32), d_frame.view(torch.int32)) and torch.equal(d_rgb.view(torch.int32), d_argb.view(torch.int32)))
            same_noise = bool(torch.equal(d_noise.view(torch.int32), d_anoise.view(torch.int32)))
            row["b_minus_a_ms_of_medians"] = round(statistics.median(times["b_frame_noise"]) - statistics.median(times["a_frame_stream_one_call"]), 4)
            row["c_over_b_of_medians"] = round(statistics.median(times["c_adaptive_min_eq_spp"]) / statistics.median(times["b_frame_noise"]), 3)
            row["every_b_faster_than_every_c"] = bool(max(times["b_frame_noise"]) < min(times["c_adaptive_min_eq_spp"]))
            row["rgb_bits_equal_a_b_c"] = same_rgb
            row["noise_bits_equal_b_c"] = same_noise
            row["noise_fallbacks"] = acc.noise_fallbacks()
            result["spp"][str(spp)] = row
            del acc

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
