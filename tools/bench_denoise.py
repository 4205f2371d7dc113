"""Measures rtk_denoise_frame: what its kernels cost, launch by launch, and what the filter buys on a global-illumination frame.

  time     1920 x 1080, 5 iterations, with noise and albedo, on the synthetic planes of tests/denoise_model.py.  Every launch of a
           call -- k_denoise_prepare and k_denoise_atrous at steps 1, 2, 4, 8, 16 -- is timed alone with device events through the
           measurement probe (make denoise_probe: the launchers of csrc/denoise.hip, the path chosen per launch), the LDS-staged
           and the direct variant of a step alternating inside the repetition loop of one process.  From the medians the tool adds
           up what a call costs with RTK_DENOISE_LDS_MAX_STEP = 0, 1, 2, 4, 8, and beside every launch puts what one pass over its
           bytes (the packed records read once, 16 B written per pixel) would take at the 6.29 TB/s a device copy reaches.  The
           whole public call (rtk_denoise_frame_device, this process's knob) is timed the same way as a cross-check.
  quality  hw15/scene2 with GI at the size and depth of tools/bench_adaptive.py (1920 x 1920, depth 5, one diffuse ray): the
           RMSE against a 512-spp frame of an 8-spp frame, the same denoised, an adaptive render at threshold 0.04 denoised, and
           the plain 128-spp frame, each with its total time (render + g-buffer + filter).

    python tools/bench_denoise.py [--reps 15] [--warmup 3] [--skip-quality] [--out profiles/denoise_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simd-raytracer_amd")
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "hw15", "scene2.crtscene")
PROBE = os.path.join(ROOT, "tests", "cpp", "_build", "libdenoise_probe.so")
COPY_TBPS = 6.29          # measured device copy bandwidth of an MI355X
PASS = 16                 # samples per progressive pass of a plain frame
KNOBS = (0, 1, 2, 4, 8)


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def timed(torch, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def rmse(torch, a, b):
    return float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)).item())


def time_part(torch, rtk, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_model as dm

    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-C", PKG, "-s", "denoise_probe"])
    probe = C.CDLL(PROBE)
    vp = C.c_void_p
    probe.dn_probe_prepare.argtypes = [C.POINTER(rtk.DenoiseParams), C.c_int32, C.POINTER(rtk.DenoiseInputs), vp, vp]
    probe.dn_probe_atrous.argtypes = [C.POINTER(rtk.DenoiseParams), C.c_int32, vp, vp, vp, C.c_int, C.c_int, vp]
    w, h, its = args.width, args.height, 5
    cfg = rtk.DenoiseConfig(**dict(dm.PARAMS, iterations=its))
    p = cfg.to_c(w, h)
    planes = dm.synthetic(w, h)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        d = {k: torch.from_numpy(planes[k]).cuda() for k in ("rgb", "noise", "albedo", "normal", "position", "depth")}
        need = rtk.denoise_workspace_bytes(w, h, 1, cfg)
        ws = torch.zeros(need // 4, dtype=torch.float32, device="cuda")
        out = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        out_ref = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        inputs = rtk.DenoiseInputs(*(d[k].data_ptr() for k in ("rgb", "noise", "albedo", "normal", "position", "depth")))

        def ok(rc):
            if rc != 0:
                raise SystemExit(f"probe launch failed: hipError {rc}")

        def whole(o=out):
            rtk.denoise_device(w, h, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["position"].data_ptr(), d["depth"].data_ptr(),
                               o.data_ptr(), ws.data_ptr(), need, d_noise_ptr=d["noise"].data_ptr(), d_albedo_ptr=d["albedo"].data_ptr(),
                               cfg=cfg, stream=s)

        prepare = lambda: ok(probe.dn_probe_prepare(C.byref(p), 1, C.byref(inputs), ws.data_ptr(), s))
        atrous = lambda k, staged: (lambda: ok(probe.dn_probe_atrous(C.byref(p), 1, d["albedo"].data_ptr(), out.data_ptr(), ws.data_ptr(), k, staged, s)))
        # the probe's launches, every step staged where it can be, give the bits of the public call
        whole(out_ref)
        prepare()
        for k in range(its):
            atrous(k, 1 if (1 << k) <= 8 else 0)()
        stream.synchronize()
        assert torch.equal(out.view(torch.int32), out_ref.view(torch.int32)), "the probe's launches are not the call"
        # every launch alone.  An iteration's input is whatever the workspace holds from the launches before it: the weights'
        # values change, the work does not (no branch of the kernel depends on them).
        sides = {"prepare": prepare, "whole_call_this_process": whole}
        for k in range(its):
            sides[f"step{1 << k}_direct"] = atrous(k, 0)
            if (1 << k) <= 8:
                sides[f"step{1 << k}_staged"] = atrous(k, 1)
        times = {key: [] for key in sides}
        for i in range(args.warmup + args.reps):
            for key, call in sides.items():
                t = timed(torch, stream, call)
                if i >= args.warmup:
                    times[key].append(t)
    px = w * h
    floor_ms = lambda nbytes: round(nbytes / (COPY_TBPS * 1e12) * 1e3, 4)
    res = {"w": w, "h": h, "iterations": its, "planes": "synthetic, noise + albedo", "launches": {k: spread(t) for k, t in times.items()},
           # prepare reads 3 + 3 + 3 + 3 + 1 + 1 floats and writes three records; an iteration reads three records and writes one
           "copy_floor_ms": {"prepare": floor_ms(px * (14 * 4 + 48)), "iteration": floor_ms(px * 64), "last_iteration": floor_ms(px * (48 + 12 + 12))}}
    med = {k: statistics.median(t) for k, t in times.items()}
    totals = {}
    for knob in KNOBS:
        parts = ["prepare"] + [f"step{1 << k}_" + ("staged" if knob and (1 << k) <= knob else "direct") for k in range(its)]
        totals[str(knob)] = {"ms_sum_of_medians": round(sum(med[x] for x in parts), 4), "launches": parts}
    res["call_by_lds_max_step"] = totals
    res["fastest_lds_max_step"] = int(min(totals, key=lambda k: totals[k]["ms_sum_of_medians"]))
    res["lds_max_step_of_this_process"] = os.environ.get("RTK_DENOISE_LDS_MAX_STEP", "default")
    return res


def quality_part(torch, rtk, args):
    w = h = args.size
    n = w * h
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE))
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    dcfg = rtk.DenoiseConfig()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")
        d_ref, d_rgb, d_out, d_noise = f32(n * 3), f32(n * 3), f32(n * 3), f32(n)
        d_samples = torch.zeros(n, dtype=torch.int32, device="cuda")
        gb = {k: f32(n * c) for k, c in (("depth", 1), ("position", 3), ("normal", 3), ("albedo", 3))}
        need = rtk.denoise_workspace_bytes(w, h, 1, dcfg)
        ws = f32(need // 4)

        def frame(spp, out):
            cfgs = ([rtk.RenderConfig(spp=spp, **kw)] if spp <= PASS else
                    [rtk.RenderConfig(spp=spp, sample_begin=b, sample_count=min(PASS, spp - b), **kw) for b in range(0, spp, PASS)])
            for c in cfgs:
                acc.render_frame_device(c, out.data_ptr(), s)

        def adaptive(spp, mn, step, thr):
            acc.render_adaptive_device(rtk.RenderConfig(spp=spp, **kw), rtk.AdaptiveConfig(min_samples=mn, step=step, threshold=thr, floor=0.01),
                                       d_rgb.data_ptr(), d_samples.data_ptr(), d_noise.data_ptr(), s)

        def guides(spp):
            acc.render_gbuffer_device(rtk.RenderConfig(spp=spp, **kw), {k: t.data_ptr() for k, t in gb.items()}, sample=0, stream=s)

        def filt():
            rtk.denoise_device(w, h, d_rgb.data_ptr(), gb["normal"].data_ptr(), gb["position"].data_ptr(), gb["depth"].data_ptr(), d_out.data_ptr(),
                               ws.data_ptr(), need, d_noise_ptr=d_noise.data_ptr(), d_albedo_ptr=gb["albedo"].data_ptr(), cfg=dcfg, stream=s)

        frame(args.ref_spp, d_ref)
        stream.synchronize()
        rows = {}

        def measure(name, render, denoised, spp_for_guides=0):
            ts = {"render": [], "gbuffer": [], "denoise": []}
            for _ in range(args.quality_reps):
                ts["render"].append(timed(torch, stream, render))
                if denoised:
                    ts["gbuffer"].append(timed(torch, stream, lambda: guides(spp_for_guides)))
                    ts["denoise"].append(timed(torch, stream, filt))
            row = {"rmse_vs_ref": rmse(torch, d_out if denoised else d_rgb, d_ref), "ms": {k: spread(v) for k, v in ts.items() if v}}
            row["ms_total_of_medians"] = round(sum(statistics.median(v) for v in ts.values() if v), 3)
            if denoised:
                row["rmse_before_filter"] = rmse(torch, d_rgb, d_ref)
            rows[name] = row

        measure("plain_8spp", lambda: frame(8, d_rgb), False)
        # (an adaptive render with min_samples = spp is the 8-spp frame, bit for bit, and writes the noise plane the filter wants)
        measure("denoised_8spp", lambda: adaptive(8, 8, 1, 0.0), True, 8)
        measure("denoised_adaptive_0.04", lambda: adaptive(args.spp, 16, 16, 0.04), True, args.spp)
        rows["denoised_adaptive_0.04"]["mean_samples"] = round(float(d_samples.float().mean().item()), 3)
        measure(f"plain_{args.spp}spp", lambda: frame(args.spp, d_rgb), False)
    return {"scene": "hw15/scene2", "w": w, "h": h, "max_ray_depth": 5, "diffuse_rays": 1, "ref_spp": args.ref_spp, "reps": args.quality_reps,
            "denoise": dict(iterations=dcfg.iterations, normal_power_log2=dcfg.normal_power_log2, sigma_luminance=dcfg.sigma_luminance,
                            sigma_plane=dcfg.sigma_plane, albedo_floor=dcfg.albedo_floor), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--size", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--quality-reps", type=int, default=3)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_denoise needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    result = {"tool": "bench_denoise", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "timing": "device events around every launch, sides alternating in one process",
              "time": time_part(torch, rtk, args)}
    if not args.skip_quality:
        result["quality"] = quality_part(torch, rtk, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
