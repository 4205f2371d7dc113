"""Measures rtk_temporal_accumulate: what its kernel costs beside a copy of the bytes it must move, and what a history buys on an
orbit around a global-illumination scene.

  time     1920 x 1080 on the synthetic frames of tests/temporal_model.py, with the noise and the mesh planes.  Two sides: `static`
           (a frame accumulated onto a history of its own camera: every tap accepted) and `motion` (the synthetic pair's camera
           move).  Every launch of rtk_temporal_accumulate_device is timed with device events, the sides alternating inside the
           repetition loop of one process, and beside each a hipMemcpyAsync, timed the same way, of the bytes the algorithm must
           move: per pixel 56 B read and 20 B written for the new frame, and 20 B of history for every pixel of the history that
           some tap accepted (counted once; the numpy model says which).
  quality  hw15/scene2 with GI at the size and depth of tools/bench_denoise.py (1920 x 1920, depth 5, one diffuse ray): an orbit of
           16 frames at 8 spp, each accumulated onto the one before.  For the last camera the RMSE against a 512-spp frame of the
           plain 8-spp frame, the same denoised, the accumulated frame denoised (and not), and the plain 128-spp frame, each with
           the time of what a frame of that row costs; and, to tell the reprojection's error from the noise that is left, the same
           16 frames accumulated under the last camera standing still.

    python tools/bench_temporal.py [--reps 15] [--warmup 3] [--skip-quality] [--out profiles/temporal_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "hw15", "scene2.crtscene")
PASS = 16                 # samples per progressive pass of a plain frame
NEW_FRAME_READ, NEW_FRAME_WRITTEN, HISTORY_TAP = 56, 20, 20      # bytes per pixel: rgb noise position normal depth mesh; rgb noise length
GUIDES = ("depth", "position", "normal", "mesh")


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


def hip_runtime():
    """the HIP runtime this process already has (one per process: the package's note on torch)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        raise SystemExit("no HIP runtime is loaded")
    hip = C.CDLL(sorted(paths)[0])
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def time_part(torch, rtk, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import temporal_model as tm

    hip = hip_runtime()
    w, h = args.width, args.height
    px = w * h
    cfg = rtk.TemporalConfig(**tm.PARAMS)
    cur, prev = tm.synthetic_pair(w, h)
    # static: the previous frame again, seen from its own camera, onto its own history
    sides = {"static": (dict(prev, rgb=cur["rgb"], noise=cur["noise"]), prev), "motion": (cur, prev)}
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    res = {"w": w, "h": h, "planes": "synthetic pair, noise + mesh", "bytes_per_pixel": {"new_frame_read": NEW_FRAME_READ,
           "new_frame_written": NEW_FRAME_WRITTEN, "history_per_accepted_pixel": HISTORY_TAP}, "sides": {}}
    with torch.cuda.stream(stream):
        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

        calls, copies, meta = {}, {}, {}
        keep = []
        for name, (c, q) in sides.items():
            detail = tm.accumulate(c, q, detail=True, **tm.PARAMS)
            used = int(detail["used"].sum())
            nbytes = px * (NEW_FRAME_READ + NEW_FRAME_WRITTEN) + HISTORY_TAP * used
            dc = {k: up(c[k]) for k in ("rgb", "noise") + GUIDES}
            dq = {k: up(q[k]) for k in ("rgb", "noise", "length") + GUIDES}
            out = {k: torch.zeros(px * m, dtype=torch.float32, device="cuda") for k, m in (("rgb", 3), ("noise", 1), ("length", 1))}
            # a copy moves its bytes once in and once out: half of them on each side
            src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
            keep += [dc, dq, out, src, dst]
            cp, pp, op = ({k: t.data_ptr() for k, t in d.items()} for d in (dc, dq, out))
            pp["view"] = q["view"]
            calls[name] = (lambda cp=cp, pp=pp, op=op: rtk.temporal_accumulate_device(w, h, cp, pp, op, cfg=cfg, stream=s))
            copies[name] = (lambda src=src, dst=dst: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, s))
            calls[name]()
            stream.synchronize()
            for k in out:                                   # what is timed is what the model says
                assert np.array_equal(out[k].cpu().numpy().view(np.uint32), tm.bits(detail[k]).reshape(-1)), (name, k)
            hit = c["depth"] >= 0
            meta[name] = {"hit_pixels": int(hit.sum()), "pixels_with_history": int(detail["blended"].sum()),
                          "accepted_taps": int(detail["accepted"].sum()), "history_pixels_used": used, "bytes_moved": nbytes}
        times = {f"{n}_{kind}": [] for n in sides for kind in ("kernel", "copy")}
        for i in range(args.warmup + args.reps):
            for name in sides:
                for kind, call in (("kernel", calls[name]), ("copy", copies[name])):
                    t = timed(torch, stream, call)
                    if i >= args.warmup:
                        times[f"{name}_{kind}"].append(t)
    for name in sides:
        k, c = spread(times[f"{name}_kernel"]), spread(times[f"{name}_copy"])
        res["sides"][name] = dict(meta[name], kernel=k, copy_of_the_bytes=c, kernel_over_copy=round(k["ms_median"] / c["ms_median"], 3),
                                  kernel_gbps=round(meta[name]["bytes_moved"] / (k["ms_median"] * 1e-3) / 1e9, 1))
    return res


def quality_part(torch, rtk, args):
    w = h = args.size
    n = w * h
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE))
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    fov = rtk.RenderConfig(**kw).fov_degrees
    dcfg, tcfg = rtk.DenoiseConfig(), rtk.TemporalConfig(fov_degrees=fov)
    home = acc.camera()
    # the orbit: around the middle of the box, half a degree a frame, ending at the scene's own camera
    centre = np.array((0.0, 0.0, -3.0))
    arm = home[0].astype(np.float64) - centre

    def view(k):
        t = np.deg2rad(0.5 * (k - (args.frames - 1)))
        c, s_ = np.cos(t), np.sin(t)
        r = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
        # the rays are transpose(M) * dir: a camera turned by r has the matrix M * transpose(r)
        return (centre + r @ arm).astype(np.float32), (home[1].reshape(3, 3).astype(np.float64) @ r.T).astype(np.float32).reshape(9)

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")
        d_ref, d_rgb, d_noise, d_out = f32(n * 3), f32(n * 3), f32(n), f32(n * 3)
        shapes = (("depth", 1), ("position", 3), ("normal", 3), ("mesh", 1), ("albedo", 3))
        gb = [{k: f32(n * c) for k, c in shapes} for _ in (0, 1)]
        hist = [{"rgb": f32(n * 3), "noise": f32(n), "length": f32(n)} for _ in (0, 1)]
        need = rtk.denoise_workspace_bytes(w, h, 1, dcfg)
        ws = f32(need // 4)

        def frame(spp, out, seed=0):
            cfgs = ([rtk.RenderConfig(spp=spp, seed=seed, **kw)] if spp <= PASS else
                    [rtk.RenderConfig(spp=spp, seed=seed, sample_begin=b, sample_count=min(PASS, spp - b), **kw) for b in range(0, spp, PASS)])
            for c in cfgs:
                acc.render_frame_device(c, out.data_ptr(), s)

        def noisy(seed):
            acc.render_frame_noise_device(rtk.RenderConfig(spp=8, seed=seed, **kw), d_rgb.data_ptr(), d_noise.data_ptr(), s)

        def guides(g):      # through the pixel centres: spp = 1
            acc.render_gbuffer_device(rtk.RenderConfig(spp=1, **kw), {k: t.data_ptr() for k, t in g.items()}, sample=0, stream=s)

        def temporal(k):
            cur = dict(rgb=d_rgb.data_ptr(), noise=d_noise.data_ptr(), **{x: gb[k & 1][x].data_ptr() for x in GUIDES})
            prev = None
            if k > 0:
                prev = dict({x: t.data_ptr() for x, t in hist[(k - 1) & 1].items()}, view=view(k - 1),
                            **{x: gb[(k - 1) & 1][x].data_ptr() for x in GUIDES})
            rtk.temporal_accumulate_device(w, h, cur, prev, {x: t.data_ptr() for x, t in hist[k & 1].items()}, cfg=tcfg, stream=s)

        def filt(rgb, noise, g):
            rtk.denoise_device(w, h, rgb.data_ptr(), g["normal"].data_ptr(), g["position"].data_ptr(), g["depth"].data_ptr(), d_out.data_ptr(),
                               ws.data_ptr(), need, d_noise_ptr=noise.data_ptr(), d_albedo_ptr=g["albedo"].data_ptr(), cfg=dcfg, stream=s)

        last = args.frames - 1
        ts = {k: [] for k in ("render", "gbuffer", "temporal", "denoise")}
        try:
            for k in range(args.frames):
                acc.set_camera(*view(k))
                ts["render"].append(timed(torch, stream, lambda: noisy(100 + k)))
                ts["gbuffer"].append(timed(torch, stream, lambda: guides(gb[k & 1])))
                ts["temporal"].append(timed(torch, stream, lambda: temporal(k)))
            acc.set_camera(*view(last))
            frame(args.ref_spp, d_ref)
            stream.synchronize()
            g, hs = gb[last & 1], hist[last & 1]
            med = {k: statistics.median(v) for k, v in ts.items() if v}
            rows = {}
            rows["plain_8spp"] = {"rmse_vs_ref": rmse(torch, d_rgb, d_ref), "ms": round(med["render"], 3)}
            ts["denoise"] = [timed(torch, stream, lambda: filt(d_rgb, d_noise, g)) for _ in range(args.quality_reps)]
            med["denoise"] = statistics.median(ts["denoise"])
            rows["denoised_8spp"] = {"rmse_vs_ref": rmse(torch, d_out, d_ref), "ms": round(med["render"] + med["gbuffer"] + med["denoise"], 3)}
            rows["temporal_8spp"] = {"rmse_vs_ref": rmse(torch, hs["rgb"], d_ref), "ms": round(med["render"] + med["gbuffer"] + med["temporal"], 3),
                                     "mean_history_length": round(float(hs["length"].mean().item()), 3)}
            filt(hs["rgb"], hs["noise"], g)
            rows["temporal_denoised_8spp"] = {"rmse_vs_ref": rmse(torch, d_out, d_ref),
                                              "ms": round(med["render"] + med["gbuffer"] + med["temporal"] + med["denoise"], 3)}
            # the same count of frames without the motion: what of the gap to the reference is the reprojection's (view-dependent
            # light behind the moving camera, the repeated bilinear fetch) and what is the noise left after 16 x 8 samples
            for k in range(args.frames):
                noisy(200 + k)
                cur = dict(rgb=d_rgb.data_ptr(), noise=d_noise.data_ptr(), **{x: g[x].data_ptr() for x in GUIDES})
                prev = None if k == 0 else dict({x: t.data_ptr() for x, t in hist[(k - 1) & 1].items()}, view=view(last),
                                                **{x: g[x].data_ptr() for x in GUIDES})
                rtk.temporal_accumulate_device(w, h, cur, prev, {x: t.data_ptr() for x, t in hist[k & 1].items()}, cfg=tcfg, stream=s)
            hs = hist[last & 1]
            rows["temporal_8spp_static_camera"] = {"rmse_vs_ref": rmse(torch, hs["rgb"], d_ref), "mean_history_length": round(float(hs["length"].mean().item()), 3)}
            filt(hs["rgb"], hs["noise"], g)
            rows["temporal_denoised_8spp_static_camera"] = {"rmse_vs_ref": rmse(torch, d_out, d_ref)}
            rows["hit_share"] = round(float((g["depth"] >= 0).float().mean().item()), 4)
            t128 = [timed(torch, stream, lambda: frame(args.spp, d_rgb, seed=7)) for _ in range(args.quality_reps)]
            rows[f"plain_{args.spp}spp"] = {"rmse_vs_ref": rmse(torch, d_rgb, d_ref), "ms": round(statistics.median(t128), 3)}
        finally:
            acc.set_camera(*home)
    return {"scene": "hw15/scene2", "w": w, "h": h, "max_ray_depth": 5, "diffuse_rays": 1, "ref_spp": args.ref_spp, "frames": args.frames,
            "orbit_degrees_per_frame": 0.5, "ms_is": "medians over the orbit's frames of what one frame of the row costs",
            "ms_parts": {k: spread(v) for k, v in ts.items() if v},
            "temporal": dict(alpha_min=tcfg.alpha_min, plane_tolerance=tcfg.plane_tolerance, normal_min_dot=tcfg.normal_min_dot,
                             max_history=tcfg.max_history), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--size", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=16)
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
        raise SystemExit("bench_temporal needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    result = {"tool": "bench_temporal", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
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
