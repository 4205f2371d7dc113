"""Measures rtk_temporal_accumulate_clamped: what its kernel costs beside the plain k_temporal_accumulate and beside a copy of the
bytes that must move, and what the clamp does to the accumulated frame where the history is wrong -- and where it is right.

  time     1920 x 1080 on the synthetic pair of tests/temporal_model.py (its camera move), noise and mesh planes, gamma = 1.  Sides,
           alternating inside the repetition loop of one process, every launch between device events: the plain call, the clamped
           call at radius 1, 2, 3, and a hipMemcpyAsync of the bytes the algorithm must move (those of tools/bench_temporal.py: the
           clamp needs no byte the plain call does not read).  The same sides without a history (prev = NULL): there the plain
           kernel passes the frame through and the clamped kernel stages its tiles, meets its two barriers and passes through, so
           the difference is the staging (the halo re-reads among it) and the barriers; what a radius adds with a history on top of
           what it adds without one is the box loop.
  quality  hw15/scene2 with GI at 1920 x 1920, depth 5, one diffuse ray, 16 frames of 8 spp, RMSE against 512 spp of the last
           frame's state, over the frame and over its hit pixels.  Four sequences, each rendered once and kept on the device, then
           replayed through the plain call and through every clamp setting of radius x gamma x history_keep, each with and without
           rtk_denoise_frame behind it: `orbit` (the orbit of tools/bench_temporal.py), `moved_mesh` (the sequence of
           tools/bench_motion.py, fed prev_position), `moved_light` (rtk_accel_set_lights moves every light along x each frame) and
           `static` (nothing changes: clamping can only lose averaging there).

    python tools/bench_temporal_clamp.py [--reps 15] [--warmup 3] [--skip-quality] [--out profiles/temporal_clamp_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_temporal import GUIDES, HISTORY_TAP, NEW_FRAME_READ, NEW_FRAME_WRITTEN, SCENE, hip_runtime, rmse, spread, timed  # noqa: E402

RADII, GAMMAS, KEEPS = (1, 2, 3), (0.5, 1.0, 1.5, 2.0, 3.0), (0.0, 0.5, 1.0)


def time_part(torch, rtk, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import temporal_clamp_model as cm
    import temporal_model as tm

    hip = hip_runtime()
    w, h = args.width, args.height
    px = w * h
    cfg = rtk.TemporalConfig(**tm.PARAMS)
    cur, prev = tm.synthetic_pair(w, h)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

        detail = tm.accumulate(cur, prev, detail=True, **tm.PARAMS)
        used = int(detail["used"].sum())
        nbytes = {"history": px * (NEW_FRAME_READ + NEW_FRAME_WRITTEN) + HISTORY_TAP * used, "no_history": px * (20 + NEW_FRAME_WRITTEN)}
        dc = {k: up(cur[k]) for k in ("rgb", "noise") + GUIDES}
        dq = {k: up(prev[k]) for k in ("rgb", "noise", "length") + GUIDES}
        out = {k: torch.zeros(px * m, dtype=torch.float32, device="cuda") for k, m in (("rgb", 3), ("noise", 1), ("length", 1))}
        cp, pp, op = ({k: t.data_ptr() for k, t in d.items()} for d in (dc, dq, out))
        pp["view"] = prev["view"]
        clamps = {r: rtk.ClampConfig(radius=r, gamma=args.gamma, history_keep=1.0) for r in RADII}
        calls = {}
        for side, q in (("history", pp), ("no_history", None)):
            # a copy moves its bytes once in and once out: half of them on each side
            src = torch.zeros(nbytes[side] // 2, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(nbytes[side] // 2, dtype=torch.uint8, device="cuda")
            calls[f"{side}_plain"] = (lambda q=q: rtk.temporal_accumulate_device(w, h, cp, q, op, cfg=cfg, stream=s))
            for r in RADII:
                calls[f"{side}_clamped_r{r}"] = (lambda q=q, r=r: rtk.temporal_accumulate_device(w, h, cp, q, op, cfg=cfg, stream=s, clamp=clamps[r]))
            calls[f"{side}_copy"] = (lambda src=src, dst=dst: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, s))
        # what is timed is what the model says (radius 1 and 3; the numpy box of 49 taps at this size takes its seconds)
        meta = {}
        for r in (1, 3):
            want = cm.accumulate(cur, prev, detail=True, radius=r, gamma=args.gamma, history_keep=1.0, **tm.PARAMS)
            calls[f"history_clamped_r{r}"]()
            stream.synchronize()
            for k in out:
                assert np.array_equal(out[k].cpu().numpy().view(np.uint32), tm.bits(want[k]).reshape(-1)), (r, k)
            meta[f"clamped_pixels_r{r}"] = int(want["clamped"].sum())
        times = {name: [] for name in calls}
        for i in range(args.warmup + args.reps):
            for name, call in calls.items():
                t = timed(torch, stream, call)
                if i >= args.warmup:
                    times[name].append(t)
    res = {"w": w, "h": h, "planes": "synthetic pair, noise + mesh", "gamma": args.gamma, "hit_pixels": int((cur["depth"] >= 0).sum()),
           "pixels_with_history": int(detail["blended"].sum()), **meta, "bytes_moved": nbytes, "sides": {}}
    for side in ("history", "no_history"):
        plain, copy = spread(times[f"{side}_plain"]), spread(times[f"{side}_copy"])
        row = {"plain": plain, "copy_of_the_bytes": copy, "plain_over_copy": round(plain["ms_median"] / copy["ms_median"], 3)}
        for r in RADII:
            k = spread(times[f"{side}_clamped_r{r}"])
            row[f"clamped_r{r}"] = dict(k, over_plain=round(k["ms_median"] / plain["ms_median"], 3), over_copy=round(k["ms_median"] / copy["ms_median"], 3),
                                        ms_over_plain=round(k["ms_median"] - plain["ms_median"], 4))
        res["sides"][side] = row
    # the attribution the two sides allow, in ms of the medians
    hist, none = res["sides"]["history"], res["sides"]["no_history"]
    res["attribution_ms"] = {f"r{r}": {"staging_and_barriers": none[f"clamped_r{r}"]["ms_over_plain"],
                                       "box_loop_and_blend": round(hist[f"clamped_r{r}"]["ms_over_plain"] - none[f"clamped_r{r}"]["ms_over_plain"], 4)}
                             for r in RADII}
    return res


def quality_part(torch, rtk, args):
    w = h = args.size
    n = w * h
    scene = rtk.parse_scene_file(SCENE)
    arrays = scene.arrays()
    acc = rtk.KdTreeSimdAccel(scene)
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    fov = rtk.RenderConfig(**kw).fov_degrees
    dcfg, tcfg, mcfg = rtk.DenoiseConfig(), rtk.TemporalConfig(fov_degrees=fov), rtk.MotionConfig(fov_degrees=fov)
    home = acc.camera()
    lights = acc.lights()
    frames_n, last = args.frames, args.frames - 1
    centre = np.array((0.0, 0.0, -3.0))
    arm = home[0].astype(np.float64) - centre

    def orbit_view(k):      # tools/bench_temporal.py: half a degree a frame, ending at the scene's own camera
        t = np.deg2rad(0.5 * (k - last))
        c, s_ = np.cos(t), np.sin(t)
        r = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
        return (centre + r @ arm).astype(np.float32), (home[1].reshape(3, 3).astype(np.float64) @ r.T).astype(np.float32).reshape(9)

    base = np.ascontiguousarray(arrays["vertices"], np.float32).reshape(-1, 3)
    starts = np.concatenate([[0], np.cumsum(arrays["mesh_nverts"])]).astype(np.int64)

    def pose(k):            # tools/bench_motion.py: one mesh translated a step a frame
        v = base.copy()
        v[starts[args.mesh]:starts[args.mesh + 1]] += np.float32(k) * np.array(args.step, np.float32)
        return torch.from_numpy(np.ascontiguousarray(v)).cuda()

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    result = {}
    with torch.cuda.stream(stream):
        f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")
        d_ref, d_out = f32(n * 3), f32(n * 3)
        hist = [{"rgb": f32(n * 3), "noise": f32(n), "length": f32(n)} for _ in (0, 1)]
        need = rtk.denoise_workspace_bytes(w, h, 1, dcfg)
        ws = f32(need // 4)
        shapes = (("depth", 1), ("position", 3), ("normal", 3), ("mesh", 1), ("albedo", 3), ("bary", 2), ("tri", 1))

        def record(k, view, fed_from=None):
            """frame k of a sequence, kept on the device: rgb, noise, the guides, and `fed`, the position the temporal call is handed"""
            f = {"rgb": f32(n * 3), "noise": f32(n), "view": view}
            f.update({x: f32(n * c) for x, c in shapes})
            acc.render_frame_noise_device(rtk.RenderConfig(spp=8, seed=100 + k, **kw), f["rgb"].data_ptr(), f["noise"].data_ptr(), s)
            acc.render_gbuffer_device(rtk.RenderConfig(spp=1, **kw), {x: f[x].data_ptr() for x, _ in shapes}, sample=0, stream=s)
            f["fed"] = f["position"]
            if fed_from is not None:
                f["fed"] = f32(n * 3)
                acc.render_motion_device(w, h, f["tri"].data_ptr(), f["bary"].data_ptr(), fed_from.data_ptr(), dict(prev_position=f["fed"].data_ptr()),
                                         cfg=mcfg, stream=s)
            if k != last:
                for x in ("albedo", "bary", "tri"):
                    del f[x]
            return f

        def reference():
            for b in range(0, args.ref_spp, 16):
                acc.render_frame_device(rtk.RenderConfig(spp=args.ref_spp, seed=0, sample_begin=b, sample_count=min(16, args.ref_spp - b), **kw),
                                        d_ref.data_ptr(), s)

        def replay(frames, clamp):
            for k, f in enumerate(frames):
                cur = dict(rgb=f["rgb"].data_ptr(), noise=f["noise"].data_ptr(), position=f["fed"].data_ptr(),
                           **{x: f[x].data_ptr() for x in ("normal", "depth", "mesh")})
                prev = None
                if k > 0:
                    q = frames[k - 1]
                    prev = dict({x: t.data_ptr() for x, t in hist[(k - 1) & 1].items()}, view=q["view"], **{x: q[x].data_ptr() for x in GUIDES})
                rtk.temporal_accumulate_device(w, h, cur, prev, {x: t.data_ptr() for x, t in hist[k & 1].items()}, cfg=tcfg, stream=s, clamp=clamp)
            return hist[(len(frames) - 1) & 1]

        def rows_of(frames):
            g = frames[-1]
            hit = g["depth"] >= 0
            hit3 = hit[:, None].expand(n, 3).reshape(-1)

            def row(rgb, **more):
                return dict(rmse=round(rmse(torch, rgb, d_ref), 5), rmse_hit=round(rmse(torch, rgb[hit3], d_ref[hit3]), 5), **more)

            def filt(rgb, noise):
                rtk.denoise_device(w, h, rgb.data_ptr(), g["normal"].data_ptr(), g["position"].data_ptr(), g["depth"].data_ptr(), d_out.data_ptr(),
                                   ws.data_ptr(), need, d_noise_ptr=noise.data_ptr(), d_albedo_ptr=g["albedo"].data_ptr(), cfg=dcfg, stream=s)
                return d_out

            def both(hs):
                return {"temporal": row(hs["rgb"], mean_history_length=round(float(hs["length"].mean().item()), 3)),
                        "temporal_denoised": row(filt(hs["rgb"], hs["noise"]))}

            out = {"hit_share": round(float(hit.float().mean().item()), 4), "last_frame_8spp": row(g["rgb"]),
                   "last_frame_8spp_denoised": row(filt(g["rgb"], g["noise"])), "unclamped": both(replay(frames, None)), "grid": []}
            for r in RADII:
                for gamma in GAMMAS:
                    for keep in KEEPS:
                        hs = replay(frames, rtk.ClampConfig(radius=r, gamma=gamma, history_keep=keep))
                        out["grid"].append(dict(radius=r, gamma=gamma, history_keep=keep, **both(hs)))
            for key in ("temporal", "temporal_denoised"):
                best = min(out["grid"], key=lambda e: e[key]["rmse"])
                out[f"best_{key}"] = dict(radius=best["radius"], gamma=best["gamma"], history_keep=best["history_keep"], rmse=best[key]["rmse"],
                                          unclamped_rmse=out["unclamped"][key]["rmse"])
            return out

        try:
            # orbit and static share the reference: the orbit ends at the scene's own camera
            frames = []
            for k in range(frames_n):
                acc.set_camera(*orbit_view(k))
                frames.append(record(k, orbit_view(k)))
            acc.set_camera(*home)
            reference()
            result["orbit"] = rows_of(frames)
            del frames
            frames = [record(k, home) for k in range(frames_n)]
            result["static"] = rows_of(frames)
            del frames
            # every light a step along x each frame
            frames = []
            for k in range(frames_n):
                acc.set_lights(lights[0] + np.float32(k) * np.array(args.light_step, np.float32), lights[1])
                frames.append(record(k, home))
            reference()
            result["moved_light"] = rows_of(frames)
            del frames
            acc.set_lights(*lights)
            # one mesh a step each frame, the history fetched where the surface point was (rtk_render_motion)
            poses = [pose(k) for k in range(frames_n)]
            frames = []
            for k in range(frames_n):
                if k > 0:
                    acc.update_vertices_device(poses[k].data_ptr(), s)
                frames.append(record(k, home, fed_from=poses[k - 1] if k > 0 else None))
            reference()
            result["moved_mesh"] = rows_of(frames)
            del frames
            stream.synchronize()
        finally:
            acc.set_camera(*home)
            acc.set_lights(*lights)
    return {"scene": "hw15/scene2", "w": w, "h": h, "max_ray_depth": 5, "diffuse_rays": 1, "spp": 8, "ref_spp": args.ref_spp, "frames": frames_n,
            "orbit_degrees_per_frame": 0.5, "moved_mesh": args.mesh, "mesh_step_per_frame": [float(x) for x in args.step],
            "light_step_per_frame": [float(x) for x in args.light_step],
            "temporal": dict(alpha_min=tcfg.alpha_min, plane_tolerance=tcfg.plane_tolerance, normal_min_dot=tcfg.normal_min_dot,
                             max_history=tcfg.max_history),
            "rmse_is": "against ref_spp of the last frame's state; rmse over the frame, rmse_hit over its hit pixels", "sequences": result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--gamma", type=float, default=1.0, help="of the timed clamp")
    ap.add_argument("--size", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--mesh", type=int, default=1, help="the mesh of hw15/scene2 that moves (1: the diffuse block on the left)")
    ap.add_argument("--step", type=float, nargs=3, default=(0.03, 0.0, 0.0), help="its translation per frame")
    ap.add_argument("--light-step", type=float, nargs=3, default=(0.05, 0.0, 0.0), help="the translation of every light per frame")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-time", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_temporal_clamp needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    result = {"tool": "bench_temporal_clamp", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "timing": "device events around every launch, sides alternating in one process"}
    if not args.skip_time:
        result["time"] = time_part(torch, rtk, args)
    if not args.skip_quality:
        result["quality"] = quality_part(torch, rtk, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
