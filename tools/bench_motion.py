"""Measures rtk_render_motion: what its kernel costs beside a copy of the bytes it must move, and what prev_position buys the
temporal step when a mesh moves.

  time     1920 x 1080 on hw09/scene5 and on the 199,712-triangle height field of tools/bench_update.py: the g-buffer of the scene's
           own camera (tri, bary) and, as the previous pose, the second pose of bench_update.  Every launch of
           rtk_render_motion_device -- prev_position alone, and with motion -- is timed with device events, the cases alternating
           inside the repetition loop of one process, and beside each a hipMemcpyAsync, timed the same way, of the bytes the
           algorithm must move: per pixel 12 B read (tri, bary) and 12 B (+ 8 B) written, plus 12 B of vertex ids and 36 B of
           vertices for every DISTINCT triangle that is hit.  What is timed is first compared with the numpy model.
  quality  hw15/scene2 with GI (1920 x 1920, depth 5, one diffuse ray): 16 frames at 8 spp under the standing camera, one mesh
           translated a little every frame through rtk_accel_update_vertices.  For the last pose the RMSE against a 512-spp frame of
           the plain 8-spp frame, temporal fed the g-buffer's position, temporal fed prev_position, and each of the three denoised.

    python tools/bench_motion.py [--reps 15] [--warmup 3] [--skip-quality] [--variant NAME] [--out profiles/motion_bench.json]
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
SCENE2 = os.path.join(ROOT, "tests", "golden", "scenes", "hw15", "scene2.crtscene")
PIXEL_READ, POSITION_WRITTEN, MOTION_WRITTEN, PER_TRIANGLE = 12, 12, 8, 48
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


def global_indices(a):
    starts = np.concatenate([[0], np.cumsum(a["mesh_nverts"])[:-1]]).astype(np.int64)
    tri_mesh = np.repeat(np.arange(len(a["mesh_ntris"])), a["mesh_ntris"])
    return np.asarray(a["indices"], np.int64).reshape(-1, 3) + starts[tri_mesh][:, None]


def time_part(torch, rtk, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_update as bu
    import motion_model as mm

    hip = hip_runtime()
    w, h = args.width, args.height
    px = w * h
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    res = {"w": w, "h": h, "bytes": {"per_pixel_read": PIXEL_READ, "prev_position_written": POSITION_WRITTEN, "motion_written": MOTION_WRITTEN,
                                     "per_distinct_triangle": PER_TRIANGLE}, "scenes": {}}
    with torch.cuda.stream(stream):
        for name, a in (("scene5", bu.scene5_arrays(rtk)), ("height field", bu.height_field_arrays())):
            pose = bu.poses(a)
            acc = rtk.KdTreeSimdAccel(bu.make_scene(rtk, a, pose[0]))
            cfg = rtk.RenderConfig(width=w, height=h, spp=1)
            mcfg = rtk.MotionConfig(fov_degrees=cfg.fov_degrees)
            view = acc.camera()
            d_tri = torch.zeros(px, dtype=torch.int32, device="cuda")
            d_bary = torch.zeros(px * 2, dtype=torch.float32, device="cuda")
            acc.render_gbuffer_device(cfg, dict(tri=d_tri.data_ptr(), bary=d_bary.data_ptr()), sample=0, stream=s)
            d_prev = torch.from_numpy(pose[1]).cuda()
            d_pos = torch.zeros(px * 3, dtype=torch.float32, device="cuda")
            d_mot = torch.zeros(px * 2, dtype=torch.float32, device="cuda")
            stream.synchronize()
            tri = d_tri.cpu().numpy().view(np.uint32).reshape(h, w)
            bary = d_bary.cpu().numpy().reshape(h, w, 2)
            index = global_indices(a)
            hit = tri < index.shape[0]
            distinct = int(np.unique(tri[hit]).size)
            # the share of full waves (4 rows of 16 pixels of a tile) whose 64 lanes carry one id
            th, tw = h // 16 * 16, w // 16 * 16
            waves = tri[:th, :tw].reshape(th // 16, 4, 4, tw // 16, 16).transpose(0, 1, 3, 2, 4).reshape(-1, 64)
            uniform = float((waves == waves[:, :1]).all(axis=1).mean())
            cases = {"prev_position": dict(prev_position=d_pos.data_ptr()),
                     "prev_position+motion": dict(prev_position=d_pos.data_ptr(), motion=d_mot.data_ptr())}
            calls, copies, nbytes = {}, {}, {}
            keep = []
            for case, outs in cases.items():
                nbytes[case] = px * (PIXEL_READ + POSITION_WRITTEN + (MOTION_WRITTEN if "motion" in outs else 0)) + PER_TRIANGLE * distinct
                src = torch.zeros(nbytes[case] // 2, dtype=torch.uint8, device="cuda")       # (a copy moves its bytes once in and once out)
                dst = torch.zeros(nbytes[case] // 2, dtype=torch.uint8, device="cuda")
                keep += [src, dst]
                calls[case] = (lambda outs=outs: acc.render_motion_device(w, h, d_tri.data_ptr(), d_bary.data_ptr(), d_prev.data_ptr(), outs,
                                                                          prev_view=view if "motion" in outs else None, cfg=mcfg, stream=s))
                copies[case] = (lambda src=src, dst=dst: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, s))
                calls[case]()
            stream.synchronize()
            want = mm.render_motion(tri, bary, index, pose[1], view, cfg.fov_degrees)       # what is timed is what the model says
            mm.assert_same(dict(prev_position=d_pos.cpu().numpy().reshape(h, w, 3), motion=d_mot.cpu().numpy().reshape(h, w, 2)), want, what=name)
            times = {f"{c}_{kind}": [] for c in cases for kind in ("kernel", "copy")}
            for i in range(args.warmup + args.reps):
                for case in cases:
                    for kind, call in (("kernel", calls[case]), ("copy", copies[case])):
                        t = timed(torch, stream, call)
                        if i >= args.warmup:
                            times[f"{case}_{kind}"].append(t)
            row = {"triangles": int(index.shape[0]), "vertices": int(pose[1].shape[0]), "hit_share": round(float(hit.mean()), 4),
                   "distinct_triangles_hit": distinct, "full_waves_with_one_id": round(uniform, 4), "cases": {}}
            for case in cases:
                k, c = spread(times[f"{case}_kernel"]), spread(times[f"{case}_copy"])
                row["cases"][case] = {"bytes_moved": nbytes[case], "kernel": k, "copy_of_the_bytes": c,
                                      "kernel_over_copy": round(k["ms_median"] / c["ms_median"], 3),
                                      "kernel_gbps": round(nbytes[case] / (k["ms_median"] * 1e-3) / 1e9, 1)}
            res["scenes"][name] = row
            del acc
    return res


def quality_part(torch, rtk, args):
    w = h = args.size
    n = w * h
    scene = rtk.parse_scene_file(SCENE2)
    arrays = scene.arrays()
    acc = rtk.KdTreeSimdAccel(scene)
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    fov = rtk.RenderConfig(**kw).fov_degrees
    dcfg, tcfg, mcfg = rtk.DenoiseConfig(), rtk.TemporalConfig(fov_degrees=fov), rtk.MotionConfig(fov_degrees=fov)
    view = acc.camera()
    base = np.ascontiguousarray(arrays["vertices"], np.float32).reshape(-1, 3)
    starts = np.concatenate([[0], np.cumsum(arrays["mesh_nverts"])]).astype(np.int64)
    step = np.array(args.step, np.float32)

    def pose(k):
        v = base.copy()
        v[starts[args.mesh]:starts[args.mesh + 1]] += np.float32(k) * step
        return torch.from_numpy(np.ascontiguousarray(v)).cuda()

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")
        d_ref, d_rgb, d_noise, d_out, d_back = f32(n * 3), f32(n * 3), f32(n), f32(n * 3), f32(n * 3)
        shapes = (("depth", 1), ("position", 3), ("normal", 3), ("mesh", 1), ("albedo", 3), ("bary", 2), ("tri", 1))
        gb = [{k: f32(n * c) for k, c in shapes} for _ in (0, 1)]
        # two histories side by side: fed the g-buffer's position, and fed prev_position
        hist = {feed: [{"rgb": f32(n * 3), "noise": f32(n), "length": f32(n)} for _ in (0, 1)] for feed in ("position", "prev_position")}
        need = rtk.denoise_workspace_bytes(w, h, 1, dcfg)
        ws = f32(need // 4)
        poses = [pose(k) for k in range(args.frames)]

        def temporal(k, feed):
            g = gb[k & 1]
            position = d_back if feed == "prev_position" and k > 0 else g["position"]
            cur = dict(rgb=d_rgb.data_ptr(), noise=d_noise.data_ptr(), position=position.data_ptr(),
                       **{x: g[x].data_ptr() for x in ("normal", "depth", "mesh")})
            prev = None
            if k > 0:
                prev = dict({x: t.data_ptr() for x, t in hist[feed][(k - 1) & 1].items()}, view=view,
                            **{x: gb[(k - 1) & 1][x].data_ptr() for x in GUIDES})
            rtk.temporal_accumulate_device(w, h, cur, prev, {x: t.data_ptr() for x, t in hist[feed][k & 1].items()}, cfg=tcfg, stream=s)

        def filt(rgb, noise, g):
            rtk.denoise_device(w, h, rgb.data_ptr(), g["normal"].data_ptr(), g["position"].data_ptr(), g["depth"].data_ptr(), d_out.data_ptr(),
                               ws.data_ptr(), need, d_noise_ptr=noise.data_ptr(), d_albedo_ptr=g["albedo"].data_ptr(), cfg=dcfg, stream=s)

        ts = {k: [] for k in ("update", "render", "gbuffer", "motion", "temporal")}
        for k in range(args.frames):
            if k > 0:
                ts["update"].append(timed(torch, stream, lambda: acc.update_vertices_device(poses[k].data_ptr(), s)))
            ts["render"].append(timed(torch, stream, lambda: acc.render_frame_noise_device(rtk.RenderConfig(spp=8, seed=100 + k, **kw),
                                                                                           d_rgb.data_ptr(), d_noise.data_ptr(), s)))
            g = gb[k & 1]
            ts["gbuffer"].append(timed(torch, stream, lambda: acc.render_gbuffer_device(rtk.RenderConfig(spp=1, **kw),
                                                                                        {x: t.data_ptr() for x, t in g.items()}, sample=0, stream=s)))
            if k > 0:
                ts["motion"].append(timed(torch, stream, lambda: acc.render_motion_device(w, h, g["tri"].data_ptr(), g["bary"].data_ptr(),
                                                                                          poses[k - 1].data_ptr(), dict(prev_position=d_back.data_ptr()),
                                                                                          cfg=mcfg, stream=s)))
            ts["temporal"].append(timed(torch, stream, lambda: temporal(k, "prev_position")))
            temporal(k, "position")
        last = args.frames - 1
        g = gb[last & 1]
        # the reference: 512 spp of the last pose, in passes of 16
        for b in range(0, args.ref_spp, 16):
            acc.render_frame_device(rtk.RenderConfig(spp=args.ref_spp, seed=0, sample_begin=b, sample_count=min(16, args.ref_spp - b), **kw),
                                    d_ref.data_ptr(), s)
        stream.synchronize()
        on = g["mesh"].view(torch.int32) == args.mesh                                       # the moved mesh's pixels of the last frame
        rows = {"pixels_on_the_moved_mesh": int(on.sum().item()), "hit_share": round(float((g["depth"] >= 0).float().mean().item()), 4)}

        def row(rgb, **more):
            on3 = on[:, None].expand(n, 3).reshape(-1)
            return dict(rmse_vs_ref=rmse(torch, rgb, d_ref), rmse_on_the_moved_mesh=rmse(torch, rgb[on3], d_ref[on3]), **more)

        def mean_length(hs):
            return {"mean_history_length": round(float(hs["length"].mean().item()), 3),
                    "mean_history_length_on_the_moved_mesh": round(float(hs["length"][on].mean().item()), 3)}

        rows["plain_8spp"] = row(d_rgb)
        filt(d_rgb, d_noise, g)
        rows["plain_8spp_denoised"] = row(d_out)
        for feed in ("position", "prev_position"):
            hs = hist[feed][last & 1]
            rows[f"temporal_fed_{feed}"] = row(hs["rgb"], **mean_length(hs))
            filt(hs["rgb"], hs["noise"], g)
            rows[f"temporal_fed_{feed}_denoised"] = row(d_out)
        stream.synchronize()
    return {"scene": "hw15/scene2", "w": w, "h": h, "max_ray_depth": 5, "diffuse_rays": 1, "spp": 8, "ref_spp": args.ref_spp, "frames": args.frames,
            "moved_mesh": args.mesh, "step_per_frame": [float(x) for x in step], "ms_parts": {k: spread(v) for k, v in ts.items() if v},
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
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--mesh", type=int, default=1, help="the mesh of hw15/scene2 that moves (1: the diffuse block on the left)")
    ap.add_argument("--step", type=float, nargs=3, default=(0.03, 0.0, 0.0), help="its translation per frame")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--variant", default="", help="a name for the build that is measured (RTK_LIB_OVERRIDE), stamped into the result")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_motion needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    result = {"tool": "bench_motion", "code_hash": bench.code_hash(), "variant": args.variant or "default", "library": os.path.relpath(rtk.lib_path(), ROOT),
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "timing": "device events around every launch, cases alternating in one process", "time": time_part(torch, rtk, args)}
    if not args.skip_quality:
        result["quality"] = quality_part(torch, rtk, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
