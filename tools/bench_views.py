"""Times rtk_render_views_device against the loop it replaces, and the first frame after a camera move.

Per scene (hw09/scene5, hw11/scene8), trace mode and shape -- K orbit cameras at w x h, K in {1, 4, 16, 64} at 128 x 128 and
256 x 256, K in {1, 4, 16} at 1920 x 1080 -- into device buffers, one process, 3 warm-up + 15 timed repetitions, the variants
alternating inside the repetition loop, host wall time from the first call to the idle stream:
  views    (a) one rtk_render_views_device call
  loop     (b) K x (rtk_accel_set_camera + rtk_render_frame_device) on the same accel
  rebuild  (c) K = 1 only: rtk_scene_create + rtk_accel_build + first frame + destroy, what a caller without set_camera does
The tool asserts (a) == (b) bit for bit before it reports a time.  `every_views_run_faster`: max of (a) < min of (b).

Camera move: at 1920 x 1080 on scene5, the first and the third frame after a 5 degree orbit step, with the launch order reset
(the default: the first-frame prior again) and with the previous camera's order kept (RTK_CAMERA_KEEPS_ORDER=1), two accels
alternating.  Behind the timed frames of a step 17 more are rendered untimed (RTK_COST_RESORT_EVERY is 16), so that at the next
step the kept order is that of the camera one step back, not of one several steps old.

--steady K W H (with --pkg-root DIR to load another checkout's package, e.g. the parent commit's): K steady
rtk_render_frame_device calls with the scene's own camera and, where the package has it, one views call with K copies of that
camera; prints one JSON line.  Run it in alternating processes to compare two commits.

    python tools/bench_views.py [--reps 15] [--warmup 3] [--out profiles/views_bench.json]
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
SCENES = {"hw09/scene5": ("hw09", "scene5.crtscene", 5), "hw11/scene8": ("hw11", "scene8.crtscene", 10)}
SHAPES = [(128, 128, k) for k in (1, 4, 16, 64)] + [(256, 256, k) for k in (1, 4, 16, 64)] + [(1920, 1080, k) for k in (1, 4, 16)]


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def scene_path(name):
    d, f, _ = SCENES[name]
    return os.path.join(ROOT, "tests", "golden", "scenes", d, f)


def orbit(a, degrees):
    """[12] float32: the scene's camera turned by `degrees` about the vertical axis through the centre of its largest mesh."""
    m = int(np.argmax(a["mesh_ntris"]))
    s = int(np.sum(a["mesh_nverts"][:m]))
    p = a["vertices"][s:s + int(a["mesh_nverts"][m])].astype(np.float64)
    c = (p.min(axis=0) + p.max(axis=0)) / 2
    th = np.deg2rad(degrees)
    ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    pos = c + ry @ (a["cam_pos"].astype(np.float64) - c)
    rows = a["cam_mat"].astype(np.float64).reshape(3, 3) @ ry.T
    return np.concatenate([pos, rows.reshape(-1)]).astype(np.float32)


def make_scene(rtk, a, cam):
    return rtk.Scene.from_arrays(a["mesh_material"], a["mesh_nverts"], a["mesh_ntris"], a["vertices"], a["indices"], a["mat_kind"],
                                 a["mat_albedo"], a["mat_ior"], a["mat_smooth"], a["light_pos"], a["light_intensity"], cam[:3], cam[3:],
                                 a["background"], a["width"], a["height"], a["bucket_size"], mat_texture=a["mat_texture"], uvs=a["uvs"],
                                 mesh_has_uvs=a["mesh_has_uvs"], tex_kind=a["tex_kind"], tex_color_a=a["tex_color_a"],
                                 tex_color_b=a["tex_color_b"], tex_param=a["tex_param"], tex_pixels=a["tex_pixels"], tex_bitmap=a["tex_bitmap"])


def wall(stream, call):
    t0 = time.perf_counter()
    call()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure_shape(rtk, torch, stream, a, depth, mode, shape, args):
    w, h, k = shape
    cams = np.stack([orbit(a, 360.0 * i / max(k, 4)) for i in range(k)])
    d_views = torch.from_numpy(cams).cuda()
    cfg = rtk.RenderConfig(width=w, height=h, max_ray_depth=depth, trace_mode=mode)
    out_a = torch.empty((k, h, w, 3), dtype=torch.float32, device="cuda")
    out_b = torch.empty_like(out_a)
    acc_a = rtk.KdTreeSimdAccel(make_scene(rtk, a, cams[0]))
    acc_b = rtk.KdTreeSimdAccel(make_scene(rtk, a, cams[0]))

    def views():
        acc_a.render_views_device(cfg, d_views.data_ptr(), k, out_a.data_ptr(), stream.cuda_stream)

    def loop():
        for v in range(k):
            acc_b.set_camera(cams[v, :3], cams[v, 3:])
            acc_b.render_frame_device(cfg, out_b[v].data_ptr(), stream.cuda_stream)

    def rebuild():
        acc = rtk.KdTreeSimdAccel(make_scene(rtk, a, cams[0]))
        acc.render_frame_device(cfg, out_b[0].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        del acc

    ta, tb, tc = [], [], []
    for i in range(args.warmup + args.reps):
        x, y = wall(stream, views), wall(stream, loop)
        assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)), "the views call and the set_camera loop render different pixels"
        z = wall(stream, rebuild) if k == 1 else None
        if i >= args.warmup:
            ta.append(x); tb.append(y)
            if z is not None:
                tc.append(z)
    res = {"w": w, "h": h, "k": k, "views": spread(ta), "loop": spread(tb)}
    res["loop_over_views"] = round(res["loop"]["ms_median"] / res["views"]["ms_median"], 3)
    res["every_views_run_faster"] = max(ta) < min(tb)
    if tc:
        res["rebuild"] = spread(tc)
    return res


def camera_move(rtk, torch, stream, a, args):
    """First frame after a 5 degree step, order kept against order reset: two accels, built under the two settings, alternating."""
    w, h = 1920, 1080
    cfg = rtk.RenderConfig(width=w, height=h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    accs = {}
    for name, env in (("kept", "1"), ("reset", "0")):
        os.environ["RTK_CAMERA_KEEPS_ORDER"] = env                 # (knobs are read when an accel is built)
        accs[name] = rtk.KdTreeSimdAccel(make_scene(rtk, a, orbit(a, 0.0)))
    del os.environ["RTK_CAMERA_KEEPS_ORDER"]
    first = {"kept": [], "reset": []}
    third = {"kept": [], "reset": []}
    for i in range(args.warmup + args.reps):
        cam = orbit(a, 5.0 * (i + 1))
        for name, acc in accs.items():
            acc.set_camera(cam[:3], cam[3:])
            t = [wall(stream, lambda: acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)) for _ in range(3)]
            for _ in range(17):                                    # settle: the order this camera leaves behind is its own
                acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            if i >= args.warmup:
                first[name].append(t[0]); third[name].append(t[2])
    return {"frame": [w, h], "step_degrees": 5.0, "first_frame": {n: spread(v) for n, v in first.items()},
            "third_frame": {n: spread(v) for n, v in third.items()},
            "every_kept_run_faster": max(first["kept"]) < min(first["reset"]),
            "every_reset_run_faster": max(first["reset"]) < min(first["kept"])}


def steady(rtk, torch, stream, args):
    k, w, h = args.steady
    a = rtk.parse_scene_file(scene_path("hw09/scene5")).arrays()
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(scene_path("hw09/scene5")))
    cfg = rtk.RenderConfig(width=w, height=h)
    out = torch.empty((k, h, w, 3), dtype=torch.float32, device="cuda")
    cam = np.concatenate([a["cam_pos"], a["cam_mat"]]).astype(np.float32)
    d_views = torch.from_numpy(np.ascontiguousarray(np.tile(cam, (k, 1)))).cuda()

    def frames():
        for v in range(k):
            acc.render_frame_device(cfg, out[v].data_ptr(), stream.cuda_stream)

    def views():
        acc.render_views_device(cfg, d_views.data_ptr(), k, out.data_ptr(), stream.cuda_stream)

    res = {"tool": "bench_views --steady", "k": k, "w": w, "h": h}
    variants = {"frames": frames}
    if hasattr(acc, "render_views_device"):
        variants["views"] = views
    times = {n: [] for n in variants}
    for i in range(args.warmup + args.reps):
        for n, f in variants.items():
            t = wall(stream, f)
            if i >= args.warmup:
                times[n].append(t)
    for n, t in times.items():
        res[n] = spread(t)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--steady", type=int, nargs=3, metavar=("K", "W", "H"))
    ap.add_argument("--pkg-root", default=ROOT)
    args = ap.parse_args()
    import torch

    sys.path.insert(0, args.pkg_root)
    import __graft_entry__ as ge

    ge.build()
    rtk = importlib.import_module("simd-raytracer_amd")
    if rtk.device_count() < 1:
        raise SystemExit("bench_views needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        if args.steady:
            result = steady(rtk, torch, stream, args)
        else:
            import bench  # (code_hash: the hash bench.py stamps its results with)
            result = {"tool": "bench_views", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "scenes": {}}
            for name, (_, _, depth) in SCENES.items():
                sc = rtk.parse_scene_file(scene_path(name))
                a = sc.arrays()
                runs = [("auto", rtk.TRACE_AUTO)] + ([("group4", rtk.TRACE_GROUP4)] if name == "hw11/scene8" else [])
                result["scenes"][name] = {m: [measure_shape(rtk, torch, stream, a, depth, mode, s, args) for s in SHAPES] for m, mode in runs}
            a5 = rtk.parse_scene_file(scene_path("hw09/scene5")).arrays()
            result["camera_move"] = camera_move(rtk, torch, stream, a5, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
