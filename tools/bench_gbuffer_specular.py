"""Measures rtk_render_gbuffer_specular: what the call costs between its floor and its ceiling, and what its planes buy the
temporal step and the denoiser behind mirrors and glass.

  time     1920 x 1080 on hw09/scene5 (a mirror floor), hw11/scene8 (glass) and hw09/scene5 with every material turned diffuse
           ("nothing specular").  Sides, alternating inside the repetition loop of one process, every call between device events
           on the call's stream: rtk_render_gbuffer_device with its eight planes (the floor: on the non-specular variant both
           calls trace the same rays), rtk_render_gbuffer_specular_device with the eight shared planes and with all twelve, and
           rtk_render_frame_device at spp = 1 and the same depth (the ceiling: the frame traces these rays plus every shadow ray).
           Before a time counts the tool checks that, where bounces == 0, the shared planes of the two calls hold the same bits.
  quality  hw09/scene5 (a PLANAR mirror floor under the dragon) and hw15/scene2 (a mirror SPHERE beside a glass sphere), both under
           diffuse GI, depth 5, one diffuse ray, the half-degree orbit of tools/bench_temporal.py: 16 frames of 8 spp, RMSE against
           512 spp of the last frame, over the frame and over the pixels with bounces > 0, split by the material of the first hit
           into pixels behind a mirror and pixels behind glass.  The sequence is rendered
           once and replayed through rtk_temporal_accumulate, plain and clamped, each with and without rtk_denoise_frame behind it,
           fed depth / position / normal / mesh of rtk_render_gbuffer and fed those of this call (the albedo plane is
           rtk_render_gbuffer's on both sides).

    python tools/bench_gbuffer_specular.py [--reps 15] [--warmup 3] [--size 960] [--skip-quality] [--out profiles/gbuffer_specular_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_temporal import GUIDES, SCENE, rmse, spread, timed  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SHARED = {"depth": 1, "position": 3, "normal": 3, "albedo": 3, "bary": 2, "tri": 1, "mesh": 1, "material": 1}
EXTRA = {"surface_position": 3, "surface_normal": 3, "bounces": 1, "last_ray": 6}
DIFFUSE = 0


def time_scene(torch, rtk, stream, name, path, diffuse, args):
    w, h = args.width, args.height
    n = w * h
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    if diffuse:
        m = acc.materials()
        acc.set_materials(np.full_like(m["kind"], DIFFUSE), m["albedo"], m["ior"], m["smooth"], m["texture"])
    cfg = rtk.RenderConfig(width=w, height=h, spp=1, max_ray_depth=args.depth)
    s = stream.cuda_stream
    gb = {p: torch.zeros(n * c, dtype=torch.int32, device="cuda") for p, c in SHARED.items()}
    sp = {p: torch.zeros(n * c, dtype=torch.int32, device="cuda") for p, c in {**SHARED, **EXTRA}.items()}
    rgb = torch.zeros(acc.output_floats(cfg), dtype=torch.float32, device="cuda")
    calls = {
        "gbuffer_8": lambda: acc.render_gbuffer_device(cfg, {p: t.data_ptr() for p, t in gb.items()}, 0, 0, 1, s),
        "specular_shared_8": lambda: acc.render_gbuffer_specular_device(cfg, {p: sp[p].data_ptr() for p in SHARED}, 0, 0, 1, s),
        "specular_12": lambda: acc.render_gbuffer_specular_device(cfg, {p: t.data_ptr() for p, t in sp.items()}, 0, 0, 1, s),
        "frame_spp1": lambda: acc.render_frame_device(cfg, rgb.data_ptr(), s),
    }
    times = {key: [] for key in calls}
    for i in range(args.warmup + args.reps):
        for key, call in calls.items():
            t = timed(torch, stream, call)
            if i >= args.warmup:
                times[key].append(t)
        if i == 0:          # the same answers where the chain has no bounce, before any time counts
            direct = sp["bounces"] == 0
            for p, c in SHARED.items():
                d = direct[:, None].expand(n, c).reshape(-1)
                assert torch.equal(sp[p][d], gb[p][d]), f"{name}: plane {p} differs from rtk_render_gbuffer where bounces == 0"
    bounces = sp["bounces"].cpu().numpy()
    res = {"scene": name, "w": w, "h": h, "max_ray_depth": args.depth,
           "pixels_by_bounces": np.bincount(bounces, minlength=args.depth + 1).tolist(),
           "secondary_rays": int(bounces.sum()), **{key: spread(t) for key, t in times.items()}}
    g, f = res["gbuffer_8"]["ms_median"], res["frame_spp1"]["ms_median"]
    for key in ("specular_shared_8", "specular_12"):
        res[key]["over_gbuffer"] = round(res[key]["ms_median"] / g, 3)
        res[key]["ms_over_gbuffer"] = round(res[key]["ms_median"] - g, 4)
        res[key]["under_frame"] = res[key]["ms_median"] < f
        res[key]["every_run_under_every_frame_run"] = max(times[key]) < min(times["frame_spp1"])
    res["bytes_written"] = {"gbuffer_8": 4 * n * sum(SHARED.values()), "specular_12": 4 * n * (sum(SHARED.values()) + sum(EXTRA.values()))}
    return res


def quality_part(torch, rtk, args, name, path, centre=None):
    """`centre`: the point the camera orbits about its vertical axis; None = the middle of the scene's largest mesh"""
    w = h = args.size
    n = w * h
    scene = rtk.parse_scene_file(path)
    acc = rtk.KdTreeSimdAccel(scene)
    if centre is None:
        a = scene.arrays()
        big = int(np.argmax(a["mesh_ntris"]))
        first = int(np.sum(a["mesh_nverts"][:big]))
        v = np.asarray(a["vertices"], np.float64).reshape(-1, 3)[first:first + int(a["mesh_nverts"][big])]
        centre = 0.5 * (v.min(axis=0) + v.max(axis=0))
    kw = dict(width=w, height=h, max_ray_depth=5, diffuse_rays=1, trace_mode=rtk.TRACE_STREAM)
    fov = rtk.RenderConfig(**kw).fov_degrees
    dcfg, tcfg, clamp = rtk.DenoiseConfig(), rtk.TemporalConfig(fov_degrees=fov), rtk.ClampConfig()
    home = acc.camera()
    frames_n, last = args.frames, args.frames - 1
    centre = np.asarray(centre, np.float64)
    arm = home[0].astype(np.float64) - centre

    def orbit_view(k):      # tools/bench_temporal.py: half a degree a frame, ending at the scene's own camera
        t = np.deg2rad(0.5 * (k - last))
        c, s_ = np.cos(t), np.sin(t)
        r = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
        return (centre + r @ arm).astype(np.float32), (home[1].reshape(3, 3).astype(np.float64) @ r.T).astype(np.float32).reshape(9)

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        f32 = lambda m: torch.zeros(m, dtype=torch.float32, device="cuda")      # noqa: E731
        d_ref, d_out = f32(n * 3), f32(n * 3)
        hist = [{"rgb": f32(n * 3), "noise": f32(n), "length": f32(n)} for _ in (0, 1)]
        need = rtk.denoise_workspace_bytes(w, h, 1, dcfg)
        ws = f32(need // 4)
        shapes = (("depth", 1), ("position", 3), ("normal", 3), ("mesh", 1))
        try:
            frames = []
            for k in range(frames_n):
                view = orbit_view(k)
                acc.set_camera(*view)
                f = {"rgb": f32(n * 3), "noise": f32(n), "view": view, "first": {x: f32(n * c) for x, c in shapes},
                     "specular": {x: f32(n * c) for x, c in shapes}}
                acc.render_frame_noise_device(rtk.RenderConfig(spp=8, seed=100 + k, **kw), f["rgb"].data_ptr(), f["noise"].data_ptr(), s)
                g1 = rtk.RenderConfig(spp=1, **kw)
                if k == last:
                    f["albedo"], f["bounces"] = f32(n * 3), f32(n)
                    acc.render_gbuffer_device(g1, dict({x: t.data_ptr() for x, t in f["first"].items()}, albedo=f["albedo"].data_ptr()), sample=0, stream=s)
                    acc.render_gbuffer_specular_device(g1, dict({x: t.data_ptr() for x, t in f["specular"].items()}, bounces=f["bounces"].data_ptr()),
                                                       sample=0, stream=s)
                else:
                    acc.render_gbuffer_device(g1, {x: t.data_ptr() for x, t in f["first"].items()}, sample=0, stream=s)
                    acc.render_gbuffer_specular_device(g1, {x: t.data_ptr() for x, t in f["specular"].items()}, sample=0, stream=s)
                frames.append(f)
            acc.set_camera(*home)
            for b in range(0, args.ref_spp, 16):
                acc.render_frame_device(rtk.RenderConfig(spp=args.ref_spp, seed=0, sample_begin=b, sample_count=min(16, args.ref_spp - b), **kw),
                                        d_ref.data_ptr(), s)
            stream.synchronize()
            g = frames[-1]
            bounces = g["bounces"].view(torch.int32)
            # the pixels behind a mirror and behind glass, by the material of the FIRST hit
            first_mat = acc.materials()["kind"]
            mesh_first = g["first"]["mesh"].view(torch.int32).cpu().numpy()
            mesh_mat = acc.scene.arrays()["mesh_material"]
            kind_first = np.where(mesh_first >= 0, first_mat[mesh_mat[np.where(mesh_first >= 0, mesh_first, 0)]], -1)
            masks = {"frame": torch.ones(n, dtype=torch.bool, device="cuda"), "bounces_gt_0": bounces > 0,
                     "first_hit_mirror": torch.from_numpy(kind_first == 1).cuda() & (bounces > 0),
                     "first_hit_glass": torch.from_numpy(kind_first == 2).cuda() & (bounces > 0)}
            masks3 = {key: m[:, None].expand(n, 3).reshape(-1) for key, m in masks.items()}

            def row(rgb, **more):
                return dict({f"rmse_{key}": round(rmse(torch, rgb[m3], d_ref[m3]), 5) for key, m3 in masks3.items()}, **more)

            def replay(guides, cl):
                for k, f in enumerate(frames):
                    cur = dict(rgb=f["rgb"].data_ptr(), noise=f["noise"].data_ptr(), **{x: f[guides][x].data_ptr() for x in GUIDES})
                    prev = None
                    if k > 0:
                        q = frames[k - 1]
                        prev = dict({x: t.data_ptr() for x, t in hist[(k - 1) & 1].items()}, view=q["view"], **{x: q[guides][x].data_ptr() for x in GUIDES})
                    rtk.temporal_accumulate_device(w, h, cur, prev, {x: t.data_ptr() for x, t in hist[k & 1].items()}, cfg=tcfg, stream=s, clamp=cl)
                return hist[(len(frames) - 1) & 1]

            def filt(guides, rgb, noise):
                p = g[guides]
                rtk.denoise_device(w, h, rgb.data_ptr(), p["normal"].data_ptr(), p["position"].data_ptr(), p["depth"].data_ptr(), d_out.data_ptr(),
                                   ws.data_ptr(), need, d_noise_ptr=noise.data_ptr(), d_albedo_ptr=g["albedo"].data_ptr(), cfg=dcfg, stream=s)
                return d_out

            out = {"pixel_share": {key: round(float(m.float().mean().item()), 4) for key, m in masks.items()}, "last_frame_8spp": row(g["rgb"])}
            for guides in ("first", "specular"):
                side = {"last_frame_8spp_denoised": row(filt(guides, g["rgb"], g["noise"]))}
                for label, cl in (("plain", None), ("clamped", clamp)):
                    hs = replay(guides, cl)
                    mean_len = {key: round(float(hs["length"][m].mean().item()), 3) for key, m in masks.items()}
                    side[f"temporal_{label}"] = row(hs["rgb"], mean_history_length=mean_len)
                    side[f"temporal_{label}_denoised"] = row(filt(guides, hs["rgb"], hs["noise"]))
                out["fed_rtk_gbuffer" if guides == "first" else "fed_rtk_gbuffer_specular"] = side
            stream.synchronize()
        finally:
            acc.set_camera(*home)
    return {"scene": name, "orbit_centre": [round(float(x), 4) for x in centre], "w": w, "h": h, "max_ray_depth": 5, "diffuse_rays": 1, "spp": 8, "ref_spp": args.ref_spp, "frames": frames_n,
            "orbit_degrees_per_frame": 0.5, "clamp": dict(radius=clamp.radius, gamma=clamp.gamma, history_keep=clamp.history_keep),
            "rmse_is": "against ref_spp of the last frame; per pixel set of the last frame: the frame, bounces > 0, and of those the "
                       "pixels whose first hit is a mirror / is glass", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--size", type=int, default=960, help="of the quality part's square frames")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=512)
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
        raise SystemExit("bench_gbuffer_specular needs a HIP device: the rtk engine has no CPU path")
    import bench  # (code_hash: the hash bench.py stamps its results with)

    result = {"tool": "bench_gbuffer_specular", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "timing": "device events around every call, sides alternating in one process"}

    def save():
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result) + "\n")

    if not args.skip_time:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            result["time"] = [time_scene(torch, rtk, stream, name, os.path.join(SCENES, *name.split("/")) + ".crtscene", diffuse, args)
                              for name, diffuse in (("hw09/scene5", False), ("hw11/scene8", False), ("hw09/scene5", True))]
            result["time"][2]["scene"] = "hw09/scene5, every material diffuse"
        save()
    if not args.skip_quality:
        # a planar mirror (the floor of hw09/scene5) and a curved one beside curved glass (the two spheres of hw15/scene2), under GI
        result["quality"] = [quality_part(torch, rtk, args, "hw09/scene5", os.path.join(SCENES, "hw09", "scene5.crtscene")),
                             quality_part(torch, rtk, args, "hw15/scene2", SCENE, centre=(0.0, 0.0, -3.0))]
    print(json.dumps(result))
    save()


if __name__ == "__main__":
    main()
