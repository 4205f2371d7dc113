"""Times the texel setters of a live accel against the only route the C-ABI offered before them to the same pixels.

On hw12/scene4 (four textured quads; the bitmap quad shows a 1024 x 1024 bitmap here), every time to the end of the next
1920 x 1080 frame into a device buffer (host wall time from the call until the stream is idle), alternating between two bitmaps:
  pixels_device  rtk_accel_set_texture_pixels_device with the bytes in device memory, then the frame
  frame_device   rtk_accel_set_texture_frame_device with the float frame those bytes are the quantisation of, then the frame
  rebuild        rtk_scene_create + rtk_accel_build of the scene with the new bytes + rtk_accel_destroy of the old accel, then the
                 new accel's first frame (which pays its upload)
The three run alternately in one process after warm-up, and the tool asserts that they give the same frame before it reports.
  view_on_quad   a 512 x 512 view through rtk_render_views_device, rtk_accel_set_texture_frame_device of it, then the frame: a
                 rendered view on a "screen" of the next frame without leaving the device
What the device synchronisation at the setters' entry costs: N frames enqueued back to back with a replacement before each,
against the same N frames with a plain device-to-device copy of the bytes before each (what a setter that did not have to wait
would enqueue), and against the frames alone; per frame.
Prints one JSON line; --out also writes it to a file (profiles/textures_bench.json).

    python tools/bench_textures.py [--reps 15] [--warmup 3] [--out profiles/textures_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (code_hash: the hash bench.py stamps its results with)
from bench_update import spread  # noqa: E402

SCENE4 = os.path.join(ROOT, "tests", "golden", "scenes", "hw12", "scene4.crtscene")
BITMAP = 3
W, H = 1920, 1080
TEX = 1024
VIEW = 512


def scene4_arrays(rtk):
    sc = rtk.parse_scene_file(SCENE4)
    a = sc.arrays()
    a["width"], a["height"], a["bucket_size"] = sc.info.width, sc.info.height, sc.info.bucket_size
    return a


def with_bitmap(a, px):
    """the scene's arrays with its (one) bitmap replaced by uint8 [h, w, 3]"""
    b = dict(a)
    t = int(np.flatnonzero(a["tex_kind"] == BITMAP)[0])
    bm = a["tex_bitmap"].copy()
    bm[t] = (0, px.shape[1], px.shape[0])
    b["tex_bitmap"], b["tex_pixels"] = bm, np.ascontiguousarray(px).reshape(-1)
    return b, t


def make_scene(rtk, a):
    return rtk.Scene.from_arrays(a["mesh_material"], a["mesh_nverts"], a["mesh_ntris"], a["vertices"], a["indices"], a["mat_kind"],
                                 a["mat_albedo"], a["mat_ior"], a["mat_smooth"], a["light_pos"], a["light_intensity"], a["cam_pos"],
                                 a["cam_mat"], a["background"], a["width"], a["height"], a["bucket_size"], mat_texture=a["mat_texture"],
                                 uvs=a["uvs"], mesh_has_uvs=a["mesh_has_uvs"], tex_kind=a["tex_kind"], tex_color_a=a["tex_color_a"],
                                 tex_color_b=a["tex_color_b"], tex_param=a["tex_param"], tex_pixels=a["tex_pixels"], tex_bitmap=a["tex_bitmap"])


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
        raise SystemExit("bench_textures needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    a = scene4_arrays(rtk)
    cfg = rtk.RenderConfig(width=W, height=H)
    result = {"tool": "bench_textures", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "scene": "hw12/scene4", "frame": [W, H], "bitmap": [TEX, TEX], "view": [VIEW, VIEW]}
    with torch.cuda.stream(stream):
        # two float frames, and the bytes they quantise to
        rng = np.random.default_rng(12)
        d_frames = [torch.from_numpy(rng.uniform(0, 1, (TEX, TEX, 3)).astype(np.float32)).cuda() for _ in range(2)]
        d_bytes = [torch.empty((TEX, TEX, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        for f, b in zip(d_frames, d_bytes):
            rtk.frame_to_rgb8_device(f.data_ptr(), f.numel(), b.data_ptr(), s)
        stream.synchronize()
        states = [with_bitmap(a, b.cpu().numpy())[0] for b in d_bytes]
        tex = with_bitmap(a, d_bytes[0].cpu().numpy())[1]
        outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3)]

        def frame(acc, out):
            acc.render_frame_device(cfg, out.data_ptr(), s)
            stream.synchronize()

        by_bytes, by_frame = rtk.KdTreeSimdAccel(make_scene(rtk, states[0])), rtk.KdTreeSimdAccel(make_scene(rtk, states[0]))
        holder = {"acc": rtk.KdTreeSimdAccel(make_scene(rtk, states[0]))}

        def go_bytes(k):
            t0 = time.perf_counter()
            by_bytes.set_texture_pixels_device(tex, TEX, TEX, d_bytes[k].data_ptr(), s)
            frame(by_bytes, outs[0])
            return (time.perf_counter() - t0) * 1e3

        def go_frame(k):
            t0 = time.perf_counter()
            by_frame.set_texture_frame_device(tex, TEX, TEX, d_frames[k].data_ptr(), s)
            frame(by_frame, outs[1])
            return (time.perf_counter() - t0) * 1e3

        def go_rebuild(k):
            t0 = time.perf_counter()
            new = rtk.KdTreeSimdAccel(make_scene(rtk, states[k]))
            old, holder["acc"] = holder["acc"], new
            del old
            frame(new, outs[2])
            return (time.perf_counter() - t0) * 1e3

        frame(by_bytes, outs[0]); frame(by_frame, outs[1]); frame(holder["acc"], outs[2])
        t_bytes, t_frame, t_rebuild = [], [], []
        for i in range(args.warmup + args.reps):                     # alternating: all three see the same machine
            k = (i + 1) % 2
            x, y, z = go_bytes(k), go_frame(k), go_rebuild(k)
            assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2]), "the live and the rebuilt accel render different frames"
            if i >= args.warmup:
                t_bytes.append(x); t_frame.append(y); t_rebuild.append(z)
        steady = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            frame(by_bytes, outs[0])
            steady.append((time.perf_counter() - t0) * 1e3)
        result["replace_and_frame"] = {
            "set_texture_pixels_device": spread(t_bytes), "set_texture_frame_device": spread(t_frame),
            "create_build_destroy_and_first_frame": spread(t_rebuild), "steady_frame": spread(steady),
            "rebuild_over_pixels_device_median": round(spread(t_rebuild)["ms_median"] / spread(t_bytes)["ms_median"], 2),
            "rebuild_over_frame_device_median": round(spread(t_rebuild)["ms_median"] / spread(t_frame)["ms_median"], 2)}

        # a view on the quad, entirely on the device
        screen = rtk.KdTreeSimdAccel(make_scene(rtk, with_bitmap(a, np.zeros((VIEW, VIEW, 3), np.uint8))[0]))
        vcfg = rtk.RenderConfig(width=VIEW, height=VIEW)
        pos, mat = screen.camera()
        views = [np.concatenate([pos + np.array([dx, 0.0, 0.0], np.float32), mat]).astype(np.float32)[None, :] for dx in (0.0, 0.5)]
        d_views = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in views]
        d_view_out = torch.empty((1, VIEW, VIEW, 3), dtype=torch.float32, device="cuda")
        stream.synchronize()
        frame(screen, outs[0])
        t_view, t_parts = [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            screen.render_views_device(vcfg, d_views[i % 2].data_ptr(), 1, d_view_out.data_ptr(), s)
            stream.synchronize()
            t1 = time.perf_counter()
            screen.set_texture_frame_device(tex, VIEW, VIEW, d_view_out.data_ptr(), s)
            frame(screen, outs[0])
            t2 = time.perf_counter()
            if i >= args.warmup:
                t_view.append((t2 - t0) * 1e3); t_parts.append((t1 - t0) * 1e3)
        result["view_on_quad"] = {"view_texture_and_frame": spread(t_view), "of_which_the_view": spread(t_parts)}

        # what the synchronisation at entry costs per replaced frame
        n = 20
        spare = torch.empty_like(d_bytes[0])

        def run(before_each):
            stream.synchronize()
            t0 = time.perf_counter()
            for j in range(n):
                before_each(j)
                by_bytes.render_frame_device(cfg, outs[0].data_ptr(), s)
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        loops = {"setter_then_frame": lambda j: by_bytes.set_texture_pixels_device(tex, TEX, TEX, d_bytes[j % 2].data_ptr(), s),
                 "plain_copy_then_frame": lambda j: spare.copy_(d_bytes[j % 2], non_blocking=True),
                 "frame_alone": lambda j: None}
        per = {k: [] for k in loops}
        for i in range(args.warmup + args.reps):
            for k, f in loops.items():
                t = run(f)
                if i >= args.warmup:
                    per[k].append(t)
        q = {k: spread(v) for k, v in per.items()}
        q["frames_per_loop"] = n
        q["sync_at_entry_ms_per_frame_median"] = round(q["setter_then_frame"]["ms_median"] - q["plain_copy_then_frame"]["ms_median"], 4)
        result["back_to_back_per_frame"] = q
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
