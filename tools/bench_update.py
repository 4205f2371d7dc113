"""Times rtk_accel_update_vertices_device against what the C-ABI offered before it for geometry that moves.

Per update of every vertex, alternating between two poses, on hw09/scene5 (4,014 triangles) and on a generated height field of
about 2 * 10^5 triangles:
  update   rtk_accel_update_vertices_device from a device tensor: the time between two events on the stream, and the host's wall
           time around the call (it blocks the host once), then the first frame after it
  rebuild  rtk_scene_create + rtk_accel_build of the moved scene + rtk_accel_destroy of the old accel (host wall time), then the
           first frame of the new accel, which pays its upload (ensure_device)
Frames are rendered at the scene's own size into a device buffer and timed by the host from call to idle stream, so the upload of
the rebuilt accel counts.  Both paths run alternately in one process after warm-up; the tool asserts that they give the same
frame before it reports a time.  Prints one JSON line; --out also writes it to a file (profiles/update_bench.json).

    python tools/bench_update.py [--reps 15] [--warmup 3] [--out profiles/update_bench.json]
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
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (code_hash: the hash bench.py stamps its results with)

SCENE5 = os.path.join(ROOT, "tests", "golden", "scenes", "hw09", "scene5.crtscene")


def scene5_arrays(rtk):
    a = rtk.parse_scene_file(SCENE5).arrays()
    info = rtk.parse_scene_file(SCENE5).info
    a["width"], a["height"], a["bucket_size"] = info.width, info.height, info.bucket_size
    return a


def height_field_arrays(g=317):
    """A g x g grid over [-8, 8]^2: 2 (g - 1)^2 triangles (g = 317: 199,712), one diffuse material, two lights."""
    xs, zs = np.meshgrid(np.linspace(-8, 8, g), np.linspace(-8, 8, g), indexing="ij")
    ys = 0.5 * np.sin(1.3 * xs) * np.cos(0.9 * zs) - 1.0
    v = np.stack([xs, ys, zs], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(g - 1), np.arange(g - 1), indexing="ij")
    a = (i * g + j).reshape(-1)
    t = np.stack([np.stack([a, a + 1, a + g], axis=1), np.stack([a + 1, a + g + 1, a + g], axis=1)], axis=1).reshape(-1, 3)
    c, s = np.cos(0.45), np.sin(0.45)
    return dict(mesh_material=np.array([0], np.int32), mesh_nverts=np.array([len(v)], np.int32), mesh_ntris=np.array([len(t)], np.int32),
                vertices=v, indices=t.astype(np.uint32), mat_kind=np.array([0], np.int32),
                mat_albedo=np.array([[0.8, 0.7, 0.5]], np.float32), mat_ior=np.array([1.0], np.float32), mat_smooth=np.array([1], np.int32),
                light_pos=np.array([[3, 6, 2], [-5, 8, -3]], np.float32), light_intensity=np.array([900, 700], np.float32),
                cam_pos=np.array([0, 5, 12], np.float32), cam_mat=np.array([1, 0, 0, 0, c, -s, 0, s, c], np.float32),
                background=np.array([0.1, 0.2, 0.3], np.float32), width=1280, height=720, bucket_size=64)


def poses(a):
    """Two poses of every vertex: as given, and bent (a wave along x, a stretch in y)."""
    v = a["vertices"].astype(np.float64)
    w = v.copy()
    w[:, 1] = v[:, 1] * 1.15 + 0.3 * np.sin(0.8 * v[:, 0])
    w[:, 2] = v[:, 2] + 0.2 * np.cos(0.5 * v[:, 0])
    return [np.ascontiguousarray(v.astype(np.float32)), np.ascontiguousarray(w.astype(np.float32))]


def make_scene(rtk, a, vertices):
    return rtk.Scene.from_arrays(a["mesh_material"], a["mesh_nverts"], a["mesh_ntris"], vertices, a["indices"], a["mat_kind"], a["mat_albedo"],
                                 a["mat_ior"], a["mat_smooth"], a["light_pos"], a["light_intensity"], a["cam_pos"], a["cam_mat"],
                                 a["background"], a["width"], a["height"], a["bucket_size"])


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def measure(rtk, torch, stream, a, args):
    pose = poses(a)
    d_pose = [torch.from_numpy(p).cuda() for p in pose]
    cfg = rtk.RenderConfig(width=a["width"], height=a["height"])
    out_u = torch.empty((a["height"], a["width"], 3), dtype=torch.float32, device="cuda")
    out_r = torch.empty_like(out_u)
    upd = rtk.KdTreeSimdAccel(make_scene(rtk, a, pose[0]))
    holder = {"acc": rtk.KdTreeSimdAccel(make_scene(rtk, a, pose[0]))}
    ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]

    def frame(acc, out):
        t0 = time.perf_counter()
        acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def update(k):
        ev[0].record(stream)
        t0 = time.perf_counter()
        upd.update_vertices_device(d_pose[k].data_ptr(), stream.cuda_stream)
        t_call = (time.perf_counter() - t0) * 1e3
        ev[1].record(stream)
        stream.synchronize()
        t_idle = (time.perf_counter() - t0) * 1e3
        return ev[0].elapsed_time(ev[1]), t_call, t_idle, frame(upd, out_u)

    def rebuild(k):
        t0 = time.perf_counter()
        new = rtk.KdTreeSimdAccel(make_scene(rtk, a, pose[k]))
        old, holder["acc"] = holder["acc"], new
        del old                                                                # rtk_accel_destroy: frees every device buffer of the old accel
        t_host = (time.perf_counter() - t0) * 1e3
        return t_host, frame(new, out_r)

    frame(upd, out_u); frame(holder["acc"], out_r)
    for i in range(args.warmup):
        update((i + 1) % 2); rebuild((i + 1) % 2)
        assert torch.equal(out_u, out_r), "the updated and the rebuilt accel render different frames"
    u, r = [], []
    for i in range(args.reps):                                                 # alternating: both see the same machine
        k = (i + args.warmup + 1) % 2
        u.append(update(k))
        r.append(rebuild(k))
        assert torch.equal(out_u, out_r), "the updated and the rebuilt accel render different frames"
    steady = [frame(upd, out_u) for _ in range(args.reps)]
    ti = upd.tree_info()
    res = {"triangles": int(ti.n_triangles), "nodes": int(ti.n_nodes), "leaf_refs": int(ti.n_leaf_refs), "frame": [a["width"], a["height"]],
           "update": {"stream_events": spread([x[0] for x in u]), "host_call": spread([x[1] for x in u]), "host_until_idle": spread([x[2] for x in u]),
                      "first_frame": spread([x[3] for x in u])},
           "rebuild": {"host_create_build_destroy": spread([x[0] for x in r]), "first_frame_with_upload": spread([x[1] for x in r])},
           "steady_frame": spread(steady)}
    res["update_to_first_frame_ms"] = round(res["update"]["host_until_idle"]["ms_median"] + res["update"]["first_frame"]["ms_median"], 4)
    res["rebuild_to_first_frame_ms"] = round(res["rebuild"]["host_create_build_destroy"]["ms_median"] + res["rebuild"]["first_frame_with_upload"]["ms_median"], 4)
    res["rebuild_over_update"] = round(res["rebuild_to_first_frame_ms"] / res["update_to_first_frame_ms"], 3)
    return res


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
        raise SystemExit("bench_update needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    result = {"tool": "bench_update", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "scenes": {}}
    with torch.cuda.stream(stream):
        result["scenes"]["hw09/scene5"] = measure(rtk, torch, stream, scene5_arrays(rtk), args)
        result["scenes"]["height field"] = measure(rtk, torch, stream, height_field_arrays(), args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
