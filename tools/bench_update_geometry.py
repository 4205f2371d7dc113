"""Times rtk_accel_update_geometry_device against the path it replaces for geometry whose TRIANGLES change.

Per change of the triangle lists, alternating between the full lists and every mesh cut to the first 3/4 of its triangles (the
vertices stay), on hw09/scene5 (4,014 triangles) and on bench_update.py's height field (199,712):
  geometry  rtk_accel_update_geometry_device from device tensors: the time between two events on the stream, the host's wall time
            around the call (it blocks the host once) and until the stream is idle, then the first frame after it
  rebuild   rtk_scene_create + rtk_accel_build of the changed scene + rtk_accel_destroy of the old accel (host wall time), then the
            first frame of the new accel, which pays its upload
  vertices  rtk_accel_update_vertices_device on the accel the geometry update left, i.e. the same topology: what the topology
            tables cost on top of the rebuild of the tree
Frames are 1920 x 1080 into a device buffer, timed by the host from call to idle stream.  All paths run alternately in one
process after warm-up; the tool asserts that the updated and the rebuilt accel give the same frame before it reports a time.
Prints one JSON line; --out also writes it to a file (profiles/update_geometry_bench.json).

    python tools/bench_update_geometry.py [--reps 15] [--warmup 3] [--out profiles/update_geometry_bench.json]
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
from bench_update import height_field_arrays, scene5_arrays, spread  # noqa: E402

FRAME = (1920, 1080)


def topologies(a):
    """(indices, mesh_ntris) twice: as given, and every mesh cut to the first 3/4 of its triangles."""
    lists = np.split(a["indices"], np.cumsum(a["mesh_ntris"])[:-1])
    cut = [t[: (3 * len(t)) // 4] for t in lists]
    return [(np.ascontiguousarray(a["indices"], np.uint32), np.ascontiguousarray(a["mesh_ntris"], np.int32)),
            (np.ascontiguousarray(np.concatenate(cut), np.uint32), np.array([len(t) for t in cut], np.int32))]


def make_scene(rtk, a, topo):
    return rtk.Scene.from_arrays(a["mesh_material"], a["mesh_nverts"], topo[1], a["vertices"], topo[0], a["mat_kind"], a["mat_albedo"],
                                 a["mat_ior"], a["mat_smooth"], a["light_pos"], a["light_intensity"], a["cam_pos"], a["cam_mat"],
                                 a["background"], a["width"], a["height"], a["bucket_size"])


def measure(rtk, torch, stream, a, args):
    topo = topologies(a)
    d_v = torch.from_numpy(np.ascontiguousarray(a["vertices"], np.float32)).cuda()
    d_idx = [torch.from_numpy(t[0].view(np.int32)).cuda() for t in topo]
    cfg = rtk.RenderConfig(width=FRAME[0], height=FRAME[1])
    out_u = torch.empty((FRAME[1], FRAME[0], 3), dtype=torch.float32, device="cuda")
    out_r = torch.empty_like(out_u)
    upd = rtk.KdTreeSimdAccel(make_scene(rtk, a, topo[0]))
    holder = {"acc": rtk.KdTreeSimdAccel(make_scene(rtk, a, topo[0]))}
    ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]

    def frame(acc, out):
        t0 = time.perf_counter()
        acc.render_frame_device(cfg, out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed(call):
        ev[0].record(stream)
        t0 = time.perf_counter()
        call()
        t_call = (time.perf_counter() - t0) * 1e3
        ev[1].record(stream)
        stream.synchronize()
        t_idle = (time.perf_counter() - t0) * 1e3
        return ev[0].elapsed_time(ev[1]), t_call, t_idle, frame(upd, out_u)

    def geometry(k):
        return timed(lambda: upd.update_geometry_device(d_v.data_ptr(), d_idx[k].data_ptr(), topo[k][1], stream.cuda_stream))

    def vertices():
        return timed(lambda: upd.update_vertices_device(d_v.data_ptr(), stream.cuda_stream))

    def rebuild(k):
        t0 = time.perf_counter()
        new = rtk.KdTreeSimdAccel(make_scene(rtk, a, topo[k]))
        old, holder["acc"] = holder["acc"], new
        del old                                                                # rtk_accel_destroy: frees every device buffer of the old accel
        t_host = (time.perf_counter() - t0) * 1e3
        return t_host, frame(new, out_r)

    frame(upd, out_u); frame(holder["acc"], out_r)
    g, v, r = [], [], []
    for i in range(args.warmup + args.reps):                                   # alternating: all paths see the same machine
        k = (i + 1) % 2
        x, y, z = geometry(k), rebuild(k), None
        assert torch.equal(out_u, out_r), "the updated and the rebuilt accel render different frames"
        z = vertices()
        assert torch.equal(out_u, out_r), "update_vertices on the new topology renders a different frame"
        if i >= args.warmup:
            g.append(x); r.append(y); v.append(z)
    ti = upd.tree_info()

    def update_stats(u):
        return {"stream_events": spread([x[0] for x in u]), "host_call": spread([x[1] for x in u]), "host_until_idle": spread([x[2] for x in u]),
                "first_frame": spread([x[3] for x in u])}

    res = {"triangles": [int(t[1].sum()) for t in topo], "last": {"triangles": int(ti.n_triangles), "nodes": int(ti.n_nodes), "leaf_refs": int(ti.n_leaf_refs)},
           "frame": list(FRAME), "geometry": update_stats(g), "vertices_same_topology": update_stats(v),
           "rebuild": {"host_create_build_destroy": spread([x[0] for x in r]), "first_frame_with_upload": spread([x[1] for x in r])}}
    res["geometry_to_first_frame_ms"] = round(res["geometry"]["host_until_idle"]["ms_median"] + res["geometry"]["first_frame"]["ms_median"], 4)
    res["rebuild_to_first_frame_ms"] = round(res["rebuild"]["host_create_build_destroy"]["ms_median"] + res["rebuild"]["first_frame_with_upload"]["ms_median"], 4)
    res["rebuild_over_geometry"] = round(res["rebuild_to_first_frame_ms"] / res["geometry_to_first_frame_ms"], 3)
    res["rebuild_host_over_geometry_until_idle"] = round(res["rebuild"]["host_create_build_destroy"]["ms_median"] / res["geometry"]["host_until_idle"]["ms_median"], 3)
    res["geometry_over_vertices"] = round(res["geometry"]["host_until_idle"]["ms_median"] / res["vertices_same_topology"]["host_until_idle"]["ms_median"], 3)
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
        raise SystemExit("bench_update_geometry needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    result = {"tool": "bench_update_geometry", "code_hash": bench.code_hash(), "reps": args.reps, "warmup": args.warmup,
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
