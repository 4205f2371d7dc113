"""Times the batched occlusion query (rtk_accel_occluded_device) against its emulation with what the C-ABI offered before it.

Workload: hw09/scene5 and hw11/scene8 at 1920x1080, the shadow ray of every camera hit towards every light (device buffers).
  fused     one rtk_accel_occluded_device call
  emulated  the same answers from rounds of rtk_accel_intersect_device(cull = 0) plus torch ops for the material look-up,
            the step through transmissive surfaces and the compaction of the pending set (one host synchronisation per
            round: the caller has to know how many queries are left)
Both are timed with device events after warm-up, alternating, RTK_TRACE_AUTO; the tool asserts that they give the same
bytes before it reports a time.  Prints one JSON line; --out also writes it to a file (profiles/occluded_bench.json).

    python tools/bench_occluded.py [--reps 15] [--warmup 3] [--out profiles/occluded_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (code_hash: the hash bench.py stamps its results with)

SCENES = {"hw09/scene5": os.path.join(ROOT, "tests", "golden", "scenes", "hw09", "scene5.crtscene"),
          "hw11/scene8": os.path.join(ROOT, "tests", "golden", "scenes", "hw11", "scene8.crtscene")}
WIDTH, HEIGHT, BIAS = 1920, 1080, 1e-4


def shadow_queries(rtk, torch, acc, stream):
    """-> (rays [n,6], max_t [n]) on the device: one query per (camera hit, light), built as render.hpp:184-200 builds them."""
    cfg = rtk.RenderConfig(width=WIDTH, height=HEIGHT)
    n = WIDTH * HEIGHT
    cam = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    acc.camera_rays_device(cfg, cam.data_ptr(), 0, stream.cuda_stream)
    acc.intersect_device(cam.data_ptr(), n, True, hits.data_ptr(), rtk.TRACE_AUTO, stream.cuda_stream)
    stream.synchronize()
    hit = hits.view(torch.int32)[:, 4] != -1
    P = (cam[:, :3] + hits[:, :1] * cam[:, 3:])[hit]
    lights = torch.from_numpy(acc.scene.arrays()["light_pos"]).cuda()
    rays, max_t = [], []
    for k in range(lights.shape[0]):
        ld = lights[k][None, :] - P
        radius = torch.sqrt((ld * ld).sum(dim=1))
        ld = ld / radius[:, None]
        rays.append(torch.cat([P + BIAS * ld, ld], dim=1))
        max_t.append(radius)
    return torch.cat(rays).contiguous(), torch.cat(max_t).contiguous()


class Emulation:
    """is_occluded's loop on the caller's side of rtk_accel_intersect_device."""

    def __init__(self, rtk, torch, acc, stream):
        self.rtk, self.torch, self.acc, self.stream = rtk, torch, acc, stream
        a = acc.scene.arrays()
        self.mesh_refractive = torch.from_numpy(a["mat_kind"][a["mesh_material"]] == rtk.MAT_REFRACTIVE).cuda()
        self.rounds = 0
        self.lane_rounds = self.busy_lane_rounds = 0

    def run(self, rays, max_t, out, tally=False):
        torch, rtk = self.torch, self.rtk
        o, d, mt = rays[:, :3].clone(), rays[:, 3:].contiguous(), max_t.clone()
        out.zero_()
        idx = torch.nonzero(0.0 < mt).flatten()
        hits = torch.empty((rays.shape[0], 8), dtype=torch.float32, device="cuda")
        self.rounds = 0
        while idx.numel() > 0:                                                 # (a host synchronisation)
            if self.rounds == rtk.OCCLUDED_MAX_STEPS:                          # the kernel's bound on the reference's loop
                out[idx] = rtk.OCC_STEP_LIMIT
                break
            if tally:                                                          # what the fused kernel's waves do this round
                self.lane_rounds += 64 * int(torch.unique(idx // 64).numel())
                self.busy_lane_rounds += int(idx.numel())
            r = torch.cat([o[idx], d[idx]], dim=1).contiguous()
            self.acc.intersect_device(r.data_ptr(), r.shape[0], False, hits.data_ptr(), rtk.TRACE_AUTO, self.stream.cuda_stream)
            h = hits[: r.shape[0]]
            t, mesh = h[:, 0], h.view(torch.int32)[:, 4]
            clear = (mesh == -1) | (mt[idx] < t)
            through = ~clear & self.mesh_refractive[mesh.clamp(min=0).long()]
            done = ~through
            out[idx[done]] = torch.where(clear[done], 0, 1).to(torch.uint8)
            s, ts = idx[through], t[through]
            o[s] = (o[s] + ts[:, None] * d[s]) + BIAS * d[s]
            mt[s] = mt[s] - ts
            idx = s[0.0 < mt[s]]
            self.rounds += 1


def timed(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    stream.synchronize()
    return a.elapsed_time(b)


def spread(ms, n):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "queries_per_s": round(n / (med * 1e-3))}


def measure(rtk, torch, acc, stream, rays, max_t, args):
    n = rays.shape[0]
    fused_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    emu_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    emu = Emulation(rtk, torch, acc, stream)

    def fused():
        acc.occluded_device(rays.data_ptr(), max_t.data_ptr(), n, fused_out.data_ptr(), BIAS, rtk.TRACE_AUTO, stream.cuda_stream)

    def emulated():
        emu.run(rays, max_t, emu_out)

    fused()
    emu.run(rays, max_t, emu_out, tally=True)
    stream.synchronize()
    assert torch.equal(fused_out, emu_out), "fused and emulated answers differ"
    for _ in range(args.warmup):
        fused()
        emulated()
    stream.synchronize()
    f_ms, e_ms = [], []
    for _ in range(args.reps):                                                 # alternating: both see the same machine
        f_ms.append(timed(torch, stream, fused))
        e_ms.append(timed(torch, stream, emulated))
    assert torch.equal(fused_out, emu_out), "fused and emulated answers differ"
    f, e = spread(f_ms, n), spread(e_ms, n)
    return {"queries": n, "occluded": int((fused_out == 1).sum()), "step_limit": int((fused_out == 2).sum()), "rounds": emu.rounds,
            "idle_lane_round_share": round(1.0 - emu.busy_lane_rounds / max(emu.lane_rounds, 1), 4),
            "fused": f, "emulated": e, "emulated_over_fused": round(e["ms_median"] / f["ms_median"], 3)}


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
        raise SystemExit("bench_occluded needs a HIP device: the rtk engine has no CPU path")
    stream = torch.cuda.Stream()
    result = {"tool": "bench_occluded", "code_hash": bench.code_hash(), "width": WIDTH, "height": HEIGHT, "shadow_bias": BIAS,
              "trace_mode": "auto", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "scenes": {}}
    with torch.cuda.stream(stream):
        for name, path in SCENES.items():
            acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
            rays, max_t = shadow_queries(rtk, torch, acc, stream)
            n = rays.shape[0]
            fused_out = torch.empty(n, dtype=torch.uint8, device="cuda")

            def fused():
                acc.occluded_device(rays.data_ptr(), max_t.data_ptr(), n, fused_out.data_ptr(), BIAS, rtk.TRACE_AUTO, stream.cuda_stream)

            fused()
            stream.synchronize()
            result["scenes"][name] = measure(rtk, torch, acc, stream, rays, max_t, args)
            limit = fused_out == rtk.OCC_STEP_LIMIT
            if bool(limit.any()):
                # queries the reference itself would still be stepping after RTK_OCCLUDED_MAX_STEPS hits keep one lane (fused) or one
                # round trip per step (emulated) busy to the limit: the same workload without them, for the cost of the rest
                if os.environ.get("BENCH_OCCLUDED_TRACE"):
                    for q in torch.nonzero(limit).flatten().tolist():
                        print(f"step limit: query {q} ray {[float.hex(x) for x in rays[q].tolist()]} max_t {float.hex(float(max_t[q]))}", file=sys.stderr)
                keep = ~limit
                result["scenes"][name + " without the queries at the step limit"] = measure(
                    rtk, torch, acc, stream, rays[keep].contiguous(), max_t[keep].contiguous(), args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
