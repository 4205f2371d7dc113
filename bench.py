#!/usr/bin/env python3
"""Headline benchmark: Mrays/s and frame ms of hw09/scene5 (dragon) 1920x1080 1spp (BASELINE config 2).

One "step" = one full frame through the hot path (primary + shadow + reflection rays, shading device-side).
`python bench.py --gpus N --steps K --warmup W`; for N>1 the driver launches it under torch.distributed.run,
one rank per GPU: buckets are dealt round-robin to ranks, each rank renders its buckets, the bucket buffers
are all-gathered over RCCL/xGMI and assembled into the frame on every rank (part of the timed step).

Prints ONE JSON line on rank 0 with the driver's contract.  A plain run sets up, warms up, times the K steps and prints it;
`--dump-outputs DIR` writes the frame of the last timed step and its ray counters to DIR/*.npy.  With `--full` the line also
carries `roofline`, `cpu_baseline`, `verified` (the timed frame compared bit for bit with the CPU oracle's) and -- outside the
timed headline -- `first_frame_ms`, `critical_path_ms` and `extras`: the fixed 2^24-ray synthetic workload of SURVEY 8(d) (at
any N: sharded by contiguous ray ranges, hits all-gathered over RCCL) and, at N = 1, BASELINE configs 3, 4 and 5 at their real
frame sizes.

The headline `ms_per_step` is the STEADY STATE of a repeated frame: from the second frame of a shape on, the pixel blocks
are started most-expensive-first using the cycle counts the previous frame reported (every block is rendered in full every
frame; only the launch order changes).  `first_frame_ms` is the same frame on a fresh accelerator, without that order --
what a one-shot CLI render pays.
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SCENE = os.path.join(SCENES, "hw09", "scene5.crtscene")
WIDTH, HEIGHT, SPP, DEPTH, DIFFUSE = 1920, 1080, 1, 5, 0
HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
# VALU issue peak: 1024 SIMDs, one wave64 VALU instruction per 2 cycles each (MI355X_MICROARCH.md "Wave scheduling"), 2.4 GHz
N_SIMDS, CLOCK_GHZ, CYCLES_PER_WAVE_VALU = 1024, 2.4, 2
VALU_PEAK_GINSTR = N_SIMDS * CLOCK_GHZ / CYCLES_PER_WAVE_VALU
TRACE_NAMES = {0: "auto", 1: "lane", 2: "wave", 3: "group4", 4: "group8", 5: "group16", 6: "stream", 7: "twopass", 8: "repack"}


def code_hash() -> str:
    """Hash of the device code the profiles describe: every kernel source and the build flags."""
    import hashlib

    h = hashlib.sha256()
    base = os.path.join(ROOT, "simd-raytracer_amd")
    for rel in sorted(glob.glob(os.path.join(base, "csrc", "*.hip")) + glob.glob(os.path.join(base, "csrc", "*.hpp")) + [os.path.join(base, "Makefile")]):
        h.update(os.path.basename(rel).encode())
        h.update(open(rel, "rb").read())
    return h.hexdigest()[:16]


def profile_meta(tag: str) -> dict:
    """profiles/<tag>_meta.json (tools/summarize_profile.py): the code hash and git head the PMC passes were taken at."""
    path = os.path.join(ROOT, "profiles", tag + "_meta.json")
    try:
        return json.load(open(path))
    except (OSError, ValueError):
        return {}


def committed_profile():
    """Per-launch PMC means of k_render from the newest committed rocprofv3 passes (profiles/r*_pmc_means.csv +
    *_traffic.json, written by tools/profile_bench.sh + tools/summarize_profile.py from separate --pmc runs of this command)."""
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_means.csv"))):
        try:
            rows = list(csv.DictReader(open(path)))
        except OSError:
            continue
        vals = {r["counter"]: float(r["mean_per_launch"]) for r in rows if "k_render" in r.get("kernel", "")}
        if "SQ_INSTS_VALU" in vals:
            tag = os.path.basename(path)[: -len("_pmc_means.csv")]
            traffic = None
            tpath = os.path.join(ROOT, "profiles", tag + "_traffic.json")
            if os.path.exists(tpath):
                try:
                    traffic = json.load(open(tpath))
                except ValueError:
                    traffic = None
            meta = profile_meta(tag)
            best = {"tag": tag, "counters": vals, "traffic": traffic, "path": os.path.relpath(path, ROOT), "meta": meta,
                    "current": bool(meta) and meta.get("code_hash") == code_hash()}
    return best


def workload_profile(name: str):
    """Per-frame (or per-launch) PMC sums of one `extras` workload from the newest committed profiles/r*_workloads.json
    (tools/profile_workloads.py under rocprofv3, summarised by tools/summarize_profile.py)."""
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_workloads.json")), reverse=True):
        try:
            doc = json.load(open(path))
        except (OSError, ValueError):
            continue
        if name in doc.get("workloads", {}):
            w = dict(doc["workloads"][name])
            w["source"] = os.path.relpath(path, ROOT)
            w["current"] = doc.get("code_hash") == code_hash()
            w["git_head"] = doc.get("git_head")
            return w
    return None


def frame_roofline(name: str, ms: float):
    """VALU-issue fraction, wait share and HBM traffic of one extras frame: committed counters / live time."""
    w = workload_profile(name)
    if not w or ms <= 0:
        return None
    c = w["per_unit"]
    valu = c.get("SQ_INSTS_VALU")
    hbm = (c["FETCH_SIZE"] * 1024 * 2 + c["WRITE_SIZE"] * 1024) if ("FETCH_SIZE" in c and "WRITE_SIZE" in c) else None
    ok = w["current"]
    return {
        "bound": "valu_issue", "unit": "G wave-instr/s", "peak": VALU_PEAK_GINSTR,
        "achieved": (valu / (ms * 1e-3) / 1e9) if (valu and ok) else None,
        "frac": (valu / (ms * 1e-3) / 1e9 / VALU_PEAK_GINSTR) if (valu and ok) else None,
        "valu_instructions": valu,
        "wait_share": (c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"]) if c.get("SQ_WAVE_CYCLES") else None,
        "traffic": hbm, "hbm_frac": (hbm / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if (hbm and ok) else None,
        "kernel_launches": w.get("launches_per_unit"),
        "counters_source": w["source"], "profile_matches_code": ok, "profile_git_head": w.get("git_head"),
    }


def algorithmic_bytes(c: dict) -> int:
    """B = 32 B per node popped + 36 B per triangle tested + 32 B ray in + 32 B hit out, summed over rays."""
    return 32 * c["nodes"] + 36 * c["tris"] + 64 * c["rays"]


def cpu_baseline(seconds: float) -> dict:
    """The CPU restatement (oracle, 'port') of kd_tree_simd_accel + render loop on this host's cores:
    SIMD packets at the host's native width, bucket tiles over all hardware threads, fp-contract on (README.md:37-39)."""
    import oracle

    oracle.build()
    w = oracle.native_width()
    acc = oracle.Accel(oracle.Scene(oracle.load_crtscene(SCENE), fast=True), oracle.ACCEL_KD_SIMD, W=w)
    acc.render(WIDTH, HEIGHT, SPP, DEPTH, DIFFUSE, count_work=False)  # warm-up (page faults, thread start)
    times, rays = [], 0
    t_end = time.time() + seconds
    while time.time() < t_end or len(times) < 3:
        t0 = time.perf_counter()
        _, cn = acc.render(WIDTH, HEIGHT, SPP, DEPTH, DIFFUSE, count_work=False)   # rays/hits only: no per-triangle tallies
        times.append(time.perf_counter() - t0)
        rays = cn["rays"]
    best = min(times)
    cores = os.cpu_count() or 1
    return {
        "value": rays / best / 1e6, "unit": "Mrays/s", "cores": cores, "kind": "port",
        "sample": f"{len(times)} full frames of the same workload ({rays} rays each), best frame {best * 1e3:.1f} ms, "
                  f"median {sorted(times)[len(times) // 2] * 1e3:.1f} ms, W={w} packets, {cores} threads; in the 8-vCPU build "
                  f"container the port needs 78-86 ms per frame where SURVEY 6 measured the reference at 69-75 ms (the port is "
                  f"10-20 % slower: C with GCC vector extensions and a per-frame pthread pool against the reference's clang -O3 "
                  f"std::experimental::simd + jthreads), so gpu_over_cpu is flattered by up to that much",
        "frame_ms": best * 1e3,
    }


def dump_outputs(path: str, frame, counters: dict) -> None:
    """--dump-outputs: what a caller of the timed path receives from its last step -- the frame (float32 [h, w, 3], 24.9 MB at
    1920x1080) and the frame's counters (float64, in the order of rtk.Counters: rays, primary, hits, ...)."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "frame.npy"), np.ascontiguousarray(frame, dtype=np.float32))
    np.save(os.path.join(path, "counters.npy"), np.array(list(counters.values()), dtype=np.float64))


def event_ms(torch, stream, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(n):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def synthetic_rays(rtk, torch, stream, n: int):
    """SURVEY 8(d)'s three fixed ray sets on scene5 (the same on every rank: fixed seeds)."""
    import numpy as np

    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE))
    cfg = rtk.RenderConfig(width=WIDTH, height=HEIGHT)
    cam = torch.empty((HEIGHT * WIDTH, 6), dtype=torch.float32, device="cuda")
    acc.camera_rays_device(cfg, cam.data_ptr(), 0, stream.cuda_stream)        # the 1920x1080 pixel-centre rays, row-major
    reps = -(-n // cam.shape[0])
    coherent = cam.repeat(reps, 1)[:n].contiguous()
    g = torch.Generator(device="cpu"); g.manual_seed(42)
    shuffled = coherent[torch.randperm(n, generator=g).cuda()].contiguous()
    rng = np.random.default_rng(43)
    o = rng.uniform([-15, -5, -15], [15, 8.82, 15], size=(n, 3)).astype(np.float32)
    v = rng.normal(size=(n, 3)).astype(np.float32); v /= np.linalg.norm(v, axis=1, keepdims=True)
    secondary = torch.from_numpy(np.concatenate([o, v], axis=1).astype(np.float32)).cuda()
    return acc, (("coherent_primary", coherent, True), ("shuffled_primary", shuffled, True), ("uniform_secondary", secondary, False))


def synthetic_extras(rtk, torch, dist, stream, rank: int, world: int) -> dict:
    """N = 2^24 rays through rtk_accel_intersect_device on scene5's tree.  At world > 1 the batch is cut into
    contiguous ray ranges, one per rank, and the 32-byte hits are all-gathered over RCCL inside the timed region; the time of a
    launch is the slowest rank's.  The path has no other exchange step: rays are independent."""
    par = importlib.import_module("simd-raytracer_amd.parallel")
    n = 1 << 24
    acc, sets = synthetic_rays(rtk, torch, stream, n)
    lo, hi = par.ray_range(n, rank, world)
    m = hi - lo
    hits = torch.empty((n, 32), dtype=torch.uint8, device="cuda")            # the gathered result (rank order == ray order)
    mine = hits[lo:hi] if world == 1 else torch.empty((m, 32), dtype=torch.uint8, device="cuda")
    synth = {}
    for name, rays, cull in sets:
        part = rays[lo:hi]
        cn = acc.intersect_stats(part.data_ptr(), m, cull, mine.data_ptr(), 2)
        best = None
        for mode in (2, 0, 8):      # (0 = auto repacks by itself when its probe finds the batch incoherent; the sort is inside the timed call)
            def launch():
                acc.intersect_device(part.data_ptr(), m, cull, mine.data_ptr(), mode, stream.cuda_stream)
                if world > 1:
                    par.gather_hits(mine, n, rank, world, out=hits)
            for _ in range(5):                                                 # 5 warm-up + 20 timed launches, median
                launch()
            times = sorted(event_ms(torch, stream, launch, 1) for _ in range(20))
            ms = 0.5 * (times[9] + times[10])
            fastest = times[0]
            if world > 1:
                t = torch.tensor([ms], dtype=torch.float64, device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                ms = float(t[0])
            if best is None or ms < best[0]:
                best = (ms, TRACE_NAMES[mode], fastest)
        tot = torch.tensor([float(cn["nodes"]), float(cn["tris"]), float(cn["hits"])], dtype=torch.float64, device="cuda")
        if world > 1:
            dist.all_reduce(tot)
        nodes, tris, nhit = (float(x) for x in tot)
        b_alg = 32 * nodes + 36 * tris + 64 * n
        hbm_gbps = 56.0 * n / best[0] / 1e6                                   # 24 B ray in + 32 B hit out, each moved once
        synth[name] = {"ms": best[0], "ms_fastest_launch": best[2], "Mrays_s": n / best[0] / 1e3, "mode": best[1], "hit_fraction": nhit / n,
                       "nodes_per_ray": nodes / n, "tris_per_ray": tris / n, "algorithmic_GBps": b_alg / best[0] / 1e6,
                       "hbm_GBps": hbm_gbps, "hbm_frac": hbm_gbps / HBM_PEAK_GBPS}
        if world == 1:
            r = frame_roofline("synthetic_" + name, best[0])
            if r:
                synth[name]["roofline"] = r
    return {"workload": "SURVEY 8(d): 2^24 rays on scene5's tree through rtk_accel_intersect_device; coherent = the 1920x1080 camera rays tiled, "
                        "shuffled = the same set permuted (seed 42), uniform_secondary = origins uniform in the scene box, directions uniform on "
                        "the sphere (seed 43); 5 warm-up + 20 timed launches, MEDIAN (ms_fastest_launch beside it), the faster of the wave, auto and repack strategies (repack: the rays sorted by "
                        "origin / direction cell first, the sort inside the timed call).  hbm_GBps = 56 B per ray (24 B ray in + 32 B hit out) / ms, "
                        "hbm_frac against 8 TB/s: the bytes this path has to move, the tree itself is cache resident"
                        + (f"; {world} ranks: contiguous ray ranges, the hits all-gathered over RCCL inside the timed region, slowest rank's time" if world > 1 else ""),
            "n_gpus": world, **synth}


def fast_traversal_extras(rtk, torch, stream, parity_frame) -> dict:
    """RTK_TRAVERSAL_FAST (front-to-back leaf order, rtk.h) beside the parity mode: NOT the headline -- ties between triangles hit at
    exactly the same distance may resolve differently, so a few pixels differ.  Config 2 and config 3, steady state."""
    import numpy as np

    out = {"what": "RTK_TRAVERSAL_FAST: leaves front to back per direction octant; same closest distance for every ray, ties may pick "
                   "another triangle; occlusion through transmissive surfaces as one any-hit query against the opaque triangles; off by "
                   "default (include/rtk.h)"}
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE), traversal=rtk.TRAVERSAL_FAST)
    cfg = rtk.RenderConfig(width=WIDTH, height=HEIGHT, spp=SPP, max_ray_depth=DEPTH, diffuse_rays=DIFFUSE)
    buf = torch.empty((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda")
    for _ in range(20):
        acc.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream)
    ms = event_ms(torch, stream, lambda: acc.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream), 50)
    rays = acc.last_counters()["rays"]
    diff = (buf != parity_frame).any(dim=2)
    q = lambda t: (255.999 * t.clamp(0, 1).double()).to(torch.uint8)
    out["config2"] = {"ms": ms, "Mrays_s": rays / ms / 1e3, "rays": rays, "pixels_differing_from_parity_frame": int(diff.sum()),
                      "pixels_differing_in_8_bit": int((q(buf) != q(parity_frame)).any(dim=2).sum()),
                      "max_abs_diff": float((buf - parity_frame).abs().max())}
    scene8 = os.path.join(SCENES, "hw11", "scene8.crtscene")
    res = {}
    for name, trav in (("parity", rtk.TRAVERSAL_REFERENCE), ("fast", rtk.TRAVERSAL_FAST)):
        a = rtk.KdTreeSimdAccel(rtk.parse_scene_file(scene8), traversal=trav)
        c = rtk.RenderConfig(width=1920, height=1080, spp=4, max_ray_depth=10, trace_mode=6)      # the streaming pipeline (what AUTO settles on)
        b = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
        for _ in range(3):
            a.render_frame_device(c, b.data_ptr(), stream.cuda_stream)
        m = min(event_ms(torch, stream, lambda: a.render_frame_device(c, b.data_ptr(), stream.cuda_stream), 1) for _ in range(3))
        res[name] = (m, a.last_counters()["rays"], b)
    # (the fast mode answers an occlusion query through the transmissive dragon with one any-hit query against the opaque triangles
    # instead of the reference's loop of closest hits, rtk.h: it launches fewer rays for the same frame; Mrays_s counts the PARITY
    # mode's rays -- the reference's intersect invocations for this frame -- over the fast mode's time)
    out["config3"] = {"ms": res["fast"][0], "Mrays_s": res["parity"][1] / res["fast"][0] / 1e3, "rays_counted_by_the_reference": res["parity"][1],
                      "rays_traced": res["fast"][1], "parity_ms": res["parity"][0],
                      "pixels_differing_from_parity_frame": int((res["fast"][2] != res["parity"][2]).any(dim=2).sum()),
                      "pixels_differing_in_8_bit": int((q(res["fast"][2]) != q(res["parity"][2])).any(dim=2).sum())}
    # The reference's accelerator takes its tree depth as a template parameter (kd_tree_simd_accel<F, eps, max_depth = 8, max_leaf_size = 64>,
    # kd_tree_simd.hpp:63-67); its CLI -- and therefore BASELINE's configs and the headline above -- instantiates the defaults.  Config 2 on
    # the same reference algorithm with max_depth = 10, for information (NOT the headline: another instantiation).
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE), max_depth=10)
    for _ in range(20):
        acc.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream)
    ms = event_ms(torch, stream, lambda: acc.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream), 50)
    out["config2_reference_tree_max_depth_10"] = {
        "ms": ms, "Mrays_s": acc.last_counters()["rays"] / ms / 1e3, "rays": acc.last_counters()["rays"],
        "pixels_differing_from_parity_frame": int((buf != parity_frame).any(dim=2).sum()),
        "what": "kd_tree_simd_accel<F, eps, 10, 64> in the parity traversal: bit-exact for that instantiation of the reference (deeper trees are "
                "slower here -- the leaf-list walk is linear in the leaves: tools/tree_params_experiment.py)"}
    return out


def frame_extras(rtk, torch, stream) -> dict:
    """BASELINE configs 3, 4 and 5 at their real frame sizes (N = 1; RTK_TRACE_AUTO picks the engine on the first frames)."""
    frames = {}

    def timed_passes(a, kw, passes, reps):
        c = [rtk.RenderConfig(**kw, sample_begin=b, sample_count=n) if n else rtk.RenderConfig(**kw) for b, n in passes]
        buf = torch.empty((a.output_floats(c[0]),), dtype=torch.float32, device="cuda")
        rays = [0]

        def run():
            rays[0] = 0
            for cfg in c:
                a.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream)
                rays[0] += 0 if len(c) == 1 else a.last_counters()["rays"]
        for _ in range(reps[0]):
            run()
        ms = min(event_ms(torch, stream, run, 1) for _ in range(reps[1]))
        if len(c) == 1:
            rays[0] = a.last_counters()["rays"]
        return ms, rays[0]

    scene8 = os.path.join(SCENES, "hw11", "scene8.crtscene")
    scene2 = os.path.join(SCENES, "hw15", "scene2.crtscene")
    # (largest queues first: config 5's, which config 4 then fits into -- a workspace that is freed and allocated again larger in
    # the same process came out 20 % slower, the same kernels on the same rays: gpurun_out/r03d-f, one process per case vs one for all)
    # config 5's frame: 3840x2160, depth 10, one diffuse ray, spp = 512 in the RNG keys; 16 of the 512 samples are timed (two
    # passes of 8); the other 31 pairs of passes do the same work on other samples
    a = rtk.KdTreeSimdAccel(rtk.parse_scene_file(scene2))
    kw = dict(width=3840, height=2160, spp=512, max_ray_depth=10, diffuse_rays=1)
    ms, rays = timed_passes(a, kw, [(0, 8), (8, 8)], (1, 2))
    frames["config5_scene2_3840x2160_spp512_depth10_gi1"] = {
        "ms": ms, "rays": rays, "Mrays_s": rays / ms / 1e3, "spp_timed": 16, "passes": "2 x 8 of the 512 samples",
        "full_frame_ms_extrapolated": ms * 32, "roofline": frame_roofline("config5", ms / 2)}
    # config 4 as quoted: 1920x1920 (the scene's own size and bucket 24), 128 spp in 8 passes of 16 (progressive accumulation)
    kw = dict(spp=128, max_ray_depth=5, diffuse_rays=1)
    ms, rays = timed_passes(a, kw, [(16 * k, 16) for k in range(8)], (1, 1))
    frames["config4_scene2_1920x1920_spp128_depth5_gi1"] = {"ms": ms, "rays": rays, "Mrays_s": rays / ms / 1e3, "spp_timed": 128,
                                                            "passes": "8 x 16 samples", "roofline": frame_roofline("config4", ms / 8)}
    del a
    # config 3 as quoted
    a = rtk.KdTreeSimdAccel(rtk.parse_scene_file(scene8))
    ms, rays = timed_passes(a, dict(width=1920, height=1080, spp=4, max_ray_depth=10), [(0, 0)], (5, 3))
    frames["config3_scene8_1080p_spp4_depth10"] = {"ms": ms, "rays": rays, "Mrays_s": rays / ms / 1e3, "spp_timed": 4,
                                                   "roofline": frame_roofline("config3", ms)}
    return frames


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace-mode", type=int, default=0, choices=[0, 1, 2, 3, 4, 5, 6, 7])
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the untimed extra workloads (synthetic 2^24 rays, configs 3-5)")
    ap.add_argument("--no-verify", action="store_true", help="skip the comparison of the timed frame with the CPU oracle's")
    ap.add_argument("--pipeline-depth", type=int, default=2, help="N>1: frames in flight (1 = render, gather, assemble back to back)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what lies beside the headline: first-frame times, per-ray work counters and the roofline, the "
                         "check of the timed frame against the CPU oracle, the extra workloads and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR: frame.npy (float32 [h, w, 3]) and counters.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch
    import torch.distributed as dist

    import __graft_entry__ as ge

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    torch.cuda.set_device(local_rank)
    # RTK_BENCH_FORCE_DIST=1 runs the sharded code path (RCCL group, gather pipeline, assemble) at world size 1 too,
    # which is how it is rehearsed on a one-GPU box
    use_dist = world > 1 or (os.environ.get("RTK_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if rank == 0:
        ge.build()                      # a no-op when the in-tree libraries are current (they travel with the snapshot)
    if use_dist:
        dist.barrier()                  # nobody loads librtk_hip.so while rank 0 might still be writing it
    rtk = importlib.import_module("simd-raytracer_amd")

    stream = torch.cuda.current_stream()
    cfg = rtk.RenderConfig(width=WIDTH, height=HEIGHT, spp=SPP, max_ray_depth=DEPTH, diffuse_rays=DIFFUSE,
                           trace_mode=args.trace_mode, rank=rank, world_size=world)
    frame = torch.empty((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda")

    # ---- untimed: the first frame of a shape on a fresh accelerator (no cost-feedback order yet)
    first_frame_ms = None
    if world == 1 and args.full:
        cold = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE), device=local_rank)
        # context, uploads, code load: a small frame through the kernel the timed frame will use (a 64x64 frame would pick the
        # 8-wave kernel by itself, and the first launch of a kernel pays for loading its code)
        cold.render_frame_device(rtk.RenderConfig(width=64, height=64, trace_mode=3 if args.trace_mode == 0 else args.trace_mode),
                                 frame.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        first_frame_ms = event_ms(torch, stream, lambda: cold.render_frame_device(cfg, frame.data_ptr(), stream.cuda_stream), 1)
        del cold

    accel = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE), device=local_rank)
    n_local = accel.output_floats(cfg)
    local = frame.view(-1) if world == 1 else torch.empty((n_local,), dtype=torch.float32, device="cuda")
    pipe = None
    if use_dist:
        # sharded frames: render(k+1) overlaps all_gather(k) (parallel.FramePipeline); every frame is still rendered,
        # gathered and assembled on every rank, and the pipeline is drained inside the timed region
        par = importlib.import_module("simd-raytracer_amd.parallel")
        layout = par.BucketLayout(WIDTH, HEIGHT, accel.scene.info.bucket_size, world)
        if world > 1:
            assert layout.floats_per_rank == n_local, (layout.floats_per_rank, n_local)

            def assemble(g, f):
                accel.assemble_device(cfg, g.data_ptr(), f.data_ptr(), stream.cuda_stream)
        else:                                                   # one-GPU rehearsal: a world-1 frame is not bucket-compacted

            def assemble(g, f):
                f.view(-1).copy_(g)
        timed = []                                              # HIP event pairs around the render launches

        def render(buf, k):
            if timed is not None and recording[0]:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                accel.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream)
                b.record(stream)
                timed.append((a, b))
            else:
                accel.render_frame_device(cfg, buf.data_ptr(), stream.cuda_stream)

        recording = [False]
        pipe = par.FramePipeline(layout, accel, cfg, depth=args.pipeline_depth, render=render, assemble=assemble,
                                 floats_per_rank=n_local)

    def step() -> None:
        if pipe is None:
            accel.render_frame_device(cfg, local.data_ptr(), stream.cuda_stream)
        else:
            pipe.submit()

    # ---- untimed: per-ray work counters of this rank's share (for the algorithmic-byte figure).
    # collect_stats=2 counts what the timed kernel actually visits (its occlusion queries stop at the first answering hit);
    # collect_stats=1 counts what the reference algorithm visits for the same frame (every ray traced to the end).
    # A plain run renders one untimed frame in their place: the kernel's code is loaded and the block order has its first cycle
    # counts, as after the counting frames (the cost feedback does not tell them apart).
    if args.full:
        stats_cfg = rtk.RenderConfig(**{**cfg.__dict__, "collect_stats": 1})
        accel.render_frame_device(stats_cfg, local.data_ptr(), stream.cuda_stream)
        work_reference = accel.last_counters()
        stats_cfg = rtk.RenderConfig(**{**cfg.__dict__, "collect_stats": 2})
        accel.render_frame_device(stats_cfg, local.data_ptr(), stream.cuda_stream)
        work = accel.last_counters()
    else:
        accel.render_frame_device(cfg, local.data_ptr(), stream.cuda_stream)

    for _ in range(args.warmup):
        step()
    if pipe is not None:
        pipe.drain()
    torch.cuda.synchronize()

    # ---- timed region: exactly K steps between barrier + synchronize on both sides
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if pipe is None:
        for k in range(args.steps):
            ev[k][0].record(stream)           # HIP events on the stream the render kernel is launched on
            accel.render_frame_device(cfg, local.data_ptr(), stream.cuda_stream)
            ev[k][1].record(stream)
    else:
        recording[0] = True
        for k in range(args.steps):
            pipe.submit()
        pipe.drain()                          # the last frames are gathered and assembled inside the timed region
        ev = timed
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # ---- the frame that was just timed (rank 0; for N > 1 the assembled frame), copied out before anything renders into it again
    timed_frame = None
    if rank == 0 and (args.dump_outputs or (args.full and not args.no_verify)):
        timed_frame = (frame if pipe is None else pipe.last_frame()).detach().cpu().numpy()
    counters = accel.last_counters()           # of the last timed step (this rank's share)

    # ---- checked: bit for bit the CPU oracle's frame
    verified, verify_note = None, None
    if rank == 0 and args.full and not args.no_verify:
        import numpy as np
        import oracle

        oacc = oracle.Accel(oracle.Scene(oracle.load_crtscene(SCENE)), oracle.ACCEL_KD_SIMD)
        ref, ocn = oacc.render(WIDTH, HEIGHT, SPP, DEPTH, DIFFUSE, count_work=False)
        same = bool(np.array_equal(timed_frame.view(np.uint32), ref.view(np.uint32)))
        verified = same
        verify_note = (f"frame of the last timed step vs oracle/rt_oracle.c (kd_tree_simd_accel restatement, fp-contract off; itself pinned to the "
                       f"reference's own renders by tests/test_reference_outputs.py): {'all' if same else 'NOT all'} {ref.size} floats bit-equal, "
                       f"oracle ray count {ocn['rays']}")

    kernel_ms = sum(a.elapsed_time(b) for a, b in ev) / max(args.steps, 1)
    critical_ms = accel.last_critical_path_ms() if args.full else 0.0
    names = list(counters)
    tot = torch.tensor([float(elapsed), float(kernel_ms), float(critical_ms)] + [float(counters[n]) for n in names],
                       dtype=torch.float64, device="cuda")
    if use_dist:
        mx = tot.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = tot.clone()
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        elapsed, kernel_ms, critical_ms = float(mx[0]), float(mx[1]), float(mx[2])
        tot = sm
    frame_counters = {n: float(tot[3 + i]) for i, n in enumerate(names)}      # the whole frame's, summed over ranks
    rays_total = frame_counters["rays"]
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, timed_frame, frame_counters)

    if verified is not None and world == 1:
        verified = verified and (int(rays_total) == ocn["rays"])
    # the same first-frame measurement on another fresh accelerator, now that the timed loop has the GPU at its clocks: what of
    # first_frame_ms is launch order (no cost feedback yet) and what is a GPU woken from idle
    first_frame_busy_gpu_ms = None
    if world == 1 and args.full:
        cold = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE), device=local_rank)
        cold.render_frame_device(rtk.RenderConfig(width=64, height=64, trace_mode=3 if args.trace_mode == 0 else args.trace_mode),
                                 frame.data_ptr(), stream.cuda_stream)
        for _ in range(20):
            accel.render_frame_device(cfg, local.data_ptr(), stream.cuda_stream)
        first_frame_busy_gpu_ms = event_ms(torch, stream, lambda: cold.render_frame_device(cfg, frame.data_ptr(), stream.cuda_stream), 1)
        del cold
    extras_out = None
    if args.full and not args.no_extras:
        extras_out = {"synthetic_2p24": synthetic_extras(rtk, torch, dist, stream, rank, world)}      # every rank takes part
        if world == 1:
            extras_out["frames"] = frame_extras(rtk, torch, stream)
            extras_out["fast_traversal"] = fast_traversal_extras(rtk, torch, stream, frame)
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        out = {
            "metric": "Mrays/s (intersect invocations per second), hw09/scene5 dragon 1920x1080 1spp",
            "value": rays_total / (elapsed / args.steps) / 1e6,
            "unit": "Mrays/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "reference scene file scenes/hw09/scene5.crtscene (input data, copied under tests/golden/scenes); no weights",
            "config": {"workload": "BASELINE configs[1]: scenes/hw09/scene5.crtscene 1920x1080 1spp max_ray_depth=5 "
                                   "(primary + shadow + reflection rays), kd_tree_simd_accel semantics",
                       "rays_per_frame": int(rays_total), "primary_rays": WIDTH * HEIGHT * SPP,
                       "trace_mode": TRACE_NAMES[args.trace_mode] + (" (= group4 megakernel for this fork-free scene; group8 when a rank has < 9000 pixel blocks)" if args.trace_mode == 0 else ""),
                       "parallelism": f"bucket-tiles x{world}" + (f"; a pipelined SEQUENCE of frames: the RCCL all-gather of frame k overlaps the rendering of frame k+1 "
                                                                  f"({args.pipeline_depth} frames in flight), every frame is rendered, gathered and assembled on every rank and the "
                                                                  f"pipeline is drained inside the timed region" if pipe is not None else ""),
                       "headline": "steady state of a repeated frame (block launch order from the previous frame's cycle counts); see first_frame_ms (--full)"},
        }
        if args.full:
            # the dominant kernel is k_render; one launch processes this rank's share of the frame
            launch_bytes = algorithmic_bytes(work)
            prof = committed_profile() if world == 1 else None
            alg_gbps = launch_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
            valu = prof["counters"]["SQ_INSTS_VALU"] if prof else None
            traffic = (prof["traffic"] or {}).get("hbm_bytes_per_launch") if prof else None
            # the counters are only as good as the code they were taken from: a profile of other kernel sources gives no fraction
            fresh = bool(prof and prof["current"])
            achieved = valu / (kernel_ms * 1e-3) / 1e9 if (valu and kernel_ms > 0 and fresh) else None
            out.update({
                "first_frame_ms": first_frame_ms,
                "first_frame_busy_gpu_ms": first_frame_busy_gpu_ms,
                "critical_path_ms": critical_ms,
                "roofline": {
                    # HBM does not bound this kernel (the tree is < 0.6 MB and cache resident: `traffic` is ~1 % of what the chip could
                    # move in a frame time), MFMA does not apply (no contraction).  What bounds it is VALU instruction issue and, above
                    # that, the frame's longest dependent chain (`critical_path_ms`, one 8x8 pixel block).
                    "bound": "valu_issue",
                    "achieved": achieved, "peak": VALU_PEAK_GINSTR, "unit": "G wave-instr/s",
                    "frac": (achieved / VALU_PEAK_GINSTR) if achieved else None,
                    "traffic": traffic if fresh else None,
                    "profile_matches_code": fresh if prof else None,
                    "profile_git_head": (prof["meta"].get("git_head") if prof else None), "code_hash": code_hash(),
                    "kernel": "k_render", "kernel_ms": kernel_ms,
                    "valu_instructions_per_launch": valu,
                    "counters_source": (f"{prof['path']} (rocprofv3 --pmc passes of this command, mean per k_render launch); peak = {N_SIMDS} SIMDs x "
                                        f"{CLOCK_GHZ} GHz / {CYCLES_PER_WAVE_VALU} cycles per wave64 VALU instruction (the MI355X's wave scheduling)") if prof else None,
                    "critical_path_frac": (critical_ms / kernel_ms) if kernel_ms > 0 else None,
                    "hbm": {"traffic_GBps": (traffic / (kernel_ms * 1e-3) / 1e9) if (traffic and kernel_ms > 0 and fresh) else None,
                            "frac_of_8TBps": (traffic / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if (traffic and kernel_ms > 0 and fresh) else None},
                    "algorithmic": {
                        "note": "SURVEY 8(d) accounting, informational: 32 B/node popped + 36 B/triangle tested + 64 B ray+hit.  These are bytes the "
                                "algorithm REFERENCES, not bytes moved: one fetch serves a whole wave and the tree is cache resident, so the rate "
                                "exceeds the HBM peak and is not a roofline",
                        "bytes_per_launch": launch_bytes, "GBps": alg_gbps,
                        "bytes_per_ray": launch_bytes / max(work["rays"], 1),
                        "nodes_per_ray": work["nodes"] / max(work["rays"], 1), "tris_per_ray": work["tris"] / max(work["rays"], 1),
                        "reference_algorithm_bytes_per_launch": algorithmic_bytes(work_reference),
                        "reference_nodes_per_ray": work_reference["nodes"] / max(work_reference["rays"], 1),
                        "reference_tris_per_ray": work_reference["tris"] / max(work_reference["rays"], 1),
                    },
                },
            })
            out["verified"] = verified
            out["verified_how"] = verify_note
        if world > 1:
            out["config"]["scaling_note"] = ("tile sharding of THIS frame is bounded by its longest 8x8 pixel block (critical_path_ms): predicted ~1.3x "
                                             "at any N (profiles/r02_rank_times.json: slowest rank 0.207 / 0.202 / 0.164 / 0.157 ms at N = 1 / 2 / 4 / 8); "
                                             "frames whose blocks are small against the frame scale: config 5's shape 6.0x kernel-only at 8 ranks")
        if extras_out is not None:
            out["extras"] = extras_out
        if args.full and not args.no_cpu_baseline and world == 1:      # the CPU leg runs on rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(args.cpu_seconds)
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
        print(json.dumps(out))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
