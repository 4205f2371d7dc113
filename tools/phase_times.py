"""Diagnostic (-DRTK_DEBUG_PHASES build): where an owner wave's cycles go (node walk / small leaves / sliced leaves / shading).

    python tools/phase_times.py simd-raytracer_amd/build_dbg/librtk_hip_phases.so [trace_mode] [--width W --height H --frames N --dump FILE.npy]
"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one column per slot of `enum PhaseSlot` (csrc/phases.hip.hpp: PH_N_TRACE -> "n_trace"), in its order
SLOTS = ["total", "trace", "n_trace", "steps", "n_small", "t_small", "c_small", "n_big", "t_big", "c_big",
         "prologue", "to_first_trace", "first_trace", "after_first_trace", "chunks", "surv", "ctris", "rt0", "rt1", "wg", "wait",
         "tr0", "tr1", "tr2", "tr3", "tr4", "tr5", "kind0", "kind1", "kind2", "kind3", "kind4", "kind5", "c_bund", "c_list", "own",
         "stg_n", "stg_w1", "stg_l1", "stg_w2", "stg_l2", "stg_w3", "stg_l3", "stg_l4"]
COL = {name: i for i, name in enumerate(SLOTS)}


def measure(lib, mode, w, h, frames):
    """[blocks, len(SLOTS)] float64: the slots of every 8x8 pixel block of the last of `frames` frames of scene5"""
    import ctypes as C, importlib, numpy as np
    sys.path.insert(0, ROOT)
    import torch
    rtk = importlib.import_module("simd-raytracer_amd")
    dbg = C.CDLL(lib)
    dbg.rtk_render_frame.argtypes = rtk.lib().rtk_render_frame.argtypes
    dbg.rtk_scene_load_crtscene.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    dbg.rtk_accel_build.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    sc = C.c_void_p(); assert dbg.rtk_scene_load_crtscene(os.path.join(ROOT, "tests/golden/scenes/hw09/scene5.crtscene").encode(), C.byref(sc)) == 0
    ac = C.c_void_p(); assert dbg.rtk_accel_build(sc, None, C.byref(ac)) == 0
    world, rank = int(os.environ.get("TC_WORLD", "1")), int(os.environ.get("TC_RANK", "0"))
    p = rtk.RenderConfig(width=w, height=h, trace_mode=mode, rank=rank, world_size=world).to_c()
    cn = rtk.Counters()
    if world == 1:
        rgb = np.zeros((h, w, 3), np.float32)
        for _ in range(frames): assert dbg.rtk_render_frame(ac, C.byref(p), rgb.ctypes.data, C.byref(cn)) == 0
        # lane i of block (by, bx) wrote value i at pixel (by*8 + i//8, bx*8 + i%8)
        return rgb[:, :, 0].reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)[:, :len(SLOTS)].astype(np.float64)
    # one rank of a sharded frame: the compact [buckets_per_rank, B, B, 3] buffer; blocks keep their place inside a bucket
    B = int(os.environ.get("TC_BUCKET", "64"))
    dbg.rtk_render_output_floats.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    nf = C.c_size_t(); assert dbg.rtk_render_output_floats(ac, C.byref(p), C.byref(nf)) == 0
    dbg.rtk_render_frame_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    dbuf = torch.zeros(nf.value, dtype=torch.float32, device="cuda")
    for _ in range(frames):
        assert dbg.rtk_render_frame_device(ac, C.byref(p), dbuf.data_ptr(), None) == 0
        torch.cuda.synchronize()
    buf = dbuf.cpu().numpy()
    bpr = nf.value // (B * B * 3)
    r = buf.reshape(bpr, B, B, 3)[:, :, :, 0].reshape(bpr, B // 8, 8, B // 8, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 64)[:, :len(SLOTS)].astype(np.float64)
    r = r[r[:, COL["total"]] > 0]                            # (blocks of the padding buckets never ran)
    print(f"rank {rank} of {world}: {len(r)} blocks")
    return r


def report(r, w):
    import numpy as np
    col = lambda name, m=slice(None): r[m][:, COL[name]]
    def show(tag, m):
        d = dict(zip(SLOTS, r[m].sum(0))); n = m.sum()
        c_nodes = d["trace"] - d["c_small"] - d["c_big"]
        print(f"--- {tag}: {n} blocks, mean total {d['total']/n:.0f} cycles; trace {100*d['trace']/d['total']:.0f}% "
              f"(nodes {100*c_nodes/d['total']:.0f}%, small leaves {100*d['c_small']/d['total']:.0f}%, sliced leaves {100*d['c_big']/d['total']:.0f}%), rest {100*(1-d['trace']/d['total']):.0f}%")
        print(f"    per block: traces {d['n_trace']/n:.1f}, node steps {d['steps']/n:.0f} ({c_nodes/max(d['steps'],1):.0f} cyc/step), "
              f"small leaves {d['n_small']/n:.1f} with {d['t_small']/n:.0f} tris ({d['c_small']/max(d['t_small'],1):.0f} cyc/tri), "
              f"sliced leaves {d['n_big']/n:.1f} with {d['t_big']/n:.0f} tris ({d['c_big']/max(d['n_big'],1):.0f} cyc/leaf, {d['c_big']/max(d['t_big'],1):.0f} cyc/tri)")
        print(f"    of the total: waiting for the helpers of a light burst {100*d['wait']/d['total']:.0f}%, making bundles {100*d['c_bund']/d['total']:.0f}%, "
              f"culling the leaf list {100*d['c_list']/d['total']:.0f}%")
        if d["stg_n"] > 0:
            print(f"    owner's exact tests: {d['stg_n']/n:.0f} surviving triangles per block; the wave goes on after det + u estimate for {100*d['stg_w1']/d['stg_n']:.0f}% "
                  f"({d['stg_l1']/max(d['stg_w1'],1):.1f} lanes alive), after u for {100*d['stg_w2']/d['stg_n']:.0f}% ({d['stg_l2']/max(d['stg_w2'],1):.1f}), "
                  f"after v for {100*d['stg_w3']/d['stg_n']:.0f}% ({d['stg_l3']/max(d['stg_w3'],1):.1f}); "
                  f"{d['stg_l4']/d['stg_n']:.2f} accepted lanes per triangle")
        print(f"    owner's bundle culling per block: {d['chunks']/n:.1f} chunks, {d['ctris']/n:.0f} triangles in, {d['surv']/n:.1f} survivors ({100*d['surv']/max(d['ctris'],1):.1f}%)")
    tot = col("total")
    bg = (col("n_trace") == 1) & (col("n_small") + col("n_big") == 0)
    print("background blocks (one trace, no leaf):", bg.sum(), "mean cycles: prologue %.0f, ray setup until first trace %.0f, first trace %.0f, after it %.0f; total %.0f"
          % tuple(col(name, bg).mean() for name in ("prologue", "to_first_trace", "first_trace", "after_first_trace", "total")))
    show("all", tot >= 0)
    show("traced >1", col("n_trace") > 1)
    order = np.argsort(-tot)
    top = np.zeros(len(tot), bool); top[order[:100]] = True
    show("100 longest", top)
    top = np.zeros(len(tot), bool); top[order[:1000]] = True
    show("1000 longest", top)

    # ---- timeline (s_memrealtime, 100 MHz): when blocks start / end, how many owners are running
    t0 = col("rt0").copy(); t1 = col("rt1").copy()
    t1 = np.where(t1 < t0, t1 + 2**24, t1)
    base = np.median(t0)
    t0 = np.where(t0 < base - 2**23, t0 + 2**24, t0); t1 = np.where(t1 < base - 2**23, t1 + 2**24, t1)
    t1 -= t0.min(); t0 -= t0.min()
    start, end = t0 / 100.0, t1 / 100.0                      # microseconds
    n_trace, wg = col("n_trace"), col("wg")
    print("kernel span %.1f us; block durations us: mean %.1f p50 %.1f p90 %.1f p99 %.1f max %.1f" % (end.max(), (end - start).mean(), *np.percentile(end - start, [50, 90, 99]), (end - start).max()))
    ts = np.linspace(0, end.max(), 25)
    print("owners running over time:", [int(((start <= t) & (end > t)).sum()) for t in ts])
    last = np.argsort(-end)[:8]
    print("last to finish (end us, start us, duration us, traces, dispatch index):", [(round(float(end[i]), 1), round(float(start[i]), 1), round(float(end[i] - start[i]), 1), int(n_trace[i]), int(wg[i])) for i in last])
    longest = np.argsort(-(end - start))[:8]
    for i in np.argsort(-(end - start))[:6]:
        traces = [(r[i, COL[f"tr{k}"]], r[i, COL[f"kind{k}"]]) for k in range(6)]
        print("  block %d: %.1f us; burst wait %.1f us; traces (us, kind: 100+log2(parts) = light burst, else rays in the root box): %s" % (
            i, end[i] - start[i], r[i, COL["wait"]] / 2400.0, [(round(float(c) / 2400.0, 1), int(kind)) for c, kind in traces if c > 0]))
    print("longest (duration us, start us, traces, dispatch index, block y, block x):", [(round(float(end[i] - start[i]), 1), round(float(start[i]), 1), int(n_trace[i]), int(wg[i]), int(i // (w // 8)), int(i % (w // 8))) for i in longest])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib", help="the library of `make phases`")
    ap.add_argument("mode", nargs="?", type=int, default=3, help="trace_mode (default 3)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=3, help="frames rendered; the last one is reported")
    ap.add_argument("--dump", metavar="FILE.npy", help="also write the [blocks, slots] matrix")
    a = ap.parse_args()
    assert a.width % 8 == 0 and a.height % 8 == 0, "whole 8x8 pixel blocks"
    r = measure(a.lib, a.mode, a.width, a.height, a.frames)
    if a.dump:
        import numpy as np
        np.save(a.dump, r.astype(np.float32))                 # (what the kernel wrote: lossless)
    report(r, a.width)


if __name__ == "__main__":
    main()
