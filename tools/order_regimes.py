"""What separates a fast launch list from a slow one?  The benchmark's workload (scene5 1920x1080, depth 5) with the judge off and
the plain schedule (a new list every 16 frames, each one used whatever it scores), so that a process runs ten lists one after the
other.  The frames of a list are enqueued back to back between event pairs; at the first frame of each list the host waits once and
reads the list out (rtk_debug_order_lists).  Per list: the median frame time, the single and packed workgroups, where the 32
costliest blocks (the head of `order`) sit in the workgroup list, and those positions mod 8 (workgroups b and b + 8 share an XCD)
and mod 4 (the owner wave's SIMD is (wave + workgroup) % 4).  The lists are then split into fast and slow at 1.08 x the fastest
median and printed side by side.
usage: RTK_COST_JUDGE=0 RTK_COST_RESORT_MAX=0 python tools/order_regimes.py [lists, default 10]"""
import importlib, json, os, statistics, sys
os.environ.setdefault("RTK_COST_JUDGE", "0")
os.environ.setdefault("RTK_COST_RESORT_MAX", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
rtk = importlib.import_module("simd-raytracer_amd")
SCENE = os.path.join(ROOT, "tests/golden/scenes/hw09/scene5.crtscene")
LISTS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
st = torch.cuda.current_stream()
frame = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE))
cfg = rtk.RenderConfig(width=1920, height=1080, max_ray_depth=5)


def timed(n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(st); acc.render_frame_device(cfg, frame.data_ptr(), st.cuda_stream); b.record(st)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def describe(lists):
    order, hdr, wg_list = lists
    n_wgs = int(hdr[0])
    wgs = wg_list[:n_wgs]
    single = (wgs >> 31) == 0
    where = {int(b): i for i, b in enumerate(wgs.tolist()) if b < 0x80000000}
    pos = [where.get(int(b), -1) for b in order[:32].tolist()]                     # (-1: the block sits in a packed workgroup)
    at = np.array([p for p in pos if p >= 0], np.int64)
    return {"n_single": int(single.sum()), "n_packed": int((~single).sum()), "n_wgs": n_wgs,
            "first_packed_at": int(np.argmax(~single)) if (~single).any() else -1,
            "top32_positions": pos, "top32_mod8": np.bincount(at % 8, minlength=8).tolist(), "top32_mod4": np.bincount(at % 4, minlength=4).tolist(),
            "head": [int(b) for b in order[:8].tolist()]}


timed(1)                                                   # frame 1: the prior's list
rows = []
for k in range(LISTS):
    ms = timed(1)                                          # frame 2 + 16 k: the first of list k (frame 2 with the sort in front of it)
    d = describe(acc.order_lists(acc.order_judge()["read_set"]))
    ms += timed(15)                                        # (the last one has the next sort behind it)
    d["median_ms"] = statistics.median(ms[1:15])
    d["ms"] = [round(t, 4) for t in ms]
    rows.append(d)
fastest = min(r["median_ms"] for r in rows)
for r in rows:
    r["regime"] = "slow" if r["median_ms"] > 1.08 * fastest else "fast"
same_heads = sum(1 for a, b in zip(rows, rows[1:]) if a["head"] == b["head"])
summary = {}
for regime in ("fast", "slow"):
    sel = [r for r in rows if r["regime"] == regime]
    if sel:
        summary[regime] = {"lists": len(sel), "median_ms": [round(r["median_ms"], 4) for r in sel], "n_single": [r["n_single"] for r in sel],
                           "n_packed": [r["n_packed"] for r in sel], "first_packed_at": [r["first_packed_at"] for r in sel],
                           "top32_mod8": [r["top32_mod8"] for r in sel], "top32_mod4": [r["top32_mod4"] for r in sel],
                           "top32_last_position": [max(r["top32_positions"]) for r in sel]}
print(json.dumps({"lib": os.path.relpath(rtk.lib_path(), ROOT), "lists": LISTS, "fastest_median_ms": fastest,
                  "consecutive_lists_with_the_same_8_costliest": same_heads, "summary": summary, "rows": rows}))
