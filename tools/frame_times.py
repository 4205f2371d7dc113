"""Frame by frame: consecutive steady frames of the benchmark's workload (scene5 1920x1080, depth 5), each between an event pair of
its own, enqueued back to back.  Prints every frame's time, the median and the longest frame -- a frame with a re-sort of the launch
order behind it shows as a hitch, and so does the one behind that, which carries the judge (csrc/order_judge.hpp).  With a library
that has it, the judge's counts and scores are printed too.  RTK_LIB_OVERRIDE selects another build of the library
(simd-raytracer_amd/__init__.py).  With no warm-up, entry i of `ms` is frame i + 1 of the accel: the sorts of the default schedule
are behind frames 17, 33, 65, 129, ..., the judges behind 18, 34, 66, 130, ....
usage: python tools/frame_times.py [warm-up frames, default 21] [timed frames, default 64]"""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
rtk = importlib.import_module("simd-raytracer_amd")
SCENE = os.path.join(ROOT, "tests/golden/scenes/hw09/scene5.crtscene")
warm = int(sys.argv[1]) if len(sys.argv) > 1 else 21
N = int(sys.argv[2]) if len(sys.argv) > 2 else 64
st = torch.cuda.current_stream()
frame = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE))
cfg = rtk.RenderConfig(width=1920, height=1080, max_ray_depth=5)
for _ in range(warm):
    acc.render_frame_device(cfg, frame.data_ptr(), st.cuda_stream)
torch.cuda.synchronize()
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
for a, b in ev:
    a.record(st); acc.render_frame_device(cfg, frame.data_ptr(), st.cuda_stream); b.record(st)
torch.cuda.synchronize()
ms = [a.elapsed_time(b) for a, b in ev]
med, worst = statistics.median(ms), max(ms)
judge = acc.order_judge() if hasattr(rtk._L, "rtk_debug_order_judge") else None
print(json.dumps({"lib": os.path.relpath(rtk.lib_path(), ROOT), "frames": N, "warmup": warm, "median_ms": med, "longest_ms": worst,
                  "longest_frame": ms.index(worst), "longest_over_median": worst / med,
                  "frames_over_1p15_median": [i for i, t in enumerate(ms) if t > 1.15 * med], "judge": judge,
                  "ms": [round(t, 4) for t in ms]}))
