"""Frame by frame: 64 consecutive steady frames of the benchmark's workload (scene5 1920x1080, depth 5), each between an event
pair of its own, enqueued back to back.  Prints every frame's time, the median and the longest frame -- a frame that re-sorts the
launch order (every 16th) shows as a hitch.  RTK_LIB_OVERRIDE selects another build of the library (simd-raytracer_amd/__init__.py).
usage: python tools/frame_times.py [warm-up frames, default 21]"""
import importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
rtk = importlib.import_module("simd-raytracer_amd")
SCENE = os.path.join(ROOT, "tests/golden/scenes/hw09/scene5.crtscene")
N = 64
warm = int(sys.argv[1]) if len(sys.argv) > 1 else 21
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
print(json.dumps({"lib": os.path.relpath(rtk.lib_path(), ROOT), "frames": N, "warmup": warm, "median_ms": med, "longest_ms": worst,
                  "longest_frame": ms.index(worst), "longest_over_median": worst / med,
                  "frames_over_1p15_median": [i for i, t in enumerate(ms) if t > 1.15 * med], "ms": [round(t, 4) for t in ms]}))
