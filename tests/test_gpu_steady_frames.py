"""Steady frames without a counter fill: a megakernel frame counts into the block the frame before it cleared and clears the other
one for the frame behind it (csrc/frame_plan.hpp CounterState, RenderArgs::zero_next).  Nothing of that may show: 40 consecutive
frames of one accel -- across the re-sorts at frames 18 and 34 -- are each the frame of a fresh accel bit for bit, with the
oracle's ray count every time, also with every other user of the counters called in between, on alternating streams, across a size
change and back, with four and eight waves per block and on one rank of a sharded frame.  One loop enqueues its 40 frames
without a wait in between, as the benchmark does: the host is then frames ahead of the device.

Shapes: scene5 at 64x64 (one bucket, 64 blocks) and 320x180 (15 buckets, ragged at the right and bottom edges, several blocks
per counter shard), and two triangles at 44x28 (ragged blocks at both edges, most blocks background: packed workgroups)."""
import math

import numpy as np
import pytest

from conftest import SCENE5
from update_checks import _rtk_scene

pytestmark = pytest.mark.gpu

DEPTH = 5
FRAMES = 40
GROUP4, GROUP8 = 3, 4
KEYS = ("nodes", "boxpass", "leaves", "tris", "hits")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def two_triangle_scene(ora):
    """One diffuse floor of two triangles under one light, seen from the origin: the lower half of a frame, background above."""
    return ora.FlatScene(
        mesh_material=np.array([0], np.int32), mesh_nverts=np.array([4], np.int32), mesh_ntris=np.array([2], np.int32),
        vertices=np.array([[-4, -1, 0], [4, -1, 0], [4, -1, -8], [-4, -1, -8]], np.float32),
        indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
        mat_kind=np.array([ora.MAT_DIFFUSE], np.int32), mat_albedo=np.array([[0.8, 0.7, 0.2]], np.float32),
        mat_ior=np.array([1.0], np.float32), mat_smooth=np.zeros(1, np.int32),
        light_pos=np.array([[1, 2, -3]], np.float32), light_intensity=np.array([120], np.float32),
        cam_pos=np.zeros(3, np.float32), cam_mat=np.eye(3, dtype=np.float32).reshape(-1),
        background=np.array([0.1, 0.2, 0.3], np.float32), width=44, height=28, bucket_size=64)


CASES = {"scene5_64": ("scene5", 64, 64), "scene5_320": ("scene5", 320, 180), "two_tri_44": ("two_tri", 44, 28)}
_cache = {}


def _accel(rtk, ora, scene):
    if scene == "scene5":
        return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    return rtk.KdTreeSimdAccel(_rtk_scene(rtk, two_triangle_scene(ora)))


def _oracle(ora, scene, w, h):
    """(frame, counters) of the CPU oracle, with the reference's per-ray work; made once per shape."""
    key = ("oracle", scene, w, h)
    if key not in _cache:
        osc = ora.Scene(ora.load_crtscene(SCENE5)) if scene == "scene5" else ora.Scene(two_triangle_scene(ora))
        _cache[key] = ora.Accel(osc, ora.ACCEL_KD_SIMD).render(w, h, 1, DEPTH, 0)
    return _cache[key]


def _cfg(rtk, w, h, mode, **kw):
    return rtk.RenderConfig(width=w, height=h, max_ray_depth=DEPTH, trace_mode=mode, **kw)


def _device_frame(acc, cfg, stream=None):
    """One frame into device memory on `stream` (a torch stream; None: the current one) -> (floats, counters, critical path ms)."""
    import torch
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        buf = torch.full((acc.output_floats(cfg),), float("nan"), dtype=torch.float32, device="cuda")
    acc.render_frame_device(cfg, buf.data_ptr(), s.cuda_stream)
    cn = acc.last_counters()                           # (waits for the frame's stream)
    ms = acc.last_critical_path_ms()
    return buf.cpu().numpy(), cn, ms


def _frame_and_fills(acc, cfg, stream=None):
    """_device_frame, and how many fills of the counters the accel issued for it (rtk_debug_counter_fills: 0 for a steady frame)."""
    before = acc.counter_fills()
    got = _device_frame(acc, cfg, stream)
    return got, acc.counter_fills() - before


def _fresh(rtk, ora, scene, cfg):
    """The frame of a fresh accel, made once per (scene, configuration); never modified."""
    key = ("fresh", scene, tuple(sorted(cfg.__dict__.items())))
    if key not in _cache:
        out, cn, _ = _device_frame(_accel(rtk, ora, scene), cfg)
        out.setflags(write=False)
        _cache[key] = (out, cn)
    return _cache[key]


def _check_frame(got, want, rays, i):
    out, cn, ms = got
    assert out.shape == want[0].shape and np.array_equal(_bits(out), _bits(want[0])), i
    assert cn["rays"] == want[1]["rays"] == rays, (i, cn["rays"], want[1]["rays"], rays)
    assert math.isfinite(ms) and ms >= 0.0, (i, ms)
    return ms


@pytest.mark.parametrize("mode", [GROUP4, GROUP8], ids=["group4", "group8"])
@pytest.mark.parametrize("case", list(CASES))
def test_forty_frames_are_each_a_fresh_accels_frame(rtk, ora, case, mode):
    """Frames 18 and 34 re-sort; from frame 3 on no frame fills its counters.  The fresh frame is the oracle's, so every frame is."""
    scene, w, h = CASES[case]
    cfg = _cfg(rtk, w, h, mode)
    ref, ocn = _oracle(ora, scene, w, h)
    want = _fresh(rtk, ora, scene, cfg)
    assert np.array_equal(_bits(want[0]), _bits(ref).reshape(-1))
    acc = _accel(rtk, ora, scene)
    crit = []
    for i in range(FRAMES):
        got, fills = _frame_and_fills(acc, cfg)
        crit.append(_check_frame(got, want, ocn["rays"], i))
        assert fills == (1 if i < 2 else 0), (i, fills)        # the shape's first two frames fill their counters, no frame after them
    assert acc.counter_fills() == 2
    print(f"critical path of {case}, mode {mode}: min {min(crit):.4f} max {max(crit):.4f} ms")
    # a block reports from 10 us on (kernels.hip kCriticalMinTicks): the dragon's blocks at 320x180 take a multiple of that in
    # every frame; the other two shapes have none that long for certain, so theirs may be 0
    if case == "scene5_320":
        assert min(crit) > 0.0, crit


def test_forty_frames_of_a_sharded_rank(rtk, ora):
    """Rank 1 of 2 at 320x180 (eight of 15 buckets, one of them padding): its compact buffer and ray count never change, and the
    two ranks' rays are the oracle's."""
    _, ocn = _oracle(ora, "scene5", 320, 180)
    cfgs = [_cfg(rtk, 320, 180, GROUP4, rank=r, world_size=2) for r in (0, 1)]
    fresh = [_fresh(rtk, ora, "scene5", c) for c in cfgs]
    assert fresh[0][1]["rays"] + fresh[1][1]["rays"] == ocn["rays"]
    acc = _accel(rtk, ora, "scene5")
    for i in range(FRAMES):
        got, fills = _frame_and_fills(acc, cfgs[1])
        _check_frame(got, fresh[1], fresh[1][1]["rays"], i)
        assert fills == (1 if i < 2 else 0), (i, fills)


def _user_calls(rtk, ora, scene, w, h):
    """name -> call(accel) -> comparable result: every other user of the accel's counters, with what it reports."""
    import torch
    cfg = _cfg(rtk, w, h, GROUP4)
    rays = _accel(rtk, ora, scene).camera_rays(cfg).reshape(-1, 6)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.empty((rays.shape[0], 32), dtype=torch.uint8, device="cuda")
    max_t = np.full(rays.shape[0], 10.0, np.float32)
    views = np.zeros((2, 12), np.float32)
    views[:, 3:] = np.eye(3, dtype=np.float32).reshape(-1)
    views[1, :3] = [0.25, 0.5, 0.5]
    rects = [(3, 3, 20, 17), (w // 2, 1, w - 1, h - 5)]

    def stats_frame(level):
        def call(acc):
            out, cn = acc.render_frame(rtk.RenderConfig(**{**cfg.__dict__, "collect_stats": level}))
            return _bits(out).tobytes(), tuple(sorted(cn.items()))
        return call

    def regions(acc):
        packed, cn = acc.render_regions(cfg, rects, rtk.REGIONS_PACKED)
        return tuple(_bits(p).tobytes() for p in packed), cn["rays"]

    def views_call(acc):
        out, cn = acc.render_views(cfg, views)
        return _bits(out).tobytes(), cn["rays"]

    def occluded(acc):
        occ, n = acc.occluded(rays, max_t, count=True)
        return occ.tobytes(), n

    def intersect_stats(acc):
        cn = acc.intersect_stats(d_rays.data_ptr(), rays.shape[0], True, d_hits.data_ptr(), 2)
        torch.cuda.synchronize()
        return d_hits.cpu().numpy().tobytes(), tuple(sorted(cn.items()))

    return {"intersect_stats": intersect_stats, "occluded": occluded, "render_views": views_call, "render_regions": regions,
            "collect_stats_1": stats_frame(1), "collect_stats_2": stats_frame(2)}


USERS = ["intersect_stats", "occluded", "render_views", "render_regions", "collect_stats_1", "collect_stats_2"]


@pytest.mark.parametrize("user", USERS)
@pytest.mark.parametrize("case", list(CASES))
def test_forty_frames_with_another_counter_user_in_between(rtk, ora, case, user):
    """frame, frame, call, frame, frame, call ...: the frame behind a call fills its counters, the one after that is steady again.
    The call reports what it reports on a fresh accel (the statistics frames: the oracle's per-ray work at level 1, less at 2)."""
    scene, w, h = CASES[case]
    cfg = _cfg(rtk, w, h, GROUP4)
    ref, ocn = _oracle(ora, scene, w, h)
    want = _fresh(rtk, ora, scene, cfg)
    call = _user_calls(rtk, ora, scene, w, h)[user]
    expected = call(_accel(rtk, ora, scene))
    if user.startswith("collect_stats"):
        cn = dict(expected[1])
        assert expected[0] == _bits(ref).tobytes() and cn["rays"] == ocn["rays"]
        assert all(cn[k] == ocn[k] for k in KEYS) if user.endswith("1") else all(0 < cn[k] <= ocn[k] for k in ("nodes", "tris"))
    acc = _accel(rtk, ora, scene)
    for i in range(FRAMES):
        got, fills = _frame_and_fills(acc, cfg)
        _check_frame(got, want, ocn["rays"], i)
        assert fills == (1 if i < 2 or i % 3 == 2 else 0), (i, fills)       # only the frame right behind a call fills
        if i % 3 == 1:
            assert call(acc) == expected, i


@pytest.mark.parametrize("case", ["scene5_64", "scene5_320"])
def test_forty_frames_on_two_streams(rtk, ora, case):
    """Two frames on one torch stream, two on the other, and so on; then alternating every frame: a frame on another stream than
    the one before fills its counters itself, the second of two on one stream does not."""
    import torch
    scene, w, h = CASES[case]
    cfg = _cfg(rtk, w, h, GROUP4)
    _, ocn = _oracle(ora, scene, w, h)
    want = _fresh(rtk, ora, scene, cfg)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    acc = _accel(rtk, ora, scene)
    for i in range(FRAMES):
        s = streams[(i // 2) % 2] if i < FRAMES // 2 else streams[i % 2]
        got, fills = _frame_and_fills(acc, cfg, s)
        _check_frame(got, want, ocn["rays"], i)
        assert fills == (1 if i < 2 or i >= FRAMES // 2 or i % 2 == 0 else 0), (i, fills)
    torch.cuda.synchronize()


def test_forty_frames_with_a_size_change_and_back(rtk, ora):
    """64x64, three frames of 320x180 from frame 10, then 64x64 again: each frame is the fresh frame of its size.  The first frame of
    a size is still steady (the frame before it cleared its block) and the one behind it fills.  The longest block of 64x64 (64
    blocks, nothing to overlap with: ~0.5 ms) is longer than that of 320x180 (~0.35 ms), so the critical path of the first 320x180
    frame must come out below the 64x64 frame's before it: were the critical-path words not cleared, the maximum would stay."""
    cfgs = {False: _cfg(rtk, 64, 64, GROUP4), True: _cfg(rtk, 320, 180, GROUP4)}
    want = {k: _fresh(rtk, ora, "scene5", c) for k, c in cfgs.items()}
    rays = {False: _oracle(ora, "scene5", 64, 64)[1]["rays"], True: _oracle(ora, "scene5", 320, 180)[1]["rays"]}
    acc = _accel(rtk, ora, "scene5")
    crit = []
    for i in range(FRAMES):
        big = 10 <= i < 13
        got, fills = _frame_and_fills(acc, cfgs[big])
        crit.append(_check_frame(got, want[big], rays[big], i))
        assert fills == (1 if i in (0, 1, 11, 14) else 0), (i, fills)
    print("critical path around the size change:", [round(c, 4) for c in crit[8:15]])
    assert all(0.0 < crit[i] < crit[9] for i in (10, 11, 12)), crit[8:15]


@pytest.mark.parametrize("case", ["scene5_64", "scene5_320", "two_tri_44"])
def test_forty_frames_enqueued_without_a_wait(rtk, ora, case):
    """The host runs ahead of the device: 40 frames into 40 buffers with no wait in between (the length of the lists sorted at
    frames 18 and 34 is not seen before the wait at the end), then five more frames.  Every buffer is the fresh frame; the
    counters are the last frame's."""
    import torch
    scene, w, h = CASES[case]
    cfg = _cfg(rtk, w, h, GROUP4)
    _, ocn = _oracle(ora, scene, w, h)
    want = _fresh(rtk, ora, scene, cfg)
    acc = _accel(rtk, ora, scene)
    s = torch.cuda.current_stream()
    for n in (FRAMES, 5):
        bufs = torch.full((n, acc.output_floats(cfg)), float("nan"), dtype=torch.float32, device="cuda")
        for i in range(n):
            acc.render_frame_device(cfg, bufs[i].data_ptr(), s.cuda_stream)
        assert acc.last_counters()["rays"] == ocn["rays"]
        out = bufs.cpu().numpy()
        for i in range(n):
            assert np.array_equal(_bits(out[i]), _bits(want[0])), (n, i)
