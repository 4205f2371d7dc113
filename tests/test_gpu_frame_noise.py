"""rtk_render_frame_noise[_device] on the GPU.  The call has two existing doors to be compared with, bit for bit: rtk_render_frame for
rgb, rays and primary, and rtk_render_adaptive with min_samples = spp for the noise plane; beside them the statistic is recomputed in
numpy float64 from the single-sample colours (rtk_camera_rays + rtk_accel_radiance).  Frames are 70x36 (partial blocks on both edges)
and 5x3, with the zoomed cameras of tests/test_gpu_adaptive.py: at 90 degrees most of such a frame is background, whose noise is 0."""
import dataclasses

import numpy as np
import pytest

import denoise_model as dm
from conftest import SCENE2, SCENE5, SCENE8
from update_checks import _rtk_scene

pytestmark = pytest.mark.gpu

W, H = 70, 36
HW15 = dict(diffuse_rays=2, max_ray_depth=2, fov_degrees=40.0)
HW09 = dict(fov_degrees=12.0)
HW11 = dict(fov_degrees=60.0)
SCENES = {"hw15": (SCENE2, HW15), "hw09": (SCENE5, HW09), "hw11": (SCENE8, HW11)}
_ACCELS = {}
_BASE = {}


def _accel(rtk, path):
    if path not in _ACCELS:
        _ACCELS[path] = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    return _ACCELS[path]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cfg(rtk, spp, w=W, h=H, mode=None, **kw):
    return rtk.RenderConfig(width=w, height=h, spp=spp, trace_mode=rtk.TRACE_STREAM if mode is None else mode, **kw)


def _whole(rtk, spp):
    """the adaptive call that judges nothing before the ceiling"""
    return rtk.AdaptiveConfig(min_samples=spp, step=1, threshold=0.0, floor=1.0)


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2]


def _base(rtk, key, spp=8, w=W, h=H):
    """(rgb, noise, counters) of the call with the default knobs on the shared accel; computed once per shape, never changed"""
    k = (key, spp, w, h)
    if k not in _BASE:
        path, kw = SCENES[key]
        rgb, noise, cn = _accel(rtk, path).render_frame_noise(_cfg(rtk, spp, w, h, **kw))
        rgb.setflags(write=False)
        noise.setflags(write=False)
        _BASE[k] = (rgb, noise, cn)
    return _BASE[k]


# ---------------------------------------------------------------- 1. bits against the two existing doors

@pytest.mark.parametrize("key", ["hw15", "hw09", "hw11"])
def test_bits_against_the_frame_and_the_adaptive_call(rtk, key):
    path, kw = SCENES[key]
    acc = _accel(rtk, path)
    rgb, noise, cn = _base(rtk, key)
    ref, fcn = acc.render_frame(_cfg(rtk, 8, **kw))
    assert np.array_equal(_bits(rgb), _bits(ref)), int((_bits(rgb) != _bits(ref)).any(-1).sum())
    assert (cn["rays"], cn["primary"]) == (fcn["rays"], fcn["primary"]) and cn["primary"] == 8 * W * H
    if key == "hw09":
        ref4, fcn4 = acc.render_frame(_cfg(rtk, 8, mode=rtk.TRACE_GROUP4, **kw))
        assert np.array_equal(_bits(rgb), _bits(ref4)) and cn["rays"] == fcn4["rays"]
    argb, samples, anoise, acn = acc.render_adaptive(_cfg(rtk, 8, **kw), _whole(rtk, 8))
    assert (samples == 8).all() and np.array_equal(_bits(argb), _bits(rgb))
    assert np.array_equal(_bits(noise), _bits(anoise)), int((_bits(noise) != _bits(anoise)).sum())
    assert acn["rays"] == cn["rays"]
    # the comparison is not one of zeros
    depth = acc.render_gbuffer(_cfg(rtk, 8, **kw), sample=0, planes=("depth",))["depth"][0]
    hit = depth >= 0
    print(key, "hit pixels", int(hit.sum()), "with noise > 0", int((noise[hit] > 0).sum()), "max", float(noise.max()))
    assert hit.sum() > 0 and (noise[hit] > 0).sum() * 4 > hit.sum()
    assert (noise >= 0).all()
    assert acc.noise_fallbacks() == 0


def test_the_call_reports_itself(rtk):
    acc = _accel(rtk, SCENE2)
    got = acc.render_frame_noise(_cfg(rtk, 8, **HW15))
    assert acc.last_counters() == got[2] and acc.last_critical_path_ms() == 0.0
    assert _same(got, _base(rtk, "hw15"))
    # RTK_TRACE_AUTO means RTK_TRACE_STREAM here
    auto = acc.render_frame_noise(_cfg(rtk, 8, mode=rtk.TRACE_AUTO, **HW15))
    assert _same(auto, got)


# ---------------------------------------------------------------- 2. the statistic, recomputed

def test_noise_against_numpy_float64(rtk):
    """rtk.h: y in float32 (numpy does not contract), S1 and S2 in float64 in sample order, v = max(0, (S2 - S1^2 / n) / (n - 1)) / n"""
    acc = _accel(rtk, SCENE2)
    spp = 8
    cfg = _cfg(rtk, spp, **HW15)
    ids = np.arange(W * H, dtype=np.uint32)
    cols = np.zeros((spp, H, W, 3), np.float32)
    for s in range(spp):
        rays = acc.camera_rays(cfg, s).reshape(-1, 6)
        rc = rtk.RadianceConfig(max_ray_depth=cfg.max_ray_depth, diffuse_rays=cfg.diffuse_rays, seed=cfg.seed, sample=s,
                                shadow_bias=cfg.shadow_bias, reflection_bias=cfg.reflection_bias, refraction_bias=cfg.refraction_bias, cull=True)
        cols[s] = acc.radiance(rays, ids, rc)[0].reshape(H, W, 3)
    y = (np.float32(0.2126) * cols[..., 0] + np.float32(0.7152) * cols[..., 1]) + np.float32(0.0722) * cols[..., 2]
    assert y.dtype == np.float32
    y64 = y.astype(np.float64)
    S1, S2, n = np.cumsum(y64, axis=0)[-1], np.cumsum(y64 * y64, axis=0)[-1], np.float64(spp)
    e = np.sqrt(np.maximum(0.0, (S2 - S1 * S1 / n) / (n - 1.0)) / n)
    rgb, noise, _ = _base(rtk, "hw15")
    err = np.abs(noise.astype(np.float64) - e)
    print("max |noise - e|", float(err.max()), "max e", float(e.max()))
    assert e.max() > 1e-3 and err.max() <= 1e-6
    # and the frame is the mean of those colours, added in sample order from +0
    acc_sum = np.zeros((H, W, 3), np.float32)
    for s in range(spp):
        acc_sum = acc_sum + cols[s]
    assert np.array_equal(_bits(acc_sum / np.float32(spp)), _bits(rgb))


# ---------------------------------------------------------------- 3. batch shapes

@pytest.mark.parametrize("batch,lanes", [(3, 2), (1, 1)])
def test_batch_shapes_keep_the_bits(rtk, monkeypatch, batch, lanes):
    """spp 8 as 3 + 3 + 2 over two lanes, and as eight launches on one stream; spp 2 (one batch, first and last) and spp 3 on 5x3"""
    base = _base(rtk, "hw15")
    small = {spp: _base(rtk, "hw15", spp, 5, 3) for spp in (2, 3)}
    monkeypatch.setenv("RTK_STREAM_BATCH", str(batch))              # (read when an accel is built)
    monkeypatch.setenv("RTK_STREAM_LANES", str(lanes))
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    monkeypatch.delenv("RTK_STREAM_BATCH")
    monkeypatch.delenv("RTK_STREAM_LANES")
    got = acc.render_frame_noise(_cfg(rtk, 8, **HW15))
    assert _same(got, base), (int((_bits(got[0]) != _bits(base[0])).sum()), int((_bits(got[1]) != _bits(base[1])).sum()))
    for spp in (2, 3):
        g = acc.render_frame_noise(_cfg(rtk, spp, 5, 3, **HW15))
        assert g[0].shape == (3, 5, 3) and g[1].shape == (3, 5)
        assert _same(g, small[spp]), spp
        ref, fcn = acc.render_frame(_cfg(rtk, spp, 5, 3, **HW15))
        assert np.array_equal(_bits(g[0]), _bits(ref)) and g[2]["rays"] == fcn["rays"]
    assert acc.noise_fallbacks() == 0 and _accel(rtk, SCENE2).noise_fallbacks() == 0


def test_frames_and_noise_calls_alternate_on_one_accel(rtk, monkeypatch):
    """Both clients of the streamed-frame launcher on ONE accel, one sample per launch over two lanes: a frame at spp 1 (the
    workspace is made without a sum buffer), the noise call at spp 3 (three launches, and the workspace grows to hold the sum
    buffer), a frame at spp 1 again, a frame at spp 3.  Each is the same call on the shared default-knob accel, bit for bit."""
    shared = _accel(rtk, SCENE2)
    want_noise = _base(rtk, "hw15", 3, 5, 3)
    want_frame = {spp: shared.render_frame(_cfg(rtk, spp, 5, 3, **HW15)) for spp in (1, 3)}
    monkeypatch.setenv("RTK_STREAM_BATCH", "1")                     # (read when an accel is built)
    monkeypatch.setenv("RTK_STREAM_LANES", "2")
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    monkeypatch.delenv("RTK_STREAM_BATCH")
    monkeypatch.delenv("RTK_STREAM_LANES")

    def frame(spp):
        rgb, cn = acc.render_frame(_cfg(rtk, spp, 5, 3, **HW15))
        ref, fcn = want_frame[spp]
        assert np.array_equal(_bits(rgb), _bits(ref)), spp
        assert (cn["rays"], cn["primary"]) == (fcn["rays"], fcn["primary"]) and cn["primary"] == spp * 5 * 3, spp

    frame(1)
    got = acc.render_frame_noise(_cfg(rtk, 3, 5, 3, **HW15))
    assert np.array_equal(_bits(got[0]), _bits(want_noise[0])) and np.array_equal(_bits(got[1]), _bits(want_noise[1]))
    assert (got[2]["rays"], got[2]["primary"]) == (want_noise[2]["rays"], want_noise[2]["primary"])
    frame(1)
    frame(3)
    assert acc.noise_fallbacks() == 0 and shared.noise_fallbacks() == 0


# ---------------------------------------------------------------- 4. overflow

def test_a_queue_overflow_redoes_the_call_with_the_same_results(rtk, monkeypatch):
    """room for the camera rays only (the shape of test_streaming_pipeline_queue_overflow_falls_back_to_the_megakernel): the flag is
    read back, the call is redone through the adaptive path and counted"""
    kw = dict(max_ray_depth=6)
    ref_acc = _accel(rtk, SCENE8)
    cfg = _cfg(rtk, 2, 200, 120, **kw)
    ref, fcn = ref_acc.render_frame(cfg)
    _, _, anoise, _ = ref_acc.render_adaptive(cfg, _whole(rtk, 2))
    monkeypatch.setenv("RTK_STREAM_NODE_FACTOR", "1")               # (read when an accel is built)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    monkeypatch.delenv("RTK_STREAM_NODE_FACTOR")
    assert acc.noise_fallbacks() == 0
    rgb, noise, cn = acc.render_frame_noise(cfg)
    assert acc.noise_fallbacks() == 1
    assert np.array_equal(_bits(rgb), _bits(ref))
    assert np.array_equal(_bits(noise), _bits(anoise)) and noise.max() > 0
    assert (cn["rays"], cn["primary"]) == (fcn["rays"], fcn["primary"])
    assert acc.last_counters() == cn
    assert ref_acc.noise_fallbacks() == 0


# ---------------------------------------------------------------- 5. variants

def test_host_device_and_a_second_call_agree(rtk):
    import torch
    acc = _accel(rtk, SCENE2)
    base = _base(rtk, "hw15")
    assert _same(acc.render_frame_noise(_cfg(rtk, 8, **HW15)), base)
    n, guard = W * H, 64
    d_rgb = torch.full((n * 3 + guard,), float("nan"), dtype=torch.float32, device="cuda")
    d_noise = torch.full((n + guard,), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(stream):
            d_rgb.fill_(float("nan"))
            d_noise.fill_(float("nan"))
            acc.render_frame_noise_device(_cfg(rtk, 8, **HW15), d_rgb.data_ptr(), d_noise.data_ptr(), stream.cuda_stream)
        cn = acc.last_counters()
        stream.synchronize()
        rgb, noise = d_rgb.cpu().numpy(), d_noise.cpu().numpy()
        assert np.isnan(rgb[n * 3:]).all() and np.isnan(noise[n:]).all()
        assert not np.isnan(rgb[:n * 3]).any() and not np.isnan(noise[:n]).any()
        assert _same((rgb[:n * 3].reshape(H, W, 3), noise[:n].reshape(H, W), cn), base)
    # the host variant into the caller's arrays overwrites every element too
    L, p = rtk.lib(), _cfg(rtk, 8, **HW15).to_c()
    import ctypes
    h_rgb, h_noise = np.full((H, W, 3), np.nan, np.float32), np.full((H, W), np.nan, np.float32)
    assert L.rtk_render_frame_noise(acc._h, ctypes.byref(p), h_rgb.ctypes.data, h_noise.ctypes.data, None) == rtk.RTK_OK
    assert np.array_equal(_bits(h_rgb), _bits(base[0])) and np.array_equal(_bits(h_noise), _bits(base[1]))
    assert acc.noise_fallbacks() == 0


# ---------------------------------------------------------------- 6. state

def test_camera_and_counters_around_a_call_are_those_of_a_stream_frame(rtk):
    """two accels side by side: GROUP4 frames until they are steady, then this call on one and an RTK_TRACE_STREAM frame on the other,
    then GROUP4 frames again: the same fills and the same counters, step by step"""
    fcfg = _cfg(rtk, 1, mode=rtk.TRACE_GROUP4, **HW09)
    ncfg = _cfg(rtk, 4, **HW09)
    accs = [rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5)) for _ in range(2)]
    log = [[], []]

    def step(i, call):
        before = accs[i].counter_fills()
        out = call(accs[i])
        log[i].append((accs[i].counter_fills() - before, out[-1], accs[i].last_counters()))
        return out

    for i in range(2):
        frames = [step(i, lambda a: a.render_frame(fcfg)) for _ in range(3)]
        assert [e[0] for e in log[i]] == [1, 1, 0]
    cam = [x.copy() for x in accs[0].camera()]
    got = step(0, lambda a: a.render_frame_noise(ncfg))
    ref = step(1, lambda a: a.render_frame(ncfg))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cam, accs[0].camera()))
    assert np.array_equal(_bits(got[0]), _bits(ref[0]))
    assert accs[0].last_critical_path_ms() == 0.0
    after = [[step(i, lambda a: a.render_frame(fcfg)) for _ in range(3)] for i in range(2)]
    assert log[0] == log[1], (log[0], log[1])
    assert log[0][3][0] == 1 and log[0][-1][0] == 0                          # one fill for the call; the frames are steady again
    for a, b in zip(after[0], after[1]):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[0]), _bits(frames[2][0]))


def test_the_call_reads_the_live_lights_and_geometry(rtk, ora):
    flat = ora.load_crtscene(SCENE5)
    lights = flat.light_pos.astype(np.float32).copy()
    lights[0] = lights[0] + np.array([-6.0, 3.0, 5.0], np.float32)
    verts = (flat.vertices + np.array([0.3, 0.2, -0.4], np.float32)).astype(np.float32)
    cfg = _cfg(rtk, 4, **HW09)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    seen = [acc.render_frame_noise(cfg)]
    acc.set_lights(lights, flat.light_intensity)
    acc.update_vertices(verts)
    seen.append(acc.render_frame_noise(cfg))
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, dataclasses.replace(flat, light_pos=lights, vertices=verts)))
    assert _same(seen[-1], fresh.render_frame_noise(cfg))
    assert not np.array_equal(_bits(seen[0][0]), _bits(seen[1][0]))           # the step was no no-op


# ---------------------------------------------------------------- 7. the chain

def test_frame_noise_then_gbuffer_then_denoise(rtk):
    """render_frame_noise -> render_gbuffer -> denoise gives the bits of the chain with render_adaptive(min_samples = spp) in its place"""
    acc = _accel(rtk, SCENE2)
    cfg = _cfg(rtk, 8, **HW15)
    rgb, noise, _ = _base(rtk, "hw15")
    argb, _, anoise, _ = acc.render_adaptive(cfg, _whole(rtk, 8))
    gb = acc.render_gbuffer(cfg, sample=0, planes=("depth", "position", "normal", "albedo"))
    normal, position, depth, albedo = gb["normal"][0], gb["position"][0], gb["depth"][0], gb["albedo"][0]
    dcfg = rtk.DenoiseConfig(**dm.PARAMS)
    got = rtk.denoise(np.array(rgb), normal, position, depth, np.array(noise), albedo, dcfg)
    want = rtk.denoise(argb, normal, position, depth, anoise, albedo, dcfg)
    hit = depth >= 0
    changed = (_bits(got) != _bits(rgb)).any(-1)
    assert hit.sum() > W * H // 4 and changed[hit].sum() * 2 > hit.sum()      # otherwise the case shows nothing
    assert np.array_equal(_bits(got), _bits(want))
