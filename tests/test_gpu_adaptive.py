"""rtk_render_adaptive[_device] on the GPU.  The single-sample colours of every pixel come from existing, pinned code
(rtk_camera_rays(.., s) + rtk_accel_radiance(sample = s), bit-equal to sample s of a frame); from them the statistic of rtk.h is
recomputed in numpy float64 for every block and checkpoint, the threshold is chosen from that data so that no block sits on it, and
the call's `samples` plane is predicted.  Pixels are compared by their bits with rtk_render_frame at spp = samples[pixel], `rays`
with rtk_render_regions over the blocks that ended at each checkpoint.  Frames are 70x36 (partial blocks on both edges) and 5x3."""
import dataclasses

import numpy as np
import pytest

from conftest import SCENE2, SCENE5, SCENE8
from update_checks import _rtk_scene

pytestmark = pytest.mark.gpu

W, H = 70, 36
# hw15/scene2 is a box that a 90 degree camera sees as a tenth of a 70x36 frame, the rest background: at 40 degrees it fills the
# frame's height and most of its width, so the blocks' noise spreads over a range and the threshold has something to decide
HW15 = dict(diffuse_rays=2, max_ray_depth=2, fov_degrees=40.0)
# Likewise hw09/scene5 and hw11/scene8: at 90 degrees most blocks of a 70x36 frame see the background or the flat floor, whose
# colour no jitter changes (E_B = 0 exactly, the median included), and the few others all run to the ceiling.  Zoomed in on the
# dragon every block has a slope to alias, and stops at 2, 4, 6 or 8 samples.
HW09 = dict(fov_degrees=12.0)
HW11 = dict(fov_degrees=60.0)
_ACCELS = {}
_COLOURS = {}


def _accel(rtk, path):
    if path not in _ACCELS:
        _ACCELS[path] = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))
    return _ACCELS[path]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cfg(rtk, spp, w=W, h=H, mode=None, **kw):
    return rtk.RenderConfig(width=w, height=h, spp=spp, trace_mode=rtk.TRACE_STREAM if mode is None else mode, **kw)


def _checkpoints(spp, mn, step):
    out = list(range(mn, spp, step))
    return out + [spp]


def _blocks(w, h):
    """(x0, y0, x1, y1) of the frame's own 8x8 grid, row-major; edge blocks are partial"""
    return [(x, y, min(x + 8, w), min(y + 8, h)) for y in range(0, h, 8) for x in range(0, w, 8)]


def _colours(rtk, acc, key, spp, w, h, **kw):
    """[spp, h, w, 3]: sample s of every pixel, from rtk_camera_rays + rtk_accel_radiance; computed once per key, never changed"""
    k = (key, spp, w, h, tuple(sorted(kw.items())))
    if k not in _COLOURS:
        cfg = _cfg(rtk, spp, w, h, **kw)
        ids = np.arange(w * h, dtype=np.uint32)
        out = np.zeros((spp, h, w, 3), np.float32)
        for s in range(spp):
            rays = acc.camera_rays(cfg, s).reshape(-1, 6)
            rc = rtk.RadianceConfig(max_ray_depth=cfg.max_ray_depth, diffuse_rays=cfg.diffuse_rays, seed=cfg.seed, sample=s,
                                    shadow_bias=cfg.shadow_bias, reflection_bias=cfg.reflection_bias,
                                    refraction_bias=cfg.refraction_bias, cull=True)
            rgb, _ = acc.radiance(rays, ids, rc)
            out[s] = rgb.reshape(h, w, 3)
        out.setflags(write=False)
        _COLOURS[k] = out
    return _COLOURS[k]


def _statistic(cols, checkpoints, floor):
    """rtk.h, item 3, in numpy: e [n][h][w] (float64) and E [n][block] at every checkpoint n.  float32 products and sums for y (numpy
    does not contract), float64 running sums in sample order, the block sums over the valid pixels in row-major order."""
    r, g, b = cols[..., 0], cols[..., 1], cols[..., 2]
    y = (np.float32(0.2126) * r + np.float32(0.7152) * g) + np.float32(0.0722) * b
    assert y.dtype == np.float32
    y64 = y.astype(np.float64)
    s1, s2 = np.cumsum(y64, axis=0), np.cumsum(y64 * y64, axis=0)            # (cumsum adds in order)
    h, w = y.shape[1:]
    fl = np.float64(np.float32(floor))
    e_at, E_at = {}, {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in checkpoints:
            S1, S2, nn = s1[n - 1], s2[n - 1], np.float64(n)
            m = S1 / nn
            v = np.maximum(0.0, (S2 - S1 * S1 / nn) / (nn - 1.0)) / nn
            e = np.sqrt(v)
            E = []
            for x0, y0, x1, y1 in _blocks(w, h):
                se = sm = np.float64(0.0)
                for ev, mv in zip(e[y0:y1, x0:x1].ravel(), m[y0:y1, x0:x1].ravel()):
                    se += ev
                    sm += mv
                cnt = np.float64((x1 - x0) * (y1 - y0))
                E.append((se / cnt) / np.maximum(sm / cnt, fl))
            e_at[n], E_at[n] = e, np.array(E, np.float64)
    return e_at, E_at


def _middle(checkpoints):
    return checkpoints[(len(checkpoints) - 1) // 2]


def _choose_threshold(E_at, checkpoints):
    """the midpoint of the widest gap between neighbouring sorted E_B values around the median of the middle checkpoint: among the
    quarter of the sorted values that has the median in its middle, widened on both sides while all of them are equal"""
    E = np.sort(E_at[_middle(checkpoints)])
    n = len(E)
    assert np.isfinite(E).all() and E[0] < E[-1]
    half = max(2, n // 8)
    lo, hi = max(n // 2 - half, 0), min(n // 2 + half + 1, n)
    while E[lo] == E[hi - 1]:
        lo, hi = max(lo - 1, 0), min(hi + 1, n)
    gaps = E[lo + 1:hi] - E[lo:hi - 1]
    i = lo + int(np.argmax(gaps))
    thr = np.float32((E[i] + E[i + 1]) / 2)
    assert E[i] < np.float64(thr) < E[i + 1], "the float32 threshold lies strictly inside the gap"
    return float(thr)


def _predict(E_at, checkpoints, thr, w, h):
    """samples [h][w] as the contract says, and the blocks within a relative 1e-9 of the threshold at some checkpoint"""
    t = np.float64(np.float32(thr))
    blocks = _blocks(w, h)
    samples = np.zeros((h, w), np.uint32)
    near = np.zeros(len(blocks), bool)
    for bi, (x0, y0, x1, y1) in enumerate(blocks):
        final = checkpoints[-1]
        for n in checkpoints:
            if abs(E_at[n][bi] - t) <= 1e-9 * t:
                near[bi] = True
            if E_at[n][bi] <= t:
                final = n
                break
        samples[y0:y1, x0:x1] = final
    return samples, near


def _check_against_frames(rtk, acc, got, spp, mn, step, frame_mode, what, w=W, h=H, **kw):
    """samples: checkpoints, equal over a block; rgb: the frame of spp = samples[px], by bits; primary"""
    rgb, samples, noise, cn = got
    cps = _checkpoints(spp, mn, step)
    assert set(np.unique(samples).tolist()) <= set(cps), (what, np.unique(samples))
    for x0, y0, x1, y1 in _blocks(w, h):
        assert (samples[y0:y1, x0:x1] == samples[y0, x0]).all(), (what, x0, y0)
    for n in np.unique(samples).tolist():
        ref, _ = acc.render_frame(_cfg(rtk, n, w, h, mode=frame_mode, **kw))
        mask = samples == n
        bad = int((_bits(rgb)[mask] != _bits(ref)[mask]).any(axis=-1).sum())
        assert bad == 0, (what, n, bad, int(mask.sum()))
    assert cn["primary"] == int(samples.astype(np.int64).sum()), what


def _rays_by_regions(rtk, acc, samples, w=W, h=H, **kw):
    """item 2: the sum over the checkpoints n of what rtk_render_regions(spp = n, RTK_TRACE_STREAM) reports for the blocks that ended at n"""
    total = 0
    for n in np.unique(samples).tolist():
        rects = [b for b in _blocks(w, h) if samples[b[1], b[0]] == n]
        _, cn = acc.render_regions(_cfg(rtk, n, w, h, **kw), rects, rtk.REGIONS_PACKED)
        assert cn["primary"] == n * sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in rects)
        total += cn["rays"]
    return total


def _full_check(rtk, path, key, frame_mode, spp=8, mn=2, step=2, floor=0.01, bits_only=False, **kw):
    acc = _accel(rtk, path)
    cps = _checkpoints(spp, mn, step)
    cols = _colours(rtk, acc, key, spp, W, H, **kw)
    e_at, E_at = _statistic(cols, cps, floor)
    thr = _choose_threshold(E_at, cps)
    want, near = _predict(E_at, cps, thr, W, H)
    print(key, "threshold", thr, "E at the middle checkpoint", np.sort(E_at[_middle(cps)]).tolist())
    print(key, "predicted counts", {n: int((want == n).sum()) for n in np.unique(want).tolist()}, "near", int(near.sum()))
    assert near.sum() <= len(near) // 100, (key, "blocks at the threshold", int(near.sum()))
    counts = set(np.unique(want).tolist())
    assert len(counts) >= 3 and mn in counts and spp in counts, (key, "the data decides nothing", sorted(counts))
    ad = rtk.AdaptiveConfig(min_samples=mn, step=step, threshold=thr, floor=floor)
    got = acc.render_adaptive(_cfg(rtk, spp, **kw), ad)
    rgb, samples, noise, cn = got
    print(key, "got counts", {n: int((samples == n).sum()) for n in np.unique(samples).tolist()}, cn)
    _check_against_frames(rtk, acc, got, spp, mn, step, frame_mode, key, **kw)
    if bits_only:
        return
    # the decision, on every block that is not at the threshold
    keep = np.ones((H, W), bool)
    for bi, (x0, y0, x1, y1) in enumerate(_blocks(W, H)):
        keep[y0:y1, x0:x1] = not near[bi]
    assert np.array_equal(samples[keep], want[keep]), (key, int((samples != want).sum()))
    # noise = (float)e_i at the pixel's final count
    e_final = np.zeros((H, W), np.float64)
    for n in cps:
        e_final = np.where(samples == n, e_at[n], e_final)
    assert np.allclose(noise.astype(np.float64), e_final.astype(np.float32).astype(np.float64), rtol=1e-6, atol=0.0), key
    assert (noise >= 0).all() and noise.max() > 0
    assert cn["rays"] == _rays_by_regions(rtk, acc, samples, **kw), key
    assert acc.last_counters() != cn                                         # (the regions calls behind it reported themselves)


# ---------------------------------------------------------------- 1. the contract, scene by scene

def test_hw15_scene2_diffuse_gi(rtk):
    """diffuse_rays = 2, depth 2, min 2, step 2, spp 8: samples as predicted, rgb by bits against STREAM frames, noise, rays, primary"""
    _full_check(rtk, SCENE2, "hw15", None, **HW15)


def test_hw09_scene5_jitter_only(rtk):
    """no forks, the jitter alone makes the variance; the frames it is compared with are the megakernel's (RTK_TRACE_GROUP4)"""
    _full_check(rtk, SCENE5, "hw09", rtk.TRACE_GROUP4, **HW09)


def test_hw11_scene8_refraction_bits(rtk):
    _full_check(rtk, SCENE8, "hw11", None, bits_only=True, **HW11)


# ---------------------------------------------------------------- 2. the ends of the schedule

def test_min_equal_to_spp_is_the_frame(rtk):
    acc = _accel(rtk, SCENE2)
    kw = dict(HW15)
    ref, fcn = acc.render_frame(_cfg(rtk, 4, **kw))
    rgb, samples, noise, cn = acc.render_adaptive(_cfg(rtk, 4, **kw), rtk.AdaptiveConfig(min_samples=4, step=1, threshold=0.0, floor=0.01))
    assert (samples == 4).all()
    assert np.array_equal(_bits(rgb), _bits(ref))
    assert (cn["rays"], cn["primary"]) == (fcn["rays"], 4 * W * H)
    assert noise.max() > 0


def test_zero_variance_stops_every_pixel_at_min(rtk):
    """threshold = 0 on a camera that sees the background only: E_B = 0 <= 0 everywhere"""
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    pos, mat = acc.camera()
    acc.set_camera(pos + np.array([0.0, 0.0, -1.0e5], np.float32), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32))
    rgb, samples, noise, cn = acc.render_adaptive(_cfg(rtk, 8), rtk.AdaptiveConfig(min_samples=2, step=2, threshold=0.0, floor=0.01))
    bg = np.asarray(acc.background(), np.float32)
    assert np.array_equal(_bits(rgb), _bits(np.broadcast_to(bg, (H, W, 3)))), "the camera sees more than the background"
    assert (samples == 2).all() and (noise == 0).all()
    assert (cn["rays"], cn["primary"]) == (2 * W * H, 2 * W * H)


# ---------------------------------------------------------------- 3. chunks, shapes, variants

def _hw15_call(rtk, acc, spp=8, mn=2, step=2, w=W, h=H, thr=None):
    kw = dict(HW15)
    if thr is None:
        cps = _checkpoints(8, 2, 2)
        _, E_at = _statistic(_colours(rtk, _accel(rtk, SCENE2), "hw15", 8, W, H, **kw), cps, 0.01)
        thr = _choose_threshold(E_at, cps)
    return acc.render_adaptive(_cfg(rtk, spp, w, h, **kw), rtk.AdaptiveConfig(min_samples=mn, step=step, threshold=thr, floor=0.01)), kw, thr


def _same_result(a, b):
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))
            and a[3] == b[3])


def test_chunks_of_1000_pixels_give_the_same_bits(rtk, monkeypatch):
    base, _, thr = _hw15_call(rtk, _accel(rtk, SCENE2))
    assert len(np.unique(base[1])) >= 3
    monkeypatch.setenv("RTK_ADAPTIVE_CHUNK_PIXELS", "1000")            # (read when an accel is built: 2520 pixels are three chunks)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    monkeypatch.delenv("RTK_ADAPTIVE_CHUNK_PIXELS")
    got, _, _ = _hw15_call(rtk, acc, thr=thr)
    assert _same_result(got, base)


def test_a_5x3_frame(rtk):
    acc = _accel(rtk, SCENE2)
    got, kw, _ = _hw15_call(rtk, acc, spp=6, mn=2, step=2, w=5, h=3, thr=0.05)
    assert got[0].shape == (3, 5, 3) and len(np.unique(got[1])) == 1
    _check_against_frames(rtk, acc, got, 6, 2, 2, None, "5x3", w=5, h=3, **kw)


def test_a_step_that_does_not_divide(rtk):
    """min 2, step 3, spp 7: the checkpoints are 2, 5, 7"""
    acc = _accel(rtk, SCENE2)
    got, kw, _ = _hw15_call(rtk, acc, spp=7, mn=2, step=3)
    assert set(np.unique(got[1]).tolist()) <= {2, 5, 7} and len(np.unique(got[1])) >= 2
    _check_against_frames(rtk, acc, got, 7, 2, 3, None, "2, 5, 7", **kw)
    assert got[3]["rays"] == _rays_by_regions(rtk, acc, got[1], **kw)


def test_host_and_device_variants_agree_and_two_calls_agree(rtk):
    import torch
    acc = _accel(rtk, SCENE2)
    base, kw, thr = _hw15_call(rtk, acc)
    again, _, _ = _hw15_call(rtk, acc, thr=thr)
    assert _same_result(again, base)
    n, guard = W * H, 64
    d_rgb = torch.full((n * 3 + guard,), 7.0, dtype=torch.float32, device="cuda")
    d_samples = torch.full((n + guard,), 7, dtype=torch.int32, device="cuda")
    d_noise = torch.full((n + guard,), 7.0, dtype=torch.float32, device="cuda")
    ad = rtk.AdaptiveConfig(min_samples=2, step=2, threshold=thr, floor=0.01)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        acc.render_adaptive_device(_cfg(rtk, 8, **kw), ad, d_rgb.data_ptr(), d_samples.data_ptr(), d_noise.data_ptr(), stream.cuda_stream)
    cn = acc.last_counters()
    stream.synchronize()
    rgb, samples, noise = d_rgb.cpu().numpy(), d_samples.cpu().numpy().view(np.uint32), d_noise.cpu().numpy()
    assert (rgb[n * 3:] == 7).all() and (samples[n:] == 7).all() and (noise[n:] == 7).all()
    assert _same_result((rgb[:n * 3].reshape(H, W, 3), samples[:n].reshape(H, W), noise[:n].reshape(H, W), cn), base)
    # samples and noise are optional
    d_rgb.fill_(7.0)
    acc.render_adaptive_device(_cfg(rtk, 8, **kw), ad, d_rgb.data_ptr(), 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_rgb.cpu().numpy()[:n * 3]), _bits(base[0]).reshape(-1)) and acc.last_counters() == cn


# ---------------------------------------------------------------- 4. state

def test_frames_regions_camera_and_counters_around_an_adaptive_call(rtk):
    """GROUP4 frames until they are steady, a regions call, then an adaptive call, then both again: the same bits and `rays`, the
    camera as it was.  The adaptive call fills the counter block once, as a regions call does, and reports itself
    (rtk_render_last_counters; its critical path is 0); the first frame behind it fills once more and the next is steady again."""
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    fcfg = _cfg(rtk, 1, mode=rtk.TRACE_GROUP4)
    rects = [(3, 2, 40, 30), (41, 0, 70, 36)]

    def frame():
        before = acc.counter_fills()
        rgb, cn = acc.render_frame(fcfg)
        return rgb, cn, acc.counter_fills() - before

    frames = [frame() for _ in range(3)]
    assert [f[2] for f in frames] == [1, 1, 0]
    reg = [acc.render_regions(fcfg, rects, rtk.REGIONS_PACKED) for _ in range(2)][-1]
    steady = [frame() for _ in range(2)]
    assert steady[-1][2] == 0
    cam = [x.copy() for x in acc.camera()]
    fills = acc.counter_fills()
    ad = rtk.AdaptiveConfig(min_samples=2, step=2, threshold=0.01, floor=0.01)
    got = acc.render_adaptive(_cfg(rtk, 6, mode=rtk.TRACE_AUTO), ad)
    assert acc.counter_fills() == fills + 1
    assert acc.last_counters() == got[3] and got[3]["primary"] == int(got[1].sum())
    assert acc.last_critical_path_ms() == 0.0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cam, acc.camera()))
    reg2 = acc.render_regions(fcfg, rects, rtk.REGIONS_PACKED)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(reg[0], reg2[0])) and reg2[1] == reg[1]
    after = [frame() for _ in range(3)]
    assert after[0][2] <= 1 and after[-1][2] == 0
    for f in after:
        assert np.array_equal(_bits(f[0]), _bits(frames[2][0])) and f[1] == frames[2][1]
    assert acc.last_critical_path_ms() >= 0.0
    # and the adaptive call itself is the same call before and after all that
    again = acc.render_adaptive(_cfg(rtk, 6, mode=rtk.TRACE_AUTO), ad)
    assert _same_result(again, got)


def test_the_call_reads_the_live_lights_and_geometry(rtk, ora):
    flat = ora.load_crtscene(SCENE5)
    lights = flat.light_pos.astype(np.float32).copy()
    lights[0] = lights[0] + np.array([-6.0, 3.0, 5.0], np.float32)
    verts = (flat.vertices + np.array([0.3, 0.2, -0.4], np.float32)).astype(np.float32)
    cfg = _cfg(rtk, 6)
    ad = rtk.AdaptiveConfig(min_samples=2, step=2, threshold=0.01, floor=0.01)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    seen = [acc.render_adaptive(cfg, ad)]
    acc.set_lights(lights, flat.light_intensity)
    seen.append(acc.render_adaptive(cfg, ad))
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, dataclasses.replace(flat, light_pos=lights)))
    assert _same_result(seen[-1], fresh.render_adaptive(cfg, ad))
    acc.update_vertices(verts)
    seen.append(acc.render_adaptive(cfg, ad))
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, dataclasses.replace(flat, light_pos=lights, vertices=verts)))
    assert _same_result(seen[-1], fresh.render_adaptive(cfg, ad))
    for a, b in zip(seen, seen[1:]):                                          # no step was a no-op
        assert not np.array_equal(_bits(a[0]), _bits(b[0]))
