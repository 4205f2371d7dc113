"""rtk_denoise_frame on the device against the numpy model of the contract (tests/denoise_model.py), bit for bit: the synthetic
planes at every size and with every combination of the optional planes, 130x70 through one to six iterations, two images in one
call, in place, host against device variant, every setting of RTK_DENOISE_LDS_MAX_STEP, a workspace full of NaNs, and one real
chain render_adaptive -> render_gbuffer -> denoise."""
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_model as dm
from conftest import ROOT, SCENE2

pytestmark = pytest.mark.gpu

GUARD = 64
_PLANES = {}
_MODEL = {}


def _planes(w, h, seed=0):
    if (w, h, seed) not in _PLANES:
        _PLANES[(w, h, seed)] = dm.synthetic(w, h, seed)
    return _PLANES[(w, h, seed)]


def _model(w, h, combo, iterations, seed=0):
    """the model's output for the synthetic planes, computed once and shared"""
    key = (w, h, combo, iterations, seed)
    if key not in _MODEL:
        out = dm.run(_planes(w, h, seed), combo, **dict(dm.PARAMS, iterations=iterations))
        out.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def _cfg(rtk, iterations):
    return rtk.DenoiseConfig(**dict(dm.PARAMS, iterations=iterations))


def _host(rtk, planes, combo, iterations):
    noise, albedo = dm.optional_planes(planes, combo)
    return rtk.denoise(planes["rgb"], planes["normal"], planes["position"], planes["depth"], noise, albedo, _cfg(rtk, iterations))


def _device(rtk, planes, combo, iterations, in_place=False, fill=float("nan"), stream=None):
    """the device variant on torch buffers with guard words behind the output and the workspace -> rgb_out"""
    import torch
    noise, albedo = dm.optional_planes(planes, combo)
    shape = planes["rgb"].shape
    n_images = 1 if len(shape) == 3 else shape[0]
    h, w = shape[-3], shape[-2]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    d = {k: up(a) for k, a in dict(rgb=planes["rgb"], normal=planes["normal"], position=planes["position"], depth=planes["depth"],
                                   noise=noise, albedo=albedo).items()}
    ptr = lambda t: 0 if t is None else t.data_ptr()
    cfg = _cfg(rtk, iterations)
    need = rtk.denoise_workspace_bytes(w, h, n_images, cfg)
    assert need <= 64 * w * h * n_images and need % 16 == 0
    ws = torch.full((need // 4 + GUARD,), fill, dtype=torch.float32, device="cuda")
    assert ws.data_ptr() % 16 == 0
    n = w * h * n_images * 3
    if in_place:
        d_out = torch.cat([d["rgb"].reshape(-1), torch.full((GUARD,), 7.0, dtype=torch.float32, device="cuda")])
        rgb_ptr = d_out.data_ptr()
    else:
        d_out = torch.full((n + GUARD,), 7.0, dtype=torch.float32, device="cuda")
        rgb_ptr = d["rgb"].data_ptr()
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        rtk.denoise_device(w, h, rgb_ptr, ptr(d["normal"]), ptr(d["position"]), ptr(d["depth"]), d_out.data_ptr(), ws.data_ptr(), need,
                           d_noise_ptr=ptr(d["noise"]), d_albedo_ptr=ptr(d["albedo"]), n_images=n_images, cfg=cfg, stream=s.cuda_stream)
    s.synchronize()
    out = d_out.cpu().numpy()
    tail = ws.cpu().numpy()[need // 4:]
    assert (out[n:] == 7).all()
    assert np.array_equal(dm.bits(tail), dm.bits(np.full(GUARD, fill, np.float32)))          # nothing written behind the workspace
    for k in ("normal", "position", "depth", "noise", "albedo") + (() if in_place else ("rgb",)):    # the inputs are inputs
        if d[k] is not None:
            assert np.array_equal(dm.bits(d[k].cpu().numpy()), dm.bits(planes[k]))
    return out[:n].reshape(shape)


def _same(a, b):
    return np.array_equal(dm.bits(a), dm.bits(b))


@pytest.mark.parametrize("combo", dm.COMBOS)
@pytest.mark.parametrize("w,h", dm.SIZES)
def test_synthetic_planes_equal_the_model(rtk, w, h, combo):
    it = dm.ITERATIONS[(w, h)]
    want = _model(w, h, combo, it)
    got = _host(rtk, _planes(w, h), combo, it)
    assert _same(got, want), int((dm.bits(got) != dm.bits(want)).sum())
    assert _same(_device(rtk, _planes(w, h), combo, it), want)


@pytest.mark.parametrize("combo", dm.COMBOS)
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_130x70_through_one_to_six_iterations(rtk, iterations, combo):
    """9 x 5 tiles: the tile at (4, 2) has its halo inside the image at steps 4 and 8; from step 8 on taps leave the frame"""
    want = _model(130, 70, combo, iterations)
    got = _device(rtk, _planes(130, 70), combo, iterations)
    assert _same(got, want), int((dm.bits(got) != dm.bits(want)).sum())
    hit = _planes(130, 70)["hit"]
    assert (dm.bits(want) != dm.bits(_planes(130, 70)["rgb"])).any(-1)[hit].all()            # (the case shows something)


@pytest.mark.parametrize("combo", dm.COMBOS)
def test_two_images_in_one_call_are_two_calls(rtk, combo):
    """no bleed across the image border: 37x19 has partial tiles, and image 1 begins in the middle of what a tile's halo would reach"""
    both = dm.stack([_planes(37, 19, 0), _planes(37, 19, 1)])
    got = _device(rtk, both, combo, 5)
    assert got.shape == (2, 19, 37, 3)
    for i in (0, 1):
        assert _same(got[i], _model(37, 19, combo, 5, seed=i)), i
    assert not _same(got[0], got[1])
    assert _same(_host(rtk, both, combo, 5), got)


def test_in_place_host_device_and_a_second_call_agree(rtk):
    import torch
    planes = _planes(70, 36)
    for combo in dm.COMBOS:
        want = _model(70, 36, combo, 5)
        assert _same(_device(rtk, planes, combo, 5, in_place=True), want), combo
        assert _same(_device(rtk, planes, combo, 5, stream=torch.cuda.Stream()), want), combo
        assert _same(_host(rtk, planes, combo, 5), want) and _same(_host(rtk, planes, combo, 5), want), combo
    # one iteration needs 48 B per pixel and writes rgb_out straight away
    assert _same(_device(rtk, planes, "noise+albedo", 1, in_place=True), _model(70, 36, "noise+albedo", 1))


def test_what_the_workspace_held_changes_nothing(rtk):
    planes = _planes(70, 36)
    want = _model(70, 36, "noise+albedo", 5)
    for fill in (float("nan"), 0.0, -3.0e38):
        assert _same(_device(rtk, planes, "noise+albedo", 5, fill=fill), want), fill


def test_every_setting_of_the_lds_knob_gives_the_same_bits(rtk, tmp_path):
    """RTK_DENOISE_LDS_MAX_STEP = 0 (every step reads global memory), unset (the default) and 8 (steps 1..8 staged, the largest
    tile LDS holds), each in a fresh child process: the knob is read once."""
    planes, params = dm.knob_case()
    want = dm.denoise(planes["rgb"], planes["normal"], planes["position"], planes["depth"], planes["noise"], planes["albedo"], **params)
    child = os.path.join(ROOT, "tests", "denoise_child.py")
    children = []
    for setting in ("0", None, "8"):                                  # (the three side by side: most of a child's time is its imports)
        env = {k: v for k, v in os.environ.items() if k != "RTK_DENOISE_LDS_MAX_STEP"}
        if setting is not None:
            env["RTK_DENOISE_LDS_MAX_STEP"] = setting
        out = str(tmp_path / f"knob_{setting}.npy")
        children.append((setting, out, subprocess.Popen([sys.executable, child, out], env=env, stdout=subprocess.PIPE,
                                                        stderr=subprocess.STDOUT, text=True)))
    for setting, out, proc in children:
        log, _ = proc.communicate()
        assert proc.returncode == 0, (setting, log)
        got = np.load(out)
        assert _same(got, want), (setting, int((dm.bits(got) != dm.bits(want)).sum()))


def test_render_adaptive_then_gbuffer_then_denoise(rtk):
    """hw15/scene2 at 70x36 and 40 degrees: the noise plane of an adaptive render and the guides of a g-buffer, as a caller chains them"""
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))
    cfg = rtk.RenderConfig(width=70, height=36, spp=8, trace_mode=rtk.TRACE_STREAM, diffuse_rays=2, max_ray_depth=2, fov_degrees=40.0)
    rgb, samples, noise, _ = acc.render_adaptive(cfg, rtk.AdaptiveConfig(min_samples=2, step=2, threshold=0.05, floor=0.01))
    gb = acc.render_gbuffer(cfg, sample=0, planes=("depth", "position", "normal", "albedo"))
    normal, position, depth, albedo = gb["normal"][0], gb["position"][0], gb["depth"][0], gb["albedo"][0]
    want = dm.denoise(rgb, normal, position, depth, noise, albedo, **dm.PARAMS)
    hit = depth >= 0
    changed = (dm.bits(want) != dm.bits(rgb)).any(-1)
    assert hit.sum() > 70 * 36 // 4 and changed[hit].sum() * 2 > hit.sum()                    # otherwise the case shows nothing
    assert not changed[~hit].any()
    got = rtk.denoise(rgb, normal, position, depth, noise, albedo, rtk.DenoiseConfig(**dm.PARAMS))
    assert _same(got, want), int((dm.bits(got) != dm.bits(want)).sum())
