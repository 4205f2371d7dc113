"""rtk_render_frame_noise[_device] and rtk_debug_noise_fallbacks without a GPU: the symbols, the Python methods, and the order of the
argument checks (a NULL accel / p / rgb / noise, what a frame refuses, the trace mode, spp, the progressive fields, collect_stats,
world_size, the pixel count; then the missing device) on an accel that never saw a device and stays usable."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENE5

SYMBOLS = ("rtk_render_frame_noise", "rtk_render_frame_noise_device", "rtk_debug_noise_fallbacks")
METHODS = ("render_frame_noise", "render_frame_noise_device", "noise_fallbacks")


def _accel(rtk):
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_frame_noise_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    assert re.search(r"#define RTK_ABI_VERSION 4\b", _header())
    for name in METHODS:
        assert hasattr(rtk.KdTreeSimdAccel, name)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rtk_\w+)\s*\(", text))) == sorted(rtk.ABI_SYMBOLS)


def _calls(rtk):
    L = rtk.lib()
    rgb = np.full((8, 8, 3), 7.0, np.float32)
    noise = np.full((8, 8), 7.0, np.float32)
    missing = object()

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def host(h, p, out=missing, nz=missing):
        return L.rtk_render_frame_noise(h, ref(p), rgb.ctypes.data if out is missing else out, noise.ctypes.data if nz is missing else nz, None)

    def dev(h, p, out=missing, nz=missing):          # (never dereferenced: every call here is refused, or finds no device)
        return L.rtk_render_frame_noise_device(h, ref(p), rgb.ctypes.data if out is missing else out,
                                               noise.ctypes.data if nz is missing else nz, None)

    return L, (host, dev), (rgb, noise)


def test_frame_noise_argument_errors_in_their_order(rtk):
    acc = _accel(rtk)
    L, calls, outs = _calls(rtk)
    INVALID = rtk.RTK_ERR_INVALID

    def cfg(**kw):
        kw.setdefault("spp", 8)
        kw.setdefault("width", 8)
        kw.setdefault("height", 8)
        return rtk.RenderConfig(**kw).to_c()

    # every later refusal, from the last of the list to the first: a call that is wrong in all of the ways from k on names way k
    later = [
        ("too many pixels", dict(width=65536, height=65536)),
        ("not sharded", dict(world_size=2)),
        ("statistics", dict(collect_stats=1)),
        ("not progressive", dict(sample_begin=1, sample_count=1)),
        ("spp >= 2", dict(spp=1, sample_begin=0, sample_count=0)),
        ("RTK_TRACE_AUTO or RTK_TRACE_STREAM", dict(trace_mode=rtk.TRACE_GROUP4)),
    ]
    worst = dict()
    for _, c_bad in later:
        worst.update(c_bad)
    for call in calls:
        # 1. a NULL accel, p, rgb or noise, whatever else is wrong
        assert call(None, cfg()) == INVALID
        assert call(acc._h, None) == INVALID
        assert call(acc._h, cfg(), None) == INVALID
        assert call(acc._h, cfg(), nz=None) == INVALID
        for c in (cfg(spp=0), cfg(**worst)):
            assert call(acc._h, c, None) == INVALID and "null" in L.rtk_last_error().decode()
            assert call(acc._h, c, nz=None) == INVALID and "null" in L.rtk_last_error().decode()
        # 2. what a frame refuses for *p, whatever else is wrong
        for bad in (dict(spp=0), dict(width=70000), dict(trace_mode=99), dict(max_ray_depth=17), dict(diffuse_rays=-1), dict(sample_begin=8),
                    dict(sample_begin=4, sample_count=5), dict(world_size=2, rank=2)):
            kw = dict(worst)
            kw.update(bad)
            assert call(acc._h, cfg(**kw)) == INVALID
            msg = L.rtk_last_error().decode()
            assert not any(w in msg for w, _ in later), msg
        # 3. the list of rtk.h: wrong in ways k, k + 1, ... reports way k
        ckw = dict()
        for word, c_bad in later:
            ckw.update(c_bad)
            assert call(acc._h, cfg(**ckw)) == INVALID
            assert word in L.rtk_last_error().decode(), (word, L.rtk_last_error().decode())
        # 4. each alone, in all its forms
        alone = [
            ("RTK_TRACE_AUTO or RTK_TRACE_STREAM", [dict(trace_mode=m) for m in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_GROUP4, rtk.TRACE_GROUP8,
                                                         rtk.TRACE_GROUP16, rtk.TRACE_TWOPASS)]),
            ("spp >= 2", [dict(spp=1)]),
            ("not progressive", [dict(sample_begin=2, sample_count=2), dict(sample_count=8), dict(sample_count=3)]),
            ("statistics", [dict(collect_stats=1), dict(collect_stats=2)]),
            ("not sharded", [dict(world_size=2), dict(world_size=4, rank=3)]),
            ("too many pixels", [dict(width=65536, height=65536), dict(width=65536, height=32769)]),
        ]
        for word, cs in alone:
            for c_bad in cs:
                assert call(acc._h, cfg(**c_bad)) == INVALID, (word, c_bad)
                assert word in L.rtk_last_error().decode(), (word, L.rtk_last_error().decode())
    for out in outs:
        assert (out == 7).all()
    assert acc.noise_fallbacks() == 0 and acc.counter_fills() == 0


def test_noise_fallbacks_needs_no_device_and_starts_at_zero(rtk):
    acc = _accel(rtk)
    assert acc.noise_fallbacks() == 0
    L = rtk.lib()
    n = ctypes.c_uint64(5)
    assert L.rtk_debug_noise_fallbacks(acc._h, ctypes.byref(n)) == rtk.RTK_OK and n.value == 0
    assert L.rtk_debug_noise_fallbacks(None, ctypes.byref(n)) == rtk.RTK_ERR_INVALID
    assert L.rtk_debug_noise_fallbacks(acc._h, None) == rtk.RTK_ERR_INVALID


def test_after_validation_the_answer_is_no_device_and_the_accel_stays_usable(rtk):
    acc = _accel(rtk)
    nodes = acc.tree_info().n_nodes
    cam = [x.copy() for x in acc.camera()]
    cfg = rtk.RenderConfig(width=8, height=8, spp=4)
    # refused calls first: they change nothing
    for bad in (rtk.RenderConfig(width=8, height=8, spp=1), rtk.RenderConfig(width=8, height=8, spp=4, trace_mode=rtk.TRACE_GROUP4),
                rtk.RenderConfig(width=8, height=8, spp=4, collect_stats=1)):
        with pytest.raises(rtk.RtkError) as e:
            acc.render_frame_noise(bad)
        assert e.value.code == rtk.RTK_ERR_INVALID
    assert acc.counter_fills() == 0 and acc.noise_fallbacks() == 0
    if rtk.device_count() > 0:          # a device is present: the valid call goes through (the rest: tests/test_gpu_frame_noise.py)
        rgb, noise, cn = acc.render_frame_noise(cfg)
        assert rgb.shape == (8, 8, 3) and noise.shape == (8, 8) and cn["primary"] == 4 * 64
    else:
        with pytest.raises(rtk.RtkError) as e:
            acc.render_frame_noise(cfg)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            acc.render_frame_noise_device(cfg, 16, 32)          # (never dereferenced: there is no device to launch on)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        assert acc.counter_fills() == 0 and acc.noise_fallbacks() == 0
    # still usable: the host-side queries answer as before
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cam, acc.camera()))
    assert acc.tree_info().n_nodes == nodes
    acc.set_camera(cam[0] + np.float32(1.0), cam[1])
    assert acc.camera()[0].tobytes() == (cam[0] + np.float32(1.0)).tobytes()
