"""rtk_render_adaptive[_device] without a GPU: the symbols, the layout of rtk_adaptive_params, and the order of the argument checks (a
NULL accel / p / ap / rgb, what a frame refuses, the trace mode, spp, the progressive fields, collect_stats, world_size, min_samples,
step, threshold, floor; then the missing device) on an accel that never saw a device and stays usable."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENE5

SYMBOLS = ("rtk_render_adaptive", "rtk_render_adaptive_device")
FIELDS = ("min_samples", "step", "threshold", "floor")
INF, NAN = float("inf"), float("nan")


def _accel(rtk):
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_adaptive_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    assert re.search(r"#define RTK_ABI_VERSION 4\b", _header())
    for name in ("render_adaptive", "render_adaptive_device"):
        assert hasattr(rtk.KdTreeSimdAccel, name)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rtk_\w+)\s*\(", text))) == sorted(rtk.ABI_SYMBOLS)


def test_adaptive_params_are_16_bytes_field_by_field(rtk):
    assert ctypes.sizeof(rtk.AdaptiveParams) == 16
    assert [n for n, _ in rtk.AdaptiveParams._fields_] == list(FIELDS)
    for i, name in enumerate(FIELDS):
        f = getattr(rtk.AdaptiveParams, name)
        assert (f.offset, f.size) == (4 * i, 4), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_adaptive_params;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == list(FIELDS)
    assert re.findall(r"(\w+)\s+\w+\s*;", body) == ["int32_t", "int32_t", "float", "float"]
    c = rtk.AdaptiveConfig(min_samples=3, step=5, threshold=0.25, floor=0.5).to_c()
    assert (c.min_samples, c.step, c.threshold, c.floor) == (3, 5, 0.25, 0.5)


def _calls(rtk):
    L = rtk.lib()
    rgb = np.full((8, 8, 3), 7.0, np.float32)
    samples = np.full((8, 8), 7, np.uint32)
    noise = np.full((8, 8), 7.0, np.float32)

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def host(h, p, ap, out=rgb.ctypes.data):
        return L.rtk_render_adaptive(h, ref(p), ref(ap), out, samples.ctypes.data, noise.ctypes.data, None)

    def dev(h, p, ap, out=rgb.ctypes.data):          # (never dereferenced: every call here is refused, or finds no device)
        return L.rtk_render_adaptive_device(h, ref(p), ref(ap), out, samples.ctypes.data, noise.ctypes.data, None)

    return L, (host, dev), (rgb, samples, noise)


def test_adaptive_argument_errors_in_their_order(rtk):
    acc = _accel(rtk)
    L, calls, outs = _calls(rtk)
    INVALID = rtk.RTK_ERR_INVALID

    def cfg(**kw):
        kw.setdefault("spp", 8)
        return rtk.RenderConfig(width=8, height=8, **kw).to_c()

    def ad(**kw):
        base = dict(min_samples=2, step=2, threshold=0.1, floor=0.01)
        base.update(kw)
        return rtk.AdaptiveConfig(**base).to_c()

    # every later refusal, from the last of the list to the first: a call that is wrong in all of the ways from k on names way k
    later = [
        ("floor", dict(), dict(floor=0.0)),
        ("threshold", dict(), dict(threshold=-1.0)),
        ("step", dict(), dict(step=0)),
        ("min_samples", dict(), dict(min_samples=1)),
        ("not sharded", dict(world_size=2), dict()),
        ("statistics", dict(collect_stats=1), dict()),
        ("not progressive", dict(sample_begin=1, sample_count=1), dict()),
        ("spp >= 2", dict(spp=1, sample_begin=0, sample_count=0), dict()),
        ("RTK_TRACE_AUTO or RTK_TRACE_STREAM", dict(trace_mode=rtk.TRACE_GROUP4), dict()),
    ]
    for call in calls:
        # 1. a NULL accel, p, ap or rgb
        assert call(None, cfg(), ad()) == INVALID
        assert call(acc._h, None, ad()) == INVALID
        assert call(acc._h, cfg(), None) == INVALID
        assert call(acc._h, cfg(), ad(), None) == INVALID
        # 2. what a frame refuses for *p, whatever else is wrong
        for bad in (cfg(spp=0), rtk.RenderConfig(width=70000, height=8, spp=8).to_c(), cfg(trace_mode=99), cfg(max_ray_depth=17),
                    cfg(diffuse_rays=-1), cfg(sample_begin=8), cfg(sample_begin=4, sample_count=5), cfg(world_size=2, rank=2)):
            assert call(acc._h, bad, ad(min_samples=0, step=0, threshold=NAN, floor=NAN)) == INVALID
            msg = L.rtk_last_error().decode()
            assert not any(w in msg for w, _, _ in later), msg
        # 3. the list of rtk.h: wrong in ways k, k + 1, ... reports way k
        ckw, akw = dict(), dict()
        for word, c_bad, a_bad in later:
            ckw.update(c_bad)
            akw.update(a_bad)
            assert call(acc._h, cfg(**ckw), ad(**akw)) == INVALID
            assert word in L.rtk_last_error().decode(), (word, L.rtk_last_error().decode())
        # 4. each alone, in all its forms
        alone = [
            ("RTK_TRACE_AUTO or RTK_TRACE_STREAM", [dict(trace_mode=m) for m in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_GROUP4, rtk.TRACE_GROUP8,
                                                         rtk.TRACE_GROUP16, rtk.TRACE_TWOPASS)], [dict()]),
            ("spp >= 2", [dict(spp=1)], [dict()]),
            ("not progressive", [dict(sample_begin=2, sample_count=2), dict(sample_count=8), dict(sample_count=3)], [dict()]),
            ("statistics", [dict(collect_stats=1), dict(collect_stats=2)], [dict()]),
            ("not sharded", [dict(world_size=2), dict(world_size=4, rank=3)], [dict()]),
            ("min_samples", [dict()], [dict(min_samples=1), dict(min_samples=0), dict(min_samples=-5), dict(min_samples=9)]),
            ("step", [dict()], [dict(step=0), dict(step=-1)]),
            ("threshold", [dict()], [dict(threshold=-1e-30), dict(threshold=INF), dict(threshold=-INF), dict(threshold=NAN)]),
            ("floor", [dict()], [dict(floor=0.0), dict(floor=-0.0), dict(floor=-1.0), dict(floor=INF), dict(floor=NAN)]),
        ]
        for word, cs, as_ in alone:
            for c_bad in cs:
                for a_bad in as_:
                    assert call(acc._h, cfg(**c_bad), ad(**a_bad)) == INVALID, (word, c_bad, a_bad)
                    assert word in L.rtk_last_error().decode(), (word, L.rtk_last_error().decode())
    for out in outs:
        assert (out == 7).all()


def test_after_validation_the_answer_is_no_device_and_the_accel_stays_usable(rtk):
    acc = _accel(rtk)
    nodes = acc.tree_info().n_nodes
    cam = [x.copy() for x in acc.camera()]
    cfg = rtk.RenderConfig(width=8, height=8, spp=4)
    ok = rtk.AdaptiveConfig(min_samples=2, step=1, threshold=0.0, floor=1.0)
    # refused calls first: they change nothing
    for bad in (rtk.AdaptiveConfig(min_samples=5), rtk.AdaptiveConfig(min_samples=2, step=0),
                rtk.AdaptiveConfig(min_samples=2, threshold=-1.0), rtk.AdaptiveConfig(min_samples=2, floor=0.0)):
        with pytest.raises(rtk.RtkError) as e:
            acc.render_adaptive(cfg, bad)
        assert e.value.code == rtk.RTK_ERR_INVALID
    assert acc.counter_fills() == 0
    if rtk.device_count() > 0:          # a device is present: the valid call goes through (the rest: tests/test_gpu_adaptive.py)
        rgb, samples, noise, cn = acc.render_adaptive(cfg, ok)
        assert rgb.shape == (8, 8, 3) and samples.shape == (8, 8) and noise.shape == (8, 8)
        assert set(np.unique(samples)) <= {2, 3, 4} and cn["primary"] == int(samples.sum())
    else:
        with pytest.raises(rtk.RtkError) as e:
            acc.render_adaptive(cfg, ok)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            acc.render_adaptive_device(cfg, ok, 16, 32, 48)          # (never dereferenced: there is no device to launch on)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        assert acc.counter_fills() == 0
    # still usable: the host-side queries answer as before
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cam, acc.camera()))
    assert acc.tree_info().n_nodes == nodes
    acc.set_camera(cam[0] + np.float32(1.0), cam[1])
    assert acc.camera()[0].tobytes() == (cam[0] + np.float32(1.0)).tobytes()
