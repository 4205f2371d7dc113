"""rtk_render_gbuffer_specular[_device] without a GPU: the symbols, the layout of rtk_gbuffer_specular and its Python mirror, and
the order of the argument checks -- rtk_render_gbuffer's, with "all twelve planes NULL" in the place of "all eight" -- on an accel
that never saw a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENE5

SYMBOLS = ("rtk_render_gbuffer_specular", "rtk_render_gbuffer_specular_device")
PLANES = ("depth", "position", "normal", "surface_position", "surface_normal", "albedo", "bary", "tri", "mesh", "material", "bounces",
          "last_ray")


def _accel(rtk):
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    for name in ("render_gbuffer_specular", "render_gbuffer_specular_device"):
        assert hasattr(rtk.KdTreeSimdAccel, name)


def test_struct_is_96_bytes_field_by_field(rtk):
    assert ctypes.sizeof(rtk.SpecularGBuffer) == 96
    assert [n for n, _ in rtk.SpecularGBuffer._fields_] == list(PLANES)
    for i, name in enumerate(PLANES):
        f = getattr(rtk.SpecularGBuffer, name)
        assert (f.offset, f.size) == (8 * i, 8), name
    # the header declares the same planes in the same order
    body = re.search(r"typedef struct \{([^}]*)\} rtk_gbuffer_specular;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*\s*(\w+)", body) == list(PLANES)
    assert list(rtk.SPECULAR_GBUFFER_PLANES) == list(PLANES)
    assert sum(int(np.prod(s, dtype=int)) * 4 for s, _ in rtk.SPECULAR_GBUFFER_PLANES.values()) == 112    # bytes per pixel of all twelve
    assert {n: d for n, (_, d) in rtk.SPECULAR_GBUFFER_PLANES.items() if d is np.uint32}.keys() == {"tri", "mesh", "material", "bounces"}


def test_argument_errors_in_their_order(rtk):
    acc = _accel(rtk)
    L = rtk.lib()
    views = np.zeros((2, 12), np.float32)
    depth = np.full((2, 8, 8), 7.0, np.float32)
    V = views.ctypes.data
    some = rtk.SpecularGBuffer(bounces=depth.ctypes.data)
    none = rtk.SpecularGBuffer()
    INVALID, OK = rtk.RTK_ERR_INVALID, rtk.RTK_OK

    def host(h, p, sample, v, n, o):
        return L.rtk_render_gbuffer_specular(h, ctypes.byref(p) if p is not None else None, sample, v, n,
                                             ctypes.byref(o) if o is not None else None)

    def dev(h, p, sample, v, n, o):
        return L.rtk_render_gbuffer_specular_device(h, ctypes.byref(p) if p is not None else None, sample, v, n,
                                                    ctypes.byref(o) if o is not None else None, None)

    def cfg(**kw):
        return rtk.RenderConfig(width=8, height=8, **kw).to_c()

    for call in (host, dev):
        # 1. a NULL accel, p or out
        assert call(None, cfg(), 0, V, 2, some) == INVALID
        assert call(acc._h, None, 0, V, 2, some) == INVALID
        assert call(acc._h, cfg(), 0, V, 2, None) == INVALID
        # 2. what a frame refuses for *p, whatever else is wrong or empty
        for bad in (cfg(spp=0), rtk.RenderConfig(width=70000, height=8).to_c(), cfg(trace_mode=99), cfg(max_ray_depth=17),
                    cfg(max_ray_depth=-1), cfg(diffuse_rays=-1), cfg(spp=2, sample_begin=2), cfg(world_size=2, rank=2)):
            assert call(acc._h, bad, 0, V, 2, some) == INVALID
            assert call(acc._h, bad, 0, None, 0, none) == INVALID
            assert "sample must be in" not in L.rtk_last_error().decode()
        # 3. the sample, before anything about views or planes
        for p, s in ((cfg(), 1), (cfg(), -1), (cfg(spp=4), 4)):
            assert call(acc._h, p, s, None, 0, none) == INVALID
            assert "sample must be in [0, spp)" in L.rtk_last_error().decode()
        # 4. world_size > 1, collect_stats != 0, n_views < 0 -- before NULL views and before "no plane"
        for p, n in ((cfg(world_size=2), 2), (cfg(collect_stats=1), 2), (cfg(), -1)):
            assert call(acc._h, p, 0, None, n, none) == INVALID
            msg = L.rtk_last_error().decode()
            assert "n_views must be 1" not in msg and "no plane" not in msg, msg
        # 5. NULL views with n_views != 1 -- before "no plane", and before n_views == 0
        for n in (0, 2):
            assert call(acc._h, cfg(), 0, None, n, none) == INVALID
            assert "n_views must be 1" in L.rtk_last_error().decode()
        # 6. all twelve planes NULL, with or without views, and before n_views == 0
        for v, n in ((V, 2), (None, 1), (V, 0)):
            assert call(acc._h, cfg(), 0, v, n, none) == INVALID
            assert "no plane" in L.rtk_last_error().decode() and "rtk_gbuffer_specular" in L.rtk_last_error().decode()
        # every single plane counts as "a plane"
        for name in PLANES:
            assert call(acc._h, cfg(), 0, V, 0, rtk.SpecularGBuffer(**{name: depth.ctypes.data})) == OK, name
        # 7. then n_views == 0: nothing to do, device or not, at every depth the frame accepts
        assert call(acc._h, cfg(), 0, V, 0, some) == OK
        assert call(acc._h, cfg(spp=4, max_ray_depth=0), 3, V, 0, some) == OK
        assert call(acc._h, cfg(max_ray_depth=16), 0, V, 0, some) == OK
    # behind that, and before it looks for a device, the device variant refuses planes and views that are not 4-byte aligned
    odd = rtk.SpecularGBuffer(last_ray=depth.ctypes.data + 2)
    assert dev(acc._h, cfg(), 0, V, 0, odd) == OK
    for v, o in ((V, odd), (V + 1, some)):
        assert dev(acc._h, cfg(), 0, v, 2, o) == INVALID
        assert "4-byte aligned" in L.rtk_last_error().decode()
    assert (depth == 7.0).all()


def test_python_door_validates_its_arguments(rtk):
    acc = _accel(rtk)
    cfg = rtk.RenderConfig(width=8, height=8)
    out = acc.render_gbuffer_specular(cfg, views=np.zeros((0, 12), np.float32), planes=("depth", "bounces", "last_ray"))
    assert set(out) == {"depth", "bounces", "last_ray"} and out["last_ray"].shape == (0, 8, 8, 6) and out["bounces"].dtype == np.uint32
    with pytest.raises(ValueError):
        acc.render_gbuffer_specular(cfg, planes=("depth", "colour"))
    with pytest.raises(ValueError):
        acc.render_gbuffer_specular(cfg, views=np.zeros((2, 11), np.float32))
    with pytest.raises(ValueError):
        acc.render_gbuffer_specular_device(cfg, {"shade": 16})
    with pytest.raises(rtk.RtkError) as e:
        acc.render_gbuffer_specular(cfg, planes=())
    assert e.value.code == rtk.RTK_ERR_INVALID


def test_without_a_device_the_last_answer_is_no_device(rtk):
    acc = _accel(rtk)
    cfg = rtk.RenderConfig(width=8, height=8, spp=4)
    views = np.zeros((2, 12), np.float32)
    views[:, 3] = views[:, 7] = views[:, 11] = 1.0
    cam = [x.copy() for x in acc.camera()]
    if rtk.device_count() > 0:          # a device is present: the call that would be refused last goes through (the rest: tests/test_gpu_gbuffer_specular.py)
        out = acc.render_gbuffer_specular(cfg, sample=3, views=views, planes=("depth", "bounces"))
        assert out["depth"].shape == (2, 8, 8) and out["bounces"].dtype == np.uint32
        assert all(a.tobytes() == b.tobytes() for a, b in zip(cam, acc.camera())) and acc.counter_fills() == 0
        return
    for kw in (dict(), dict(views=views), dict(sample=3, planes=("last_ray",))):
        with pytest.raises(rtk.RtkError) as e:
            acc.render_gbuffer_specular(cfg, **kw)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    for kw in (dict(), dict(d_views_ptr=views.ctypes.data, n_views=2)):     # (never dereferenced: there is no device to launch on)
        with pytest.raises(rtk.RtkError) as e:
            acc.render_gbuffer_specular_device(cfg, {"depth": 16, "bounces": 32}, **kw)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cam, acc.camera()))
    assert acc.counter_fills() == 0
