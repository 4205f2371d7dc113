"""rtk_temporal_accumulate_clamped[_device] without a GPU: the symbols, the layout of rtk_temporal_clamp on both sides of ctypes,
the order of the argument checks (a NULL p / k / cur / out; the parameters; radius, gamma, history_keep; the planes and families of
the plain call; the two aliasing refusals; the device variant's alignment; then the missing device), and that clamp=None reaches
the plain symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("rtk_temporal_accumulate_clamped", "rtk_temporal_accumulate_clamped_device")
CLAMP_FIELDS = (("radius", 0, 4, "int32_t"), ("gamma", 4, 4, "float"), ("history_keep", 8, 4, "float"), ("reserved", 12, 4, "int32_t"))
INF, NAN = float("inf"), float("nan")
W, H = 8, 6


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_clamped_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
        assert getattr(rtk.lib(), name).argtypes is not None
    assert rtk.abi_version() == 4
    for name in ("ClampConfig", "TemporalClamp"):
        assert hasattr(rtk, name)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, text)


def test_the_clamp_struct_is_16_bytes_field_by_field(rtk):
    assert ctypes.sizeof(rtk.TemporalClamp) == 16
    assert [n for n, _ in rtk.TemporalClamp._fields_] == [n for n, _, _, _ in CLAMP_FIELDS]
    for name, offset, size, _ in CLAMP_FIELDS:
        f = getattr(rtk.TemporalClamp, name)
        assert (f.offset, f.size) == (offset, size), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_temporal_clamp;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+)\s*;", body) == [(t, n) for n, _, _, t in CLAMP_FIELDS]
    d = rtk.ClampConfig()
    assert (d.radius, d.gamma, d.history_keep) == (1, 1.0, 1.0)
    c = rtk.ClampConfig(radius=3, gamma=1.5, history_keep=0.25).to_c()
    assert (c.radius, c.gamma, c.history_keep, c.reserved) == (3, 1.5, 0.25, 0)


def _setup(rtk):
    L = rtk.lib()
    mk3 = lambda: np.full((H, W, 3), 7.0, np.float32)
    mk1 = lambda: np.full((H, W), 7.0, np.float32)
    cur = dict(rgb=mk3(), noise=mk1(), position=mk3(), normal=mk3(), depth=mk1(), mesh=np.full((H, W), 7, np.uint32))
    prev = dict(rgb=mk3(), noise=mk1(), length=mk1(), position=mk3(), normal=mk3(), depth=mk1(), mesh=np.full((H, W), 7, np.uint32),
                view=np.full(12, 7.0, np.float32))
    out = dict(rgb=mk3(), noise=mk1(), length=mk1())

    def params(**kw):
        size = (kw.pop("width", W), kw.pop("height", H))
        return rtk.TemporalConfig(**kw).to_c(*size)

    def clamp(radius=2, gamma=1.0, history_keep=0.5):
        return rtk.TemporalClamp(radius, gamma, history_keep, 0x5A5A5A5A)

    def struct(cls, planes, kw):
        d = {n: planes[n].ctypes.data for n, _ in cls._fields_}
        d.update(kw)
        return cls(*(d[n] for n, _ in cls._fields_))

    frame = lambda **kw: struct(rtk.TemporalFrame, cur, kw)
    history = lambda **kw: struct(rtk.TemporalHistory, prev, kw)
    outputs = lambda **kw: struct(rtk.TemporalOutputs, out, kw)

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def host(p, k, c, q, o):
        return L.rtk_temporal_accumulate_clamped(ref(p), ref(k), ref(c), ref(q), ref(o))

    def dev(p, k, c, q, o):                            # (never dereferenced: refused, or no device)
        return L.rtk_temporal_accumulate_clamped_device(ref(p), ref(k), ref(c), ref(q), ref(o), None)

    return L, params, clamp, frame, history, outputs, (host, dev), (cur, prev, out)


def test_clamped_argument_errors_in_their_order(rtk):
    L, params, clamp, frame, history, outputs, calls, arrays = _setup(rtk)
    cur, prev, out = arrays
    INVALID = rtk.RTK_ERR_INVALID
    msg = lambda: L.rtk_last_error().decode()
    odd = lambda a: a.ctypes.data + 2
    alias_rgb, alias_noise = dict(rgb=cur["rgb"].ctypes.data), dict(noise=cur["noise"].ctypes.data)
    for call in calls:
        # 1. a NULL p, k, cur or out, whatever else is wrong
        bad_p, bad_k = params(max_history=0), clamp(radius=0)
        assert call(None, bad_k, frame(rgb=None), history(), outputs()) == INVALID and "null params" in msg()
        assert call(bad_p, None, frame(rgb=None), history(), outputs()) == INVALID and "null params" in msg()
        assert call(bad_p, bad_k, None, history(), outputs()) == INVALID and "null params" in msg()
        assert call(bad_p, bad_k, frame(rgb=None), None, None) == INVALID and "null params" in msg()
        # 2. the parameters before the clamp
        for word, bad in (("max_history", dict(max_history=0)), ("fov_degrees", dict(fov_degrees=NAN)), ("width must", dict(width=0))):
            assert call(params(**bad), clamp(radius=0, gamma=NAN, history_keep=NAN), frame(rgb=None), history(), outputs()) == INVALID
            assert word in msg(), (word, msg())
        # 3. to 5. radius, gamma, history_keep, in that order, before the planes; alone in all their forms, and the ends of the ranges
        assert call(params(), clamp(0, NAN, NAN), frame(rgb=None), history(), outputs(**alias_rgb)) == INVALID and "radius" in msg()
        assert call(params(), clamp(1, NAN, NAN), frame(rgb=None), history(), outputs(**alias_rgb)) == INVALID and "gamma" in msg()
        assert call(params(), clamp(1, 1.0, NAN), frame(rgb=None), history(), outputs(**alias_rgb)) == INVALID and "history_keep" in msg()
        for v in (0, -1, 4, 1 << 30):
            assert call(params(), clamp(radius=v), frame(), history(), outputs()) == INVALID and "radius" in msg(), v
        for v in (-1.0, -1e-30, INF, -INF, NAN):
            assert call(params(), clamp(gamma=v), frame(), history(), outputs()) == INVALID and "gamma" in msg(), v
        for v in (-1e-30, 1.0001, INF, -INF, NAN):
            assert call(params(), clamp(history_keep=v), frame(), history(), outputs()) == INVALID and "history_keep" in msg(), v
        # 6. the plane and family checks of the plain call, in its order, before the aliasing
        assert call(params(), clamp(), frame(depth=None, noise=None), history(rgb=None), outputs(**alias_rgb)) == INVALID
        assert "of the new frame" in msg()
        assert call(params(), clamp(), frame(noise=None), history(rgb=None), outputs(length=None)) == INVALID and "of the outputs" in msg()
        assert call(params(), clamp(), frame(noise=None, mesh=None), history(view=None), outputs(**alias_rgb)) == INVALID
        assert "of the history" in msg()
        assert call(params(), clamp(), frame(mesh=None), history(noise=None), outputs(**alias_rgb)) == INVALID and "noise planes" in msg()
        assert call(params(), clamp(), frame(), history(mesh=None), outputs(**alias_rgb)) == INVALID and "mesh planes" in msg()
        # 7. the aliasing refusals, rgb first, both before the alignment
        for q in (history(), None):
            assert call(params(), clamp(), frame(position=odd(cur["position"])), q, outputs(**alias_rgb, **alias_noise)) == INVALID
            assert "out->rgb" in msg(), msg()
            assert call(params(), clamp(), frame(position=odd(cur["position"])), q, outputs(**alias_noise)) == INVALID
            assert "out->noise" in msg(), msg()
    host, dev = calls
    # 8. the device variant alone: the alignment
    for name in ("rgb", "noise", "position", "normal", "depth", "mesh"):
        assert dev(params(), clamp(), frame(**{name: odd(cur[name])}), history(), outputs()) == INVALID and "4-byte" in msg(), name
    for name in ("rgb", "noise", "length", "position", "normal", "depth", "mesh"):
        assert dev(params(), clamp(), frame(), history(**{name: odd(prev[name])}), outputs()) == INVALID and "4-byte" in msg(), name
    for name in ("rgb", "noise", "length"):
        assert dev(params(), clamp(), frame(), history(), outputs(**{name: odd(out[name])})) == INVALID and "4-byte" in msg(), name
    for a in list(cur.values()) + list(prev.values()) + list(out.values()):
        assert (a == 7).all()


def test_after_validation_the_answer_is_no_device(rtk):
    L, params, clamp, frame, history, outputs, (host, dev), (cur, prev, out) = _setup(rtk)
    none = dict(noise=None, mesh=None)
    if rtk.device_count() > 0:          # a device is present: the valid host call goes through (the rest: tests/test_gpu_temporal_clamp.py)
        assert host(params(), clamp(), frame(), None, outputs()) == rtk.RTK_OK
        assert np.array_equal(out["rgb"], cur["rgb"]) and np.array_equal(out["noise"], cur["noise"]) and (out["length"] == 1).all()
    else:
        for call in (host, dev):
            assert call(params(), clamp(), frame(), history(), outputs()) == rtk.RTK_ERR_NO_DEVICE
            assert call(params(), clamp(), frame(), None, outputs()) == rtk.RTK_ERR_NO_DEVICE
            assert call(params(), clamp(), frame(**none), history(**none), outputs(noise=None)) == rtk.RTK_ERR_NO_DEVICE
            # the ends of the three ranges
            for k in (clamp(1, 0.0, 0.0), clamp(3, 3.0e38, 1.0)):
                assert call(params(), k, frame(), history(), outputs()) == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            rtk.temporal_accumulate(dict(cur), dict(prev, view=(prev["view"][:3], prev["view"][3:])), clamp=rtk.ClampConfig())
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:         # (never dereferenced: there is no device)
            rtk.temporal_accumulate_device(W, H, dict(rgb=16, position=32, normal=48, depth=64), None, dict(rgb=80, length=96),
                                           clamp=rtk.ClampConfig(radius=3))
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        for a in list(out.values()):
            assert (a == 7).all()


class _Spy:
    """stands in for the library: records which symbol a wrapper called, and answers RTK_OK"""
    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        def f(*args):
            self.called.append((name, len(args)))
            return 0
        return f


def test_clamp_none_reaches_the_plain_symbols(rtk, monkeypatch):
    spy = _Spy()
    monkeypatch.setattr(rtk, "_L", spy)
    mk3, mk1 = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    cur = dict(rgb=mk3, position=mk3, normal=mk3, depth=mk1)
    ptrs, outs = dict(rgb=16, position=32, normal=48, depth=64), dict(rgb=80, length=96)
    rtk.temporal_accumulate(cur, None)
    rtk.temporal_accumulate(cur, None, rtk.TemporalConfig(), None)
    rtk.temporal_accumulate_device(W, H, ptrs, None, outs)
    rtk.temporal_accumulate_device(W, H, ptrs, None, outs, clamp=None)
    assert spy.called == [("rtk_temporal_accumulate", 4)] * 2 + [("rtk_temporal_accumulate_device", 5)] * 2
    del spy.called[:]
    rtk.temporal_accumulate(cur, None, clamp=rtk.ClampConfig())
    rtk.temporal_accumulate_device(W, H, ptrs, None, outs, clamp=rtk.ClampConfig(radius=2))
    assert spy.called == [("rtk_temporal_accumulate_clamped", 5), ("rtk_temporal_accumulate_clamped_device", 6)]
