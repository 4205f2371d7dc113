"""rtk_denoise_workspace_bytes / rtk_denoise_frame[_device] without a GPU: the symbols, the layout of the two structs, and the order
of the argument checks (a NULL p / in / bytes; the parameters; n_images == 0 is RTK_OK; the planes; the device variant's
alignments and workspace; then the missing device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("rtk_denoise_workspace_bytes", "rtk_denoise_frame", "rtk_denoise_frame_device")
PARAM_FIELDS = ("width", "height", "iterations", "normal_power_log2", "sigma_luminance", "sigma_plane", "albedo_floor", "reserved")
INPUT_FIELDS = ("rgb", "noise", "albedo", "normal", "position", "depth")
INF, NAN = float("inf"), float("nan")
W, H = 8, 6


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_denoise_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    assert re.search(r"#define RTK_ABI_VERSION 4\b", _header())
    for name in ("denoise", "denoise_device", "denoise_workspace_bytes", "DenoiseConfig", "DenoiseParams", "DenoiseInputs"):
        assert hasattr(rtk, name)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rtk_\w+)\s*\(", text))) == sorted(rtk.ABI_SYMBOLS)


def test_denoise_structs_are_32_and_48_bytes_field_by_field(rtk):
    assert ctypes.sizeof(rtk.DenoiseParams) == 32
    assert [n for n, _ in rtk.DenoiseParams._fields_] == list(PARAM_FIELDS)
    for i, name in enumerate(PARAM_FIELDS):
        f = getattr(rtk.DenoiseParams, name)
        assert (f.offset, f.size) == (4 * i, 4), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_denoise_params;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", body) == list(PARAM_FIELDS)
    assert re.findall(r"(\w+)\s+\w+[\s\w,]*;", body) == ["int32_t", "int32_t", "int32_t", "float", "float", "float", "int32_t"]
    assert ctypes.sizeof(rtk.DenoiseInputs) == 48
    assert [n for n, _ in rtk.DenoiseInputs._fields_] == list(INPUT_FIELDS)
    for i, name in enumerate(INPUT_FIELDS):
        f = getattr(rtk.DenoiseInputs, name)
        assert (f.offset, f.size) == (8 * i, 8), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_denoise_inputs;", _header()).group(1)
    assert re.findall(r"\*(\w+)", body) == list(INPUT_FIELDS) and body.strip().startswith("const float")
    c = rtk.DenoiseConfig(iterations=3, normal_power_log2=1, sigma_luminance=2.0, sigma_plane=0.5, albedo_floor=0.25).to_c(7, 9)
    assert (c.width, c.height, c.iterations, c.normal_power_log2, c.sigma_luminance, c.sigma_plane, c.albedo_floor, c.reserved) == \
        (7, 9, 3, 1, 2.0, 0.5, 0.25, 0)


def _setup(rtk):
    L = rtk.lib()
    planes = {n: np.full((H, W, 3), 7.0, np.float32) for n in ("rgb", "albedo", "normal", "position")}
    planes.update({n: np.full((H, W), 7.0, np.float32) for n in ("noise", "depth")})
    out = np.full((H, W, 3), 7.0, np.float32)
    ws = np.zeros(W * H * 64 + 64, np.uint8)
    ws_ptr = (ws.ctypes.data + 15) & ~15

    def params(**kw):
        size = (kw.pop("width", W), kw.pop("height", H))
        return rtk.DenoiseConfig(**kw).to_c(*size)

    def inputs(**kw):
        d = {n: planes[n].ctypes.data for n in INPUT_FIELDS}
        d.update(kw)
        return rtk.DenoiseInputs(*(d[n] for n in INPUT_FIELDS))

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def host(p, n, i, o=out.ctypes.data, **_):
        return L.rtk_denoise_frame(ref(p), n, ref(i), o)

    def dev(p, n, i, o=out.ctypes.data, ws=ws_ptr, ws_bytes=W * H * 64):      # (never dereferenced: refused, or no device)
        return L.rtk_denoise_frame_device(ref(p), n, ref(i), o, ws, ws_bytes, None)

    def size(p, n, i=None, o=None, **_):
        return L.rtk_denoise_workspace_bytes(ref(p), n, ctypes.byref(ctypes.c_size_t(12345)))

    return L, params, inputs, (host, dev, size), planes, out


# every refusal of the parameters, from the last of rtk.h's list to the first: (word of the message, params, n_images)
LATER = [
    ("in total", dict(width=1 << 14, height=1 << 14), 9),
    ("n_images", dict(), -1),
    ("albedo_floor", dict(albedo_floor=0.0), None),
    ("sigma_plane", dict(sigma_plane=NAN), None),
    ("sigma_luminance", dict(sigma_luminance=-1.0), None),
    ("normal_power_log2", dict(normal_power_log2=9), None),
    ("iterations", dict(iterations=0), None),
    ("per image", dict(width=1 << 14, height=(1 << 14) + 1), None),
    ("width and height", dict(width=0), None),
]


def test_denoise_argument_errors_in_their_order(rtk):
    L, params, inputs, calls, planes, out = _setup(rtk)
    INVALID = rtk.RTK_ERR_INVALID
    msg = lambda: L.rtk_last_error().decode()
    for call in calls:
        # 1. a NULL p or in (or bytes), whatever else is wrong
        assert call(None, -1, inputs()) == INVALID
        if call is not calls[2]:
            assert call(params(iterations=0), -1, None) == INVALID and "null" in msg()
        # 2. the parameters: wrong in the ways k, k + 1, ... names way k
        kw, n = dict(), 1
        for word, bad, bad_n in LATER:
            kw.update(bad)
            n = bad_n if bad_n is not None else n
            assert call(params(**kw), n, inputs(rgb=None), None) == INVALID
            assert word in msg(), (word, msg())
        # each alone, in all its forms
        alone = [
            ("width and height", [dict(width=0), dict(height=0), dict(width=-1)]),
            ("per image", [dict(width=1 << 28, height=2), dict(width=0x7FFFFFFF, height=0x7FFFFFFF)]),
            ("iterations", [dict(iterations=0), dict(iterations=9), dict(iterations=-1)]),
            ("normal_power_log2", [dict(normal_power_log2=-1), dict(normal_power_log2=9)]),
            ("sigma_luminance", [dict(sigma_luminance=v) for v in (0.0, -0.0, -1.0, INF, -INF, NAN)]),
            ("sigma_plane", [dict(sigma_plane=v) for v in (0.0, -0.0, -1.0, INF, -INF, NAN)]),
            ("albedo_floor", [dict(albedo_floor=v) for v in (0.0, -0.0, -1.0, INF, -INF, NAN)]),
        ]
        for word, bads in alone:
            for bad in bads:
                assert call(params(**bad), 1, inputs()) == INVALID, (word, bad)
                assert word in msg(), (word, msg())
        assert call(params(), -1, inputs()) == INVALID and "n_images" in msg()
        assert call(params(width=1 << 14, height=1 << 14), 9, inputs()) == INVALID and "in total" in msg()
    host, dev, size = calls
    # 3. n_images == 0 is RTK_OK before the planes are looked at, device or not
    for call in (host, dev):
        assert call(params(), 0, inputs(rgb=None, normal=None, position=None, depth=None), None) == rtk.RTK_OK
    assert dev(params(), 0, inputs(), ws=None, ws_bytes=0) == rtk.RTK_OK
    b = ctypes.c_size_t(12345)
    assert L.rtk_denoise_workspace_bytes(ctypes.byref(params()), 0, ctypes.byref(b)) == rtk.RTK_OK and b.value == 0
    assert L.rtk_denoise_workspace_bytes(ctypes.byref(params()), 1, None) == INVALID
    # 4. a NULL rgb, normal, position, depth or output; noise and albedo may be NULL
    for call in (host, dev):
        for name in ("rgb", "normal", "position", "depth"):
            odd = {k: planes[k].ctypes.data + 2 for k in INPUT_FIELDS if k != name}        # (5. comes later)
            assert call(params(), 1, inputs(**{name: None, **odd}), ws=None) == INVALID and "null rgb" in msg(), name
        assert call(params(), 1, inputs(), None) == INVALID and "null rgb" in msg()
    # 5. the device variant alone: alignment of the planes, then the workspace
    for name in INPUT_FIELDS:
        assert dev(params(), 1, inputs(**{name: planes[name].ctypes.data + 2}), ws=None) == INVALID and "4-byte" in msg(), name
    assert dev(params(), 1, inputs(), out.ctypes.data + 1, ws=None) == INVALID and "4-byte" in msg()
    assert dev(params(), 1, inputs(), ws=None) == INVALID and "null workspace" in msg()
    good_ws = (np.zeros(1, np.uint8).ctypes.data + 15) & ~15
    assert dev(params(), 1, inputs(), ws=good_ws + 4, ws_bytes=0) == INVALID and "16-byte" in msg()
    assert dev(params(), 1, inputs(), ws_bytes=W * H * 64 - 1) == INVALID and "smaller" in msg()
    assert dev(params(iterations=1), 1, inputs(), ws_bytes=W * H * 48 - 1) == INVALID and "smaller" in msg()
    for a in list(planes.values()) + [out]:
        assert (a == 7).all()


def test_workspace_bytes_is_at_most_64_per_pixel(rtk):
    for (w, h, n) in ((1, 1, 1), (37, 19, 1), (70, 36, 2), (1920, 1080, 1), (1 << 14, 1 << 14, 8)):
        for it in (1, 2, 5, 8):
            b = rtk.denoise_workspace_bytes(w, h, n, rtk.DenoiseConfig(iterations=it))
            assert b == (48 if it == 1 else 64) * w * h * n and b % 16 == 0


def test_after_validation_the_answer_is_no_device(rtk):
    L, params, inputs, (host, dev, size), planes, out = _setup(rtk)
    if rtk.device_count() > 0:          # a device is present: the valid host call goes through (the rest: tests/test_gpu_denoise.py)
        planes["depth"][:] = -1.0       # all misses: every pixel keeps its bits
        assert host(params(), 1, inputs()) == rtk.RTK_OK
        assert np.array_equal(out, planes["rgb"])
    else:
        assert host(params(), 1, inputs()) == rtk.RTK_ERR_NO_DEVICE
        assert dev(params(), 1, inputs()) == rtk.RTK_ERR_NO_DEVICE
        assert dev(params(), 1, inputs(noise=None, albedo=None)) == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            rtk.denoise(planes["rgb"], planes["normal"], planes["position"], planes["depth"])
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            rtk.denoise_device(W, H, 16, 32, 48, 64, 80, 96, W * H * 64)          # (never dereferenced: there is no device)
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        assert (out == 7).all()
