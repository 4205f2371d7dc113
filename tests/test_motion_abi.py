"""rtk_render_motion[_device] without a GPU: the symbols, the layout of the two structs, and the order of the argument checks (a
NULL accel / p / tri / bary / prev_vertices / out; width, height; fov_degrees; both outputs NULL; motion without prev_view; the
device variant's alignment; then the missing device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENE5

SYMBOLS = ("rtk_render_motion", "rtk_render_motion_device")
PARAM_FIELDS = (("width", 0, 4), ("height", 4, 4), ("fov_degrees", 8, 8))
OUTPUT_FIELDS = ("prev_position", "motion")
INF, NAN = float("inf"), float("nan")
W, H = 8, 6


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_motion_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    assert re.search(r"#define RTK_ABI_VERSION 4\b", _header())
    for name in ("MotionConfig", "MotionParams", "MotionOutputs", "MOTION_MISS_BITS"):
        assert hasattr(rtk, name)
    assert hasattr(rtk.KdTreeSimdAccel, "render_motion") and hasattr(rtk.KdTreeSimdAccel, "render_motion_device")
    assert rtk.MOTION_MISS_BITS == 0x7FC00000
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rtk_\w+)\s*\(", text))) == sorted(rtk.ABI_SYMBOLS)


def test_motion_structs_are_16_bytes_each_field_by_field(rtk):
    assert ctypes.sizeof(rtk.MotionParams) == 16
    assert [n for n, _ in rtk.MotionParams._fields_] == [n for n, _, _ in PARAM_FIELDS]
    for name, offset, size in PARAM_FIELDS:
        f = getattr(rtk.MotionParams, name)
        assert (f.offset, f.size) == (offset, size), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_motion_params;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", body) == [n for n, _, _ in PARAM_FIELDS]
    assert re.findall(r"(\w+)\s+\w+[\s\w,]*;", body) == ["int32_t", "double"]
    assert ctypes.sizeof(rtk.MotionOutputs) == 16
    assert [n for n, _ in rtk.MotionOutputs._fields_] == list(OUTPUT_FIELDS)
    for i, name in enumerate(OUTPUT_FIELDS):
        f = getattr(rtk.MotionOutputs, name)
        assert (f.offset, f.size) == (8 * i, 8), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_motion_outputs;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*(\w+)", body) == list(OUTPUT_FIELDS)
    assert re.findall(r"(\w+)\s+\*", body) == ["float", "float"]
    c = rtk.MotionConfig(fov_degrees=40.0).to_c(7, 9)
    assert (c.width, c.height, c.fov_degrees) == (7, 9, 40.0)


def _setup(rtk):
    L = rtk.lib()
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    nv = acc.scene.info.n_vertices
    tri = np.full((H, W), 7, np.uint32)
    bary = np.full((H, W, 2), 7.0, np.float32)
    verts = np.full((nv, 3), 7.0, np.float32)
    view = np.full(12, 7.0, np.float32)
    out = dict(prev_position=np.full((H, W, 3), 7.0, np.float32), motion=np.full((H, W, 2), 7.0, np.float32))
    arrays = dict(tri=tri, bary=bary, verts=verts, view=view, **out)
    default = dict(accel=acc._h, tri=tri.ctypes.data, bary=bary.ctypes.data, verts=verts.ctypes.data, view=view.ctypes.data,
                   prev_position=out["prev_position"].ctypes.data, motion=out["motion"].ctypes.data, width=W, height=H, fov_degrees=90.0,
                   p=True, out=True)

    def call(device, **kw):
        a = dict(default, **kw)
        p = rtk.MotionConfig(fov_degrees=a["fov_degrees"]).to_c(a["width"], a["height"]) if a["p"] else None
        o = rtk.MotionOutputs(a["prev_position"], a["motion"]) if a["out"] else None
        ref = lambda x: ctypes.byref(x) if x is not None else None
        args = [a["accel"], ref(p), a["tri"], a["bary"], a["verts"], a["view"], ref(o)]
        if device:                                     # (never dereferenced: refused, or no device)
            return L.rtk_render_motion_device(*args, None)
        return L.rtk_render_motion(*args)

    return L, acc, call, arrays


def test_motion_argument_errors_in_their_order(rtk):
    L, acc, call, arrays = _setup(rtk)
    INVALID = rtk.RTK_ERR_INVALID
    msg = lambda: L.rtk_last_error().decode()
    odd = lambda name: arrays[name].ctypes.data + 2
    everything_later = dict(width=0, height=0, fov_degrees=NAN, prev_position=None, motion=None, view=None)
    for device in (False, True):
        # 1. a NULL accel, p, tri, bary, prev_vertices or out, whatever else is wrong
        for name in ("accel", "tri", "bary", "verts"):
            assert call(device, **dict(everything_later, **{name: None})) == INVALID and "null accel" in msg(), name
        assert call(device, **dict(everything_later, p=False)) == INVALID and "null accel" in msg()
        assert call(device, **dict(everything_later, out=False)) == INVALID and "null accel" in msg()
        # 2. wrong in the ways k, k + 1, ... names way k
        kw = dict(tri=odd("tri"))                      # (the alignment comes last of all)
        for word, bad in (("needs prev_view", dict(view=None)), ("both null", dict(prev_position=None, motion=None)),
                          ("fov_degrees", dict(fov_degrees=0.0)), ("height must", dict(height=0)), ("width must", dict(width=0))):
            kw.update(bad)
            assert call(device, **kw) == INVALID
            assert word in msg(), (word, msg())
        # 3. every refusal alone, with the ends of its range
        alone = [
            ("width must", [dict(width=v) for v in (0, -1, 16385)]),
            ("height must", [dict(height=v) for v in (0, -1, 16385)]),
            ("fov_degrees", [dict(fov_degrees=v) for v in (0.0, -10.0, 180.0, INF, -INF, NAN)]),
            ("both null", [dict(prev_position=None, motion=None), dict(prev_position=None, motion=None, view=None)]),
            ("needs prev_view", [dict(view=None), dict(view=None, prev_position=None)]),
        ]
        for word, bads in alone:
            for bad in bads:
                assert call(device, **bad) == INVALID, (word, bad)
                assert word in msg(), (word, msg())
    # 4. the device variant alone: the alignment of every pointer, behind everything else
    for name in ("tri", "bary", "verts", "prev_position", "motion"):
        assert call(True, **{name: odd(name)}) == INVALID and "4-byte" in msg(), name
    assert call(True, motion=odd("motion"), view=None) == INVALID and "needs prev_view" in msg()
    # a refused call changes nothing
    for a in arrays.values():
        assert (a == 7).all()


def test_after_validation_the_answer_is_no_device(rtk):
    L, acc, call, arrays = _setup(rtk)
    if rtk.device_count() > 0:          # a device is present: the valid host call goes through (the rest: tests/test_gpu_motion.py)
        assert call(False) == rtk.RTK_OK
        # id 7 is a triangle of scene5 and every vertex of the "previous pose" is (7, 7, 7): so is every point of it ((1 - 7 - 7) * 7
        # + 7 * 7 + 7 * 7), and it lies in the "camera" at (7, 7, 7), not in front of it
        assert (arrays["prev_position"] == 7).all()
        assert (arrays["motion"].view(np.uint32) == rtk.MOTION_MISS_BITS).all()
    else:
        for device in (False, True):
            assert call(device) == rtk.RTK_ERR_NO_DEVICE
            assert call(device, motion=None, view=None) == rtk.RTK_ERR_NO_DEVICE
            assert call(device, prev_position=None) == rtk.RTK_ERR_NO_DEVICE
            assert call(device, width=16384, height=16384, fov_degrees=179.0) == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            acc.render_motion(arrays["tri"], arrays["bary"], arrays["verts"], (arrays["view"][:3], arrays["view"][3:]))
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:         # (never dereferenced: there is no device)
            acc.render_motion_device(W, H, 16, 32, 48, dict(prev_position=64))
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        for a in arrays.values():
            assert (a == 7).all()
