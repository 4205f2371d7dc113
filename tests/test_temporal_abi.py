"""rtk_temporal_accumulate[_device] without a GPU: the symbols, the layout of the four structs, and the order of the argument
checks (a NULL p / cur / out; the parameters in the struct's order; the planes of the new frame and the outputs; those of the
history; the noise family, then the mesh family; the device variant's alignment; then the missing device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("rtk_temporal_accumulate", "rtk_temporal_accumulate_device")
PARAM_FIELDS = (("width", 0, 4), ("height", 4, 4), ("fov_degrees", 8, 8), ("alpha_min", 16, 4), ("plane_tolerance", 20, 4),
                ("normal_min_dot", 24, 4), ("max_history", 28, 4))
FRAME_FIELDS = ("rgb", "noise", "position", "normal", "depth", "mesh")
HISTORY_FIELDS = ("rgb", "noise", "length", "position", "normal", "depth", "mesh", "view")
OUTPUT_FIELDS = ("rgb", "noise", "length")
INF, NAN = float("inf"), float("nan")
W, H = 8, 6


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def test_library_exports_the_temporal_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    assert re.search(r"#define RTK_ABI_VERSION 4\b", _header())
    for name in ("temporal_accumulate", "temporal_accumulate_device", "TemporalConfig", "TemporalParams", "TemporalFrame",
                 "TemporalHistory", "TemporalOutputs"):
        assert hasattr(rtk, name)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rtk_\w+)\s*\(", text))) == sorted(rtk.ABI_SYMBOLS)


def test_temporal_structs_are_32_48_64_and_24_bytes_field_by_field(rtk):
    assert ctypes.sizeof(rtk.TemporalParams) == 32
    assert [n for n, _ in rtk.TemporalParams._fields_] == [n for n, _, _ in PARAM_FIELDS]
    for name, offset, size in PARAM_FIELDS:
        f = getattr(rtk.TemporalParams, name)
        assert (f.offset, f.size) == (offset, size), name
    body = re.search(r"typedef struct \{([^}]*)\} rtk_temporal_params;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", body) == [n for n, _, _ in PARAM_FIELDS]
    assert re.findall(r"(\w+)\s+\w+[\s\w,]*;", body) == ["int32_t", "double", "float", "float", "float", "int32_t"]
    for cls, fields, size, c_name in ((rtk.TemporalFrame, FRAME_FIELDS, 48, "rtk_temporal_frame"),
                                      (rtk.TemporalHistory, HISTORY_FIELDS, 64, "rtk_temporal_history"),
                                      (rtk.TemporalOutputs, OUTPUT_FIELDS, 24, "rtk_temporal_outputs")):
        assert ctypes.sizeof(cls) == size
        assert [n for n, _ in cls._fields_] == list(fields)
        for i, name in enumerate(fields):
            f = getattr(cls, name)
            assert (f.offset, f.size) == (8 * i, 8), (c_name, name)
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % c_name, _header(), flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\*(\w+)", body) == list(fields), c_name
    c = rtk.TemporalConfig(fov_degrees=40.0, alpha_min=0.25, plane_tolerance=0.5, normal_min_dot=-0.5, max_history=7).to_c(7, 9)
    assert (c.width, c.height, c.fov_degrees, c.alpha_min, c.plane_tolerance, c.normal_min_dot, c.max_history) == (7, 9, 40.0, 0.25, 0.5, -0.5, 7)


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

    def struct(cls, planes, kw):
        d = {n: planes[n].ctypes.data for n, _ in cls._fields_}
        d.update(kw)
        return cls(*(d[n] for n, _ in cls._fields_))

    frame = lambda **kw: struct(rtk.TemporalFrame, cur, kw)
    history = lambda **kw: struct(rtk.TemporalHistory, prev, kw)
    outputs = lambda **kw: struct(rtk.TemporalOutputs, out, kw)

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def host(p, c, q, o):
        return L.rtk_temporal_accumulate(ref(p), ref(c), ref(q), ref(o))

    def dev(p, c, q, o):                               # (never dereferenced: refused, or no device)
        return L.rtk_temporal_accumulate_device(ref(p), ref(c), ref(q), ref(o), None)

    return L, params, frame, history, outputs, (host, dev), (cur, prev, out)


# every refusal of the parameters, from the last of the struct to the first: (word of the message, what is wrong)
LATER = [
    ("max_history", dict(max_history=0)),
    ("normal_min_dot", dict(normal_min_dot=NAN)),
    ("plane_tolerance", dict(plane_tolerance=0.0)),
    ("alpha_min", dict(alpha_min=1.5)),
    ("fov_degrees", dict(fov_degrees=0.0)),
    ("height", dict(height=0)),
    ("width must", dict(width=0)),
]


def test_temporal_argument_errors_in_their_order(rtk):
    L, params, frame, history, outputs, calls, arrays = _setup(rtk)
    cur, prev, out = arrays
    INVALID = rtk.RTK_ERR_INVALID
    msg = lambda: L.rtk_last_error().decode()
    odd = lambda a: a.ctypes.data + 2
    for call in calls:
        # 1. a NULL p, cur or out, whatever else is wrong
        bad_p = params(max_history=0)
        assert call(None, frame(rgb=None), history(), outputs()) == INVALID and "null params" in msg()
        assert call(bad_p, None, history(), outputs()) == INVALID and "null params" in msg()
        assert call(bad_p, frame(rgb=None), None, None) == INVALID and "null params" in msg()
        # 2. the parameters: wrong in the ways k, k + 1, ... names way k; the planes come later
        kw = dict()
        for word, bad in LATER:
            kw.update(bad)
            assert call(params(**kw), frame(rgb=None), history(view=None), outputs(rgb=None)) == INVALID
            assert word in msg(), (word, msg())
        alone = [
            ("width must", [dict(width=0), dict(width=-1), dict(width=16385)]),
            ("height", [dict(height=0), dict(height=-1), dict(height=16385)]),
            ("fov_degrees", [dict(fov_degrees=v) for v in (0.0, -10.0, 180.0, INF, NAN)]),
            ("alpha_min", [dict(alpha_min=v) for v in (0.0, -0.0, -1.0, 1.5, INF, -INF, NAN)]),
            ("plane_tolerance", [dict(plane_tolerance=v) for v in (0.0, -0.0, -1.0, INF, -INF, NAN)]),
            ("normal_min_dot", [dict(normal_min_dot=v) for v in (-1.5, 1.5, INF, -INF, NAN)]),
            ("max_history", [dict(max_history=v) for v in (0, -1, (1 << 20) + 1)]),
        ]
        for word, bads in alone:
            for bad in bads:
                assert call(params(**bad), frame(), history(), outputs()) == INVALID, (word, bad)
                assert word in msg(), (word, msg())
        # 3. the planes of the new frame and of the outputs, before those of the history and before the families
        for name in ("rgb", "position", "normal", "depth"):
            assert call(params(), frame(**{name: None, "noise": None}), history(rgb=None), outputs()) == INVALID
            assert "of the new frame" in msg(), (name, msg())
        for name in ("rgb", "length"):
            assert call(params(), frame(noise=None), history(rgb=None), outputs(**{name: None})) == INVALID
            assert "of the outputs" in msg(), (name, msg())
            assert call(params(), frame(), None, outputs(**{name: None})) == INVALID and "of the outputs" in msg()
        # 4. with a prev: its planes and its view, before the families
        for name in ("rgb", "length", "position", "normal", "depth", "view"):
            assert call(params(), frame(noise=None, mesh=None), history(**{name: None}), outputs()) == INVALID
            assert "of the history" in msg(), (name, msg())
        # 5. the noise family, then the mesh family, both before the alignment
        for c, q, o in ((dict(noise=None), dict(), dict()), (dict(), dict(noise=None), dict()), (dict(), dict(), dict(noise=None)),
                        (dict(noise=None), dict(), dict(noise=None)), (dict(noise=None), dict(noise=None), dict())):
            assert call(params(), frame(mesh=None, rgb=odd(cur["rgb"]), **c), history(**q), outputs(**o)) == INVALID
            assert "noise planes" in msg(), (c, q, o, msg())
        assert call(params(), frame(noise=None), None, outputs()) == INVALID and "noise planes" in msg()
        assert call(params(), frame(), None, outputs(noise=None)) == INVALID and "noise planes" in msg()
        for c, q in ((dict(mesh=None), dict()), (dict(), dict(mesh=None))):
            assert call(params(), frame(rgb=odd(cur["rgb"]), **c), history(**q), outputs()) == INVALID
            assert "mesh planes" in msg(), (c, q, msg())
    host, dev = calls
    # 6. the device variant alone: the alignment of every plane of every struct
    for name in FRAME_FIELDS:
        assert dev(params(), frame(**{name: odd(cur[name])}), history(), outputs()) == INVALID and "4-byte" in msg(), name
        assert dev(params(), frame(**{name: odd(cur[name])}), None, outputs()) == INVALID and "4-byte" in msg(), name
    for name in HISTORY_FIELDS[:-1]:
        assert dev(params(), frame(), history(**{name: odd(prev[name])}), outputs()) == INVALID and "4-byte" in msg(), name
    for name in OUTPUT_FIELDS:
        assert dev(params(), frame(), history(), outputs(**{name: odd(out[name])})) == INVALID and "4-byte" in msg(), name
    for a in list(cur.values()) + list(prev.values()) + list(out.values()):
        assert (a == 7).all()


def test_after_validation_the_answer_is_no_device(rtk):
    L, params, frame, history, outputs, (host, dev), (cur, prev, out) = _setup(rtk)
    none = dict(noise=None, mesh=None)
    if rtk.device_count() > 0:          # a device is present: the valid host call goes through (the rest: tests/test_gpu_temporal.py)
        assert host(params(), frame(), None, outputs()) == rtk.RTK_OK
        assert np.array_equal(out["rgb"], cur["rgb"]) and np.array_equal(out["noise"], cur["noise"]) and (out["length"] == 1).all()
    else:
        for call in (host, dev):
            assert call(params(), frame(), history(), outputs()) == rtk.RTK_ERR_NO_DEVICE
            assert call(params(), frame(), None, outputs()) == rtk.RTK_ERR_NO_DEVICE
            assert call(params(), frame(**none), history(**none), outputs(noise=None)) == rtk.RTK_ERR_NO_DEVICE
            assert call(params(), frame(noise=None), history(noise=None), outputs(noise=None)) == rtk.RTK_ERR_NO_DEVICE
            assert call(params(width=16384, height=16384, alpha_min=1.0, normal_min_dot=-1.0, max_history=1 << 20), frame(), history(),
                        outputs()) == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:
            rtk.temporal_accumulate(dict(cur), dict(prev, view=(prev["view"][:3], prev["view"][3:])))
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        with pytest.raises(rtk.RtkError) as e:         # (never dereferenced: there is no device)
            rtk.temporal_accumulate_device(W, H, dict(rgb=16, position=32, normal=48, depth=64), None, dict(rgb=80, length=96))
        assert e.value.code == rtk.RTK_ERR_NO_DEVICE
        for a in list(out.values()):
            assert (a == 7).all()
