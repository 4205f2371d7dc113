"""rtk_temporal_accumulate_clamped without a GPU: the numpy model of the contract (tests/temporal_clamp_model.py) against the
plain model where the clamp never fires, what keeps the shared fixture lit_pair honest, and the model against the scalar C++ of
csrc/temporal_clamp_math.hpp (tests/cpp/temporal_clamp_math_check.cpp, built with the library's float flags, plain and with the
host sanitizers, as a stand-alone program), bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_clamp_model as cm
import temporal_model as tm
from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "temporal_clamp_math_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "temporal_math.hpp"), os.path.join(PKG, "csrc", "temporal_clamp_math.hpp")]
FIXTURE_SIZES = ((37, 19), (70, 36), (130, 70))
CHECK_SIZES = FIXTURE_SIZES + ((1, 1), (5, 3))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NEVER = dict(radius=1, gamma=1e30, history_keep=0.0)        # a clamp that never fires

_pairs = {}
_wants = {}


def _pair(w, h):
    if (w, h) not in _pairs:
        _pairs[(w, h)] = cm.lit_pair(w, h)
    return _pairs[(w, h)]


def _assert_same(got, want):
    for k in ("rgb", "noise", "length"):
        if want[k] is None:
            assert got[k] is None
        else:
            assert np.array_equal(tm.bits(got[k]), tm.bits(want[k])), (k, int((tm.bits(got[k]) != tm.bits(want[k])).sum()))


@pytest.mark.parametrize("w,h", FIXTURE_SIZES)
def test_a_clamp_that_never_fires_is_the_plain_model_in_every_bit(w, h):
    """gamma = 1e30 at sizes where every box has a spread (a box of one pixel has lo = hi at any gamma: the hostile cases)"""
    for cur, prev in (tm.synthetic_pair(w, h), _pair(w, h)):
        for combo in tm.COMBOS:
            got = cm.accumulate(cur, prev, noise="noise" in combo, mesh="mesh" in combo, detail=True, **NEVER, **tm.PARAMS)
            assert int(got["clamped"].sum()) == 0
            _assert_same(got, tm.run(cur, prev, combo, **tm.PARAMS))


def test_without_a_history_the_bits_pass_through():
    cur, _ = _pair(37, 19)
    for combo in tm.COMBOS:
        got = cm.run(cur, None, combo, **tm.PARAMS)
        assert np.array_equal(tm.bits(got["rgb"]), tm.bits(cur["rgb"])) and (got["length"] == 1).all()
        assert (got["noise"] is None) == ("noise" not in combo)
        if got["noise"] is not None:
            assert np.array_equal(tm.bits(got["noise"]), tm.bits(cur["noise"]))
        _assert_same(got, tm.run(cur, None, combo, **tm.PARAMS))


@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("w,h", FIXTURE_SIZES)
def test_the_fixture_is_honest(w, h, radius):
    cur, prev = _pair(w, h)
    d = cm.accumulate(cur, prev, radius=radius, gamma=2.0, history_keep=1.0, detail=True, **tm.PARAMS)
    b = d["blended"]
    counts = dict(clamped=d["clamped"].sum(), unclamped=(b & ~d["clamped"]).sum(), below=d["below"].sum(), above=d["above"].sum(),
                  cut_mesh=d["cut_mesh"].sum(), cut_edge=d["cut_edge"].sum())
    print(f"{w}x{h} r={radius}: with history {int(b.sum())}, " + ", ".join(f"{k} {int(v)}" for k, v in counts.items()))
    for k, v in counts.items():
        assert v >= 20, k
    assert not d["clamped"][~b].any()
    # the box never counts more taps than it has, and always its centre
    assert (d["box"][b] >= 1).all() and (d["box"][b] <= (2 * radius + 1) ** 2).all()
    # mesh 0 of the history was left alone: most of its pixels stay unclamped at two standard deviations
    floor = b & (cur["mesh"] == 0) & (d["accepted"] == 4)
    assert (~d["clamped"][floor]).mean() > 0.5


def test_history_keep_shortens_clamped_pixels_only():
    cur, prev = _pair(70, 36)
    full = cm.accumulate(cur, prev, radius=1, gamma=2.0, history_keep=1.0, detail=True, **tm.PARAMS)
    half = cm.accumulate(cur, prev, radius=1, gamma=2.0, history_keep=0.5, detail=True, **tm.PARAMS)
    none = cm.accumulate(cur, prev, radius=1, gamma=2.0, history_keep=0.0, detail=True, **tm.PARAMS)
    plain = tm.run(cur, prev, "noise+mesh", **tm.PARAMS)
    c = full["clamped"]
    assert np.array_equal(c, half["clamped"]) and np.array_equal(c, none["clamped"])
    assert np.array_equal(tm.bits(full["length"]), tm.bits(plain["length"]))            # history_keep = 1: the plain call's length
    assert (none["length"][c] == 1).all()                                               # 0: a clamped pixel starts over
    assert (half["length"][c] < full["length"][c]).all() and (half["length"][c] > 1).all()
    for other in (half, none):
        for k in ("rgb", "noise", "length"):
            assert np.array_equal(tm.bits(other[k])[~c], tm.bits(full[k])[~c]), k
    # a clamped pixel's variance is at least the neighbourhood mean's share of the blend
    assert (full["noise"][c] >= plain["noise"][c]).all() and (full["noise"][c] > plain["noise"][c]).any()


# ---- the scalar C++
def _build_check(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        # the float flags of the library's Makefile: no contraction, no fast-math
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), SRC, "-o", exe])
    return exe


def dump(path, cur, prev, combo, params, clamp):
    """the file tests/cpp/temporal_clamp_math_check.cpp reads"""
    h, w = cur["depth"].shape
    noise, mesh = "noise" in combo, "mesh" in combo
    aspect, th, wf, hf = tm.scalars(w, h, params["fov_degrees"])
    view = prev["view"] if prev is not None else (np.zeros(3, np.float32), np.zeros(9, np.float32))
    consts = np.concatenate([np.asarray(view[0], np.float32).reshape(3), np.asarray(view[1], np.float32).reshape(9),
                             np.array([th, aspect, wf, hf, np.float32(params["max_history"]), params["alpha_min"],
                                       params["plane_tolerance"], params["normal_min_dot"]], np.float32),
                             np.array([clamp["gamma"], clamp["history_keep"]], np.float32)])
    with open(path, "wb") as f:
        np.array([w, h, prev is not None, noise, mesh, clamp["radius"], 0, 0], np.int32).tofile(f)
        consts.astype(np.float32).tofile(f)
        for frame in (cur, prev):
            if frame is None:
                continue
            for k in ("rgb", "position", "normal", "depth"):
                np.ascontiguousarray(frame[k], np.float32).tofile(f)
            if frame is prev:
                np.ascontiguousarray(frame["length"], np.float32).tofile(f)
            if noise:
                np.ascontiguousarray(frame["noise"], np.float32).tofile(f)
            if mesh:
                np.ascontiguousarray(frame["mesh"], np.uint32).tofile(f)


def _run_check(exe, tmp_path, cur, prev, combo, params, clamp):
    """-> (planes, clamped pixels) of the scalar program"""
    h, w = cur["depth"].shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    dump(src, cur, prev, combo, params, clamp)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    got = np.fromfile(dst, np.float32)
    n = w * h
    out = dict(rgb=got[:3 * n].reshape(h, w, 3), noise=None, length=got[-n:].reshape(h, w))
    if "noise" in combo:
        out["noise"] = got[3 * n:4 * n].reshape(h, w)
    assert got.size == (5 if "noise" in combo else 4) * n
    return out, int(re.search(r"clamped (\d+)", res.stdout).group(1))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("w,h", CHECK_SIZES)
def test_model_and_scalar_cpp_agree_in_every_bit(tmp_path, w, h, build):
    exe = _build_check("temporal_clamp_math_check" + ("_san" if build == "sanitized" else ""), SAN if build == "sanitized" else [])
    cur, prev = _pair(w, h)
    small = (w, h) in ((1, 1), (5, 3))
    for radius in ((3,) if small else (1, 2, 3)):
        for combo in tm.COMBOS:
            for keep in (0.0, 0.5, 1.0):
                clamp = dict(radius=radius, gamma=2.0, history_keep=keep)
                key = (w, h, radius, combo, keep)
                if key not in _wants:                                          # (once for both builds)
                    _wants[key] = cm.accumulate(cur, prev, noise="noise" in combo, mesh="mesh" in combo, detail=True, **clamp, **tm.PARAMS)
                want = _wants[key]
                got, n_clamped = _run_check(exe, tmp_path, cur, prev, combo, tm.PARAMS, clamp)
                _assert_same(got, want)
                assert n_clamped == int(want["clamped"].sum())
    clamp = dict(radius=3, gamma=2.0, history_keep=0.5)
    got, n_clamped = _run_check(exe, tmp_path, cur, None, "noise+mesh", tm.PARAMS, clamp)
    _assert_same(got, cm.run(cur, None, "noise+mesh", clamp, **tm.PARAMS))
    assert n_clamped == 0


def test_hostile_inputs_on_the_model_and_the_scalar_cpp(tmp_path):
    """NaN, infinities and 1e30 in a tenth of the new frame's colours, gamma = 0, and a box of one pixel: the comparisons decide as
    written; a NaN meets a NaN (its payload is the hardware's), every other word its bits"""
    exe = _build_check("temporal_clamp_math_check_san", SAN)
    for name, cur, prev, params, clamp in cm.hostile_cases():
        want = cm.accumulate(cur, prev, detail=True, **clamp, **params)
        got, n_clamped = _run_check(exe, tmp_path, cur, prev, "noise+mesh", params, clamp)
        assert n_clamped == int(want["clamped"].sum()), name
        for k in ("rgb", "noise", "length"):
            nan = np.isnan(want[k])
            assert np.array_equal(np.isnan(got[k]), nan), (name, k)
            assert np.array_equal(tm.bits(got[k])[~nan], tm.bits(want[k])[~nan]), (name, k)
        b, c = want["blended"], want["clamped"]
        assert b.sum() >= 20, name
        if name == "colours":
            assert np.isnan(want["rgb"]).any() and np.isinf(want["rgb"]).any() and 0 < c.sum() < b.sum()
        if name == "gamma zero":
            # lo = hi = m: every pixel with history is pulled to its neighbourhood mean
            assert np.array_equal(c, b)
        if name == "box of one":
            # lo = hi = c: the history is replaced by the new colour, and with history_keep = 0 the pixel starts over
            assert (want["box"][b] == 1).all() and np.array_equal(c, b) and (want["length"][b] == 1).all()
            assert np.allclose(want["rgb"][b], cur["rgb"][b], rtol=1e-6, atol=0)
