"""rtk_temporal_accumulate on the device against the numpy model of the contract (tests/temporal_model.py), bit for bit: the
synthetic pair of frames at every size with every combination of the optional families, without a history, in place, on a second
stream and twice, hostile but legal inputs, and one real chain render_frame_noise -> render_gbuffer -> temporal_accumulate under a
moving and under a static camera."""
import numpy as np
import pytest

import temporal_model as tm
from conftest import SCENE2

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = tm.SIZES + ((130, 70),)
_PAIRS = {}
_MODEL = {}


def _pair(w, h):
    if (w, h) not in _PAIRS:
        _PAIRS[(w, h)] = tm.synthetic_pair(w, h)
    return _PAIRS[(w, h)]


def _model(w, h, combo, with_prev=True):
    """the model's output for the synthetic pair, computed once and shared"""
    key = (w, h, combo, with_prev)
    if key not in _MODEL:
        cur, prev = _pair(w, h)
        out = tm.run(cur, prev if with_prev else None, combo, **tm.PARAMS)
        for a in out.values():
            if a is not None:
                a.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def _cfg(rtk, params):
    return rtk.TemporalConfig(**params)


def _select(frame, combo, history):
    """the planes of a frame that a case hands in"""
    names = ["rgb", "position", "normal", "depth"] + (["length"] if history else []) + [k for k in ("noise", "mesh") if k in combo]
    d = {k: frame[k] for k in names}
    if history:
        d["view"] = frame["view"]
    return d


def _host(rtk, cur, prev, combo, params=tm.PARAMS):
    return rtk.temporal_accumulate(_select(cur, combo, False), None if prev is None else _select(prev, combo, True), _cfg(rtk, params))


def _device(rtk, cur, prev, combo, params=tm.PARAMS, in_place=False, stream=None, twice=False):
    """the device variant on torch buffers with guard words behind every output -> dict rgb, noise, length"""
    import torch
    h, w = cur["depth"].shape
    n = w * h

    def up(a):
        if a.dtype == np.uint32:
            return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

    c = _select(cur, combo, False)
    q = None if prev is None else _select(prev, combo, True)
    dc = {k: up(a) for k, a in c.items()}
    dq = None if q is None else {k: up(a) for k, a in q.items() if k != "view"}
    noise = "noise" in combo
    sizes = dict(rgb=3 * n, length=n, **(dict(noise=n) if noise else {}))
    outs = {k: torch.full((m + GUARD,), 7.0, dtype=torch.float32, device="cuda") for k, m in sizes.items()}
    if in_place:                                        # out.rgb = cur.rgb, out.noise = cur.noise
        for k in ("rgb", "noise"):
            if k in outs:
                outs[k][:sizes[k]] = dc[k].reshape(-1)
                dc[k] = outs[k]
    cur_ptrs = {k: t.data_ptr() for k, t in dc.items()}
    prev_ptrs = None
    if dq is not None:
        prev_ptrs = {k: t.data_ptr() for k, t in dq.items()}
        prev_ptrs["view"] = q["view"]
    out_ptrs = {k: t.data_ptr() for k, t in outs.items()}
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        for _ in range(1 if in_place or not twice else 2):
            rtk.temporal_accumulate_device(w, h, cur_ptrs, prev_ptrs, out_ptrs, cfg=_cfg(rtk, params), stream=s.cuda_stream)
    s.synchronize()
    res = dict(noise=None)
    for k, t in outs.items():
        a = t.cpu().numpy()
        assert (a[sizes[k]:] == 7).all(), k                                    # nothing written behind an output
        res[k] = a[:sizes[k]].reshape((h, w, 3) if k == "rgb" else (h, w))
    for k, t in dc.items():                                                    # the inputs are inputs
        if not (in_place and k in ("rgb", "noise")):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(c[k]).view(np.uint32)), k
    for k, t in (dq or {}).items():
        assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(q[k]).view(np.uint32)), k
    return res


def _same(got, want):
    for k in ("rgb", "noise", "length"):
        if want[k] is None:
            if got[k] is not None:
                return False
        elif not np.array_equal(tm.bits(got[k]), tm.bits(want[k])):
            print(k, int((tm.bits(got[k]) != tm.bits(want[k])).sum()), "words differ")
            return False
    return True


@pytest.mark.parametrize("combo", tm.COMBOS)
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_pair_equals_the_model(rtk, w, h, combo):
    cur, prev = _pair(w, h)
    want = _model(w, h, combo)
    assert _same(_host(rtk, cur, prev, combo), want)
    assert _same(_device(rtk, cur, prev, combo), want)
    if (w, h) not in ((1, 1), (5, 3)):
        assert (want["length"] > 1).sum() * 2 > cur["hit"].sum()                # (the case shows something)


@pytest.mark.parametrize("w,h", SIZES)
def test_without_a_history_every_pixel_keeps_its_bits(rtk, w, h):
    cur, _ = _pair(w, h)
    for combo in ("noise+mesh", "neither"):
        want = _model(w, h, combo, with_prev=False)
        assert np.array_equal(tm.bits(want["rgb"]), tm.bits(cur["rgb"])) and (want["length"] == 1).all()
        assert _same(_host(rtk, cur, None, combo), want)
        assert _same(_device(rtk, cur, None, combo), want)


def test_in_place_a_second_stream_and_a_second_call_agree(rtk):
    import torch
    cur, prev = _pair(70, 36)
    for combo in tm.COMBOS:
        want = _model(70, 36, combo)
        assert _same(_device(rtk, cur, prev, combo, in_place=True), want), combo
        assert _same(_device(rtk, cur, prev, combo, stream=torch.cuda.Stream()), want), combo
        assert _same(_device(rtk, cur, prev, combo, twice=True), want), combo
        assert _same(_host(rtk, cur, prev, combo), want) and _same(_host(rtk, cur, prev, combo), want), combo
    assert _same(_device(rtk, cur, None, "noise+mesh", in_place=True), _model(70, 36, "noise+mesh", with_prev=False))


@pytest.mark.parametrize("case", [c[0] for c in tm.hostile_cases()])
def test_hostile_but_legal_inputs(rtk, case):
    """NaN, infinities and 1e30 among the positions, a zero-filled history, a previous view behind every surface, alpha_min = 1:
    the model decides, and no float is converted before its range is known"""
    name, cur, prev, params = next(c for c in tm.hostile_cases() if c[0] == case)
    want = tm.accumulate(cur, prev, detail=True, **params)
    assert _same(_host(rtk, cur, prev, "noise+mesh", params), want)
    assert _same(_device(rtk, cur, prev, "noise+mesh", params), want)
    if name in ("zero lengths", "view behind"):
        assert not want["blended"].any()
    if name == "alpha one":
        b = want["blended"]
        assert b.any() and np.array_equal(want["rgb"][b], cur["rgb"][b])


# ---- a real chain on hw15/scene2
W, H, FOV = 70, 36, 40.0
CHAIN = dict(fov_degrees=FOV, alpha_min=0.05, plane_tolerance=0.01, normal_min_dot=0.9, max_history=32)


def _render_cfg(rtk, spp, seed):
    return rtk.RenderConfig(width=W, height=H, spp=spp, seed=seed, trace_mode=rtk.TRACE_STREAM, diffuse_rays=2, max_ray_depth=2,
                            fov_degrees=FOV)


def _guides(rtk, acc):
    """The guides of the accel's camera, through the pixel centres: a g-buffer of spp = 1.  (With spp > 1 the rays of sample 0 are
    jittered inside their pixels, and so would the positions be that the reprojection starts from.)"""
    gb = acc.render_gbuffer(_render_cfg(rtk, 1, 0), sample=0, planes=("depth", "position", "normal", "mesh"))
    return {k: gb[k][0] for k in ("depth", "position", "normal", "mesh")}


def _frame(rtk, acc, seed, guides=None):
    """one 8-spp frame with its noise plane and the guides of the accel's camera"""
    rgb, noise, _ = acc.render_frame_noise(_render_cfg(rtk, 8, seed))
    return dict(guides or _guides(rtk, acc), rgb=rgb, noise=noise)


@pytest.fixture(scope="module")
def accel(rtk):
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE2))


def test_a_moved_camera_accumulates_onto_the_first_frame(rtk, accel):
    view_a = accel.camera()
    try:
        a = _frame(rtk, accel, 1)
        start = rtk.temporal_accumulate(a, None, _cfg(rtk, CHAIN))
        assert _same(start, tm.accumulate(a, None, **CHAIN))
        c, s = np.cos(np.deg2rad(2.0)), np.sin(np.deg2rad(2.0))
        ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        view_b = (view_a[0] + np.array((0.1, 0.05, -0.07), np.float32), (ry @ view_a[1].reshape(3, 3).astype(np.float64)).astype(np.float32).reshape(9))
        accel.set_camera(*view_b)
        b = _frame(rtk, accel, 2)
    finally:
        accel.set_camera(*view_a)
    prev = dict(a, rgb=start["rgb"], noise=start["noise"], length=start["length"], view=view_a)
    want = tm.accumulate(b, prev, **CHAIN)
    assert _same(rtk.temporal_accumulate(b, prev, _cfg(rtk, CHAIN)), want)
    assert _same(_device(rtk, b, prev, "noise+mesh", CHAIN), want)
    hit = b["depth"] >= 0
    share = float((want["length"][hit] > 1).mean())
    print(f"hit pixels {int(hit.sum())} of {W * H}, with history {share:.3f}")
    assert hit.sum() > W * H // 4 and share > 0.5


@pytest.fixture(scope="module")
def static_chain(rtk, accel):
    """Four 8-spp frames of one camera with four seeds, accumulated one onto the other, the model beside the library at every step;
    and one 256-spp frame of the same camera.  Rendered once for the tests below."""
    view = accel.camera()
    guides = _guides(rtk, accel)
    frames, hist, detail = [], None, None
    for seed in (11, 12, 13, 14):
        f = _frame(rtk, accel, seed, guides)
        prev = None if hist is None else dict(guides, rgb=hist["rgb"], noise=hist["noise"], length=hist["length"], view=view)
        detail = tm.accumulate(f, prev, detail=True, **CHAIN)
        hist = rtk.temporal_accumulate(f, prev, _cfg(rtk, CHAIN))
        assert _same(hist, detail), seed
        frames.append(f["rgb"])
    hit = guides["depth"] >= 0
    full = hit & (detail["accepted"] == 4)          # the hit pixels whose four taps lie inside the image and are accepted
    print(f"hit pixels {int(hit.sum())}, with four accepted taps {int(full.sum())}")
    assert full.sum() * 2 > hit.sum()
    ref, _ = accel.render_frame(_render_cfg(rtk, 256, 99))
    return dict(frames=frames, hist=hist, full=full, ref=ref)


def test_a_static_camera_averages_four_seeds(static_chain):
    frames, hist, full, ref = (static_chain[k] for k in ("frames", "hist", "full", "ref"))
    mean = np.stack(frames).astype(np.float64).mean(0)
    dev = float(np.abs(hist["rgb"].astype(np.float64) - mean)[full].max())
    print(f"largest deviation from the plain mean of the four frames {dev:.3g}")
    assert dev <= 1e-3
    rmse = lambda x: float(np.sqrt(np.mean((x[full].astype(np.float64) - ref[full].astype(np.float64)) ** 2)))
    r_acc, r_last = rmse(hist["rgb"]), rmse(frames[-1])
    print(f"rmse against 256 spp: accumulated {r_acc:.5f}, last frame {r_last:.5f}, ratio {r_acc / r_last:.3f} (expected near 0.5)")
    assert r_acc < r_last


def test_a_static_camera_counts_four_frames(static_chain):
    length = static_chain["hist"]["length"][static_chain["full"]]
    off = length != 4
    print(f"lengths other than 4: {int(off.sum())} of {length.size}, largest deviation {float(np.abs(length - 4).max()):.3g}")
    assert not off.any()
