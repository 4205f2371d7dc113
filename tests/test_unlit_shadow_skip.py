"""Occlusion queries whose light contribution is exactly zero are counted but not traced (RTK_SKIP_UNLIT_SHADOW).

The light loop adds `((intensity / area) * cosine) * albedo` when is_occluded says "clear" and nothing otherwise.  When that
addend is +0 or -0 in every channel the answer cannot change the pixel: the sums it goes into start at +0, are only ever
results of float additions, hence never hold -0, and x + (+-0) has the bits of x for every other x.  The CPU test pins that
lemma in float32; the GPU tests demand the oracle's frame and ray count with the rule on and off, and less work with it on.
"""
import json

import numpy as np
import pytest

from conftest import SCENE5

FRAME_MODES = {"lane": 1, "group4": 3, "group8": 4, "stream": 6}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- the lemma (no GPU)

def test_adding_a_signed_zero_never_changes_a_sum_that_started_at_plus_zero():
    rng = np.random.default_rng(5)
    f32 = np.float32
    n = 200_000
    # terms of every kind: normal, subnormal, huge, exact cancellations, signed zeros, infinities, NaN
    mag = (10.0 ** rng.uniform(-45, 38, size=n)).astype(f32)
    terms = (mag * rng.choice([-1.0, 1.0], size=n).astype(f32)).astype(f32)
    terms[::7] = -terms[1::7][: terms[::7].size]                       # x then -x: sums that come back to zero
    terms[3::11] = f32(0.0)
    terms[5::13] = f32(-0.0)
    special = np.array([np.inf, -np.inf, np.nan, np.finfo(f32).max, -np.finfo(f32).max, np.finfo(f32).tiny, 1e-45, -1e-45], dtype=f32)
    terms[rng.integers(0, n, size=4000)] = special[rng.integers(0, special.size, size=4000)]
    chains = terms.reshape(-1, 20)                                     # 10,000 running sums of 20 terms, all from +0
    pz, nz = f32(0.0), f32(-0.0)
    with np.errstate(all="ignore"):
        acc = np.zeros(chains.shape[0], dtype=f32)
        seen_zero = seen_nan = seen_inf = 0
        for j in range(chains.shape[1]):
            acc = (acc + chains[:, j]).astype(f32)
            # a chain that starts at +0 never holds -0 ...
            assert not np.any((acc == 0) & np.signbit(acc)), j
            # ... so adding +0 or -0 leaves its bits alone, NaN and infinities included
            assert np.array_equal(_bits((acc + pz).astype(f32)), _bits(acc)), j
            assert np.array_equal(_bits((acc + nz).astype(f32)), _bits(acc)), j
            seen_zero += int(np.sum(acc == 0)); seen_nan += int(np.sum(np.isnan(acc))); seen_inf += int(np.sum(np.isinf(acc)))
    assert seen_zero > 100 and seen_nan > 100 and seen_inf > 100        # the cases the argument is about did occur
    # the one value the argument excludes really is different: -0 + +0 = +0
    assert np.signbit(nz) and not np.signbit(f32(nz + pz))
    # and the skip test itself: an addend is +-0 in all channels exactly when the channel of largest magnitude is
    contrib = np.concatenate([(10.0 ** rng.uniform(-45, 10, size=5000)), [0.0, -0.0, np.inf, np.nan]]).astype(f32)
    alb = (10.0 ** rng.uniform(-45, 3, size=(contrib.size, 3)) * rng.choice([-1.0, 0.0, 1.0], size=(contrib.size, 3))).astype(f32)
    alb[-1] = (0.0, 0.0, 0.0); alb[-2] = (0.0, 1.0, 0.0); alb[7] = (np.nan, 0.0, 0.0); alb[8] = (np.inf, 0.0, 0.0)
    with np.errstate(all="ignore"):
        per_channel = np.all((contrib[:, None] * alb).astype(f32) == 0, axis=1)
        reach = np.where(np.isnan(alb).any(axis=1), f32(np.nan), np.abs(alb).max(axis=1)).astype(f32)
        by_reach = (contrib * reach).astype(f32) == 0
    assert np.array_equal(per_channel, by_reach)
    assert 100 < per_channel.sum() < per_channel.size - 100


# ---------------------------------------------------------------- GPU: scene5, rule on and off

def _accel(rtk, monkeypatch, path, knob):
    """Environment knobs are read when an accel is built."""
    if knob is None:
        monkeypatch.delenv("RTK_SKIP_UNLIT_SHADOW", raising=False)
    else:
        monkeypatch.setenv("RTK_SKIP_UNLIT_SHADOW", knob)
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(path))


_ORACLE_FRAMES = {}


def _oracle_frame(ora, path, w, h, spp, depth, gi):
    key = (path, w, h, spp, depth, gi)
    if key not in _ORACLE_FRAMES:
        oacc = ora.Accel(ora.Scene(ora.load_crtscene(path)), ora.ACCEL_KD_SIMD)
        _ORACLE_FRAMES[key] = oacc.render(w, h, spp, depth, gi)
    return _ORACLE_FRAMES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(320, 180), (203, 117), (640, 360)])
@pytest.mark.parametrize("mode", list(FRAME_MODES))
def test_scene5_same_frame_and_rays_less_work(rtk, ora, monkeypatch, mode, w, h):
    ref, ocn = _oracle_frame(ora, SCENE5, w, h, 1, 5, 0)
    tris = {}
    for knob in ("0", None):                                           # off, then the default (on)
        acc = _accel(rtk, monkeypatch, SCENE5, knob)
        for rep in range(3):                                           # (repeats: the cost-feedback order, packed workgroups)
            rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, max_ray_depth=5, trace_mode=FRAME_MODES[mode]))
            assert cn["rays"] == ocn["rays"], (knob, rep)
            assert np.array_equal(_bits(rgb), _bits(ref)), (knob, rep, float(np.max(np.abs(rgb - ref))))
        rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, max_ray_depth=5, trace_mode=FRAME_MODES[mode], collect_stats=2))
        assert cn["rays"] == ocn["rays"], knob
        assert np.array_equal(_bits(rgb), _bits(ref)), knob
        tris[knob] = cn["tris"]
        rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, max_ray_depth=5, trace_mode=FRAME_MODES[mode], collect_stats=1))
        assert cn["tris"] == ocn["tris"] and cn["nodes"] == ocn["nodes"], knob      # the reference's work: the rule is off there
    print(f"{mode} {w}x{h}: tris visited with the rule off {tris['0']}, on {tris[None]}")
    assert tris[None] < tris["0"]                                      # the rule fired


# ---------------------------------------------------------------- GPU: the edges of the argument, on a hand-made scene

def _quad(p0, p1, p2, p3):
    return [c for p in (p0, p1, p2, p3) for c in p], [0, 1, 2, 0, 2, 3]


def _edge_scene(smooth):
    """A floor of five strips (plain, a zero channel, a negative channel, black, plain again), a back wall with a mirror in its
    middle, a tent and a slab above the floor that cast shadows, and six lights: one in the wall's plane, one in the floor's plane,
    one below the floor and behind the wall, one of intensity 0, one of negative intensity, and an ordinary one."""
    mats = [{"type": "diffuse", "albedo": a, "smooth_shading": smooth} for a in
            ([0.8, 0.7, 0.6], [0.0, 0.5, 1.0], [0.5, -0.25, 0.75], [0.0, 0.0, 0.0], [0.3, 0.9, 0.4])]
    mats.append({"type": "reflective", "albedo": [1.0, 1.0, 1.0], "smooth_shading": smooth})        # 5
    mats.append({"type": "diffuse", "albedo": [0.9, 0.2, -0.5], "smooth_shading": smooth})           # 6: the tent (its vertex normals differ from its face normals)
    objs = []
    for i in range(5):                                                 # floor strips along x, normal +y
        x0, x1 = -5.0 + 2.0 * i, -3.0 + 2.0 * i
        v, t = _quad((x0, 0.0, 2.0), (x1, 0.0, 2.0), (x1, 0.0, -6.0), (x0, 0.0, -6.0))
        objs.append({"material_index": i, "vertices": v, "triangles": t})
    for (x0, x1, m) in ((-5.0, -1.5, 0), (-1.5, 1.5, 5), (1.5, 5.0, 2)):                            # back wall, normal +z
        v, t = _quad((x0, 0.0, -6.0), (x1, 0.0, -6.0), (x1, 4.0, -6.0), (x0, 4.0, -6.0))
        objs.append({"material_index": m, "vertices": v, "triangles": t})
    apex = (0.5, 1.6, -3.0)                                            # tent: four faces sharing an apex (smooth normals differ per vertex)
    base = [(-0.7, 0.4, -1.8), (1.7, 0.4, -1.8), (1.7, 0.4, -4.2), (-0.7, 0.4, -4.2)]
    objs.append({"material_index": 6, "vertices": [c for p in base + [apex] for c in p],
                 "triangles": [0, 1, 4, 1, 2, 4, 2, 3, 4, 3, 0, 4, 0, 2, 1, 0, 3, 2]})
    v, t = _quad((-3.5, 1.0, -1.0), (-2.0, 1.0, -1.0), (-2.0, 1.0, -3.0), (-3.5, 1.0, -3.0))          # slab over the floor's left
    objs.append({"material_index": 4, "vertices": v, "triangles": t})
    lights = [{"intensity": 900, "position": [2.0, 2.0, -6.0]},        # exactly in the wall's plane
              {"intensity": 700, "position": [7.0, 0.0, -2.0]},        # exactly in the floor's plane
              {"intensity": 800, "position": [0.0, -3.0, -9.0]},       # below the floor and behind the wall
              {"intensity": 0, "position": [1.0, 5.0, 1.0]},           # lights nothing
              {"intensity": -300, "position": [-2.0, 6.0, 0.0]},       # negative addends
              {"intensity": 1200, "position": [3.0, 5.0, 1.0]}]
    return {"settings": {"background_color": [0.1, 0.2, 0.3], "image_settings": {"width": 160, "height": 120}},
            "camera": {"matrix": [1, 0, 0, 0, 1, 0, 0, 0, 1], "position": [0.0, 2.0, 3.0]},
            "lights": lights, "materials": mats, "objects": objs}


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "smooth"])
@pytest.mark.parametrize("gi", [0, 2], ids=["direct", "gi"])
def test_edge_cases_of_the_argument_in_both_engines(rtk, ora, monkeypatch, tmp_path, smooth, gi):
    path = str(tmp_path / "unlit_edges.crtscene")
    with open(path, "w") as f:
        json.dump(_edge_scene(smooth), f)
    w, h, spp, depth = 160, 120, (2 if gi else 1), 4
    ref, ocn = _oracle_frame(ora, path, w, h, spp, depth, gi)
    assert np.isfinite(ref).all() and ref.min() < 0.0 < ref.max()       # negative addends reach pixels; nothing degenerate
    tris = {}
    for knob in ("0", None):
        acc = _accel(rtk, monkeypatch, path, knob)
        for mode in ("group4", "group8", "stream", "lane") + ((0,) if gi else ()):       # + RTK_TRACE_AUTO's trials between the engines
            tm = FRAME_MODES.get(mode, 0)
            for rep in range(4 if mode == 0 else 2):
                rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, spp=spp, max_ray_depth=depth, diffuse_rays=gi, trace_mode=tm))
                assert cn["rays"] == ocn["rays"], (knob, mode, rep)
                assert np.array_equal(_bits(rgb), _bits(ref)), (knob, mode, rep, float(np.max(np.abs(rgb - ref))))
            if mode in ("group4", "stream"):
                rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, spp=spp, max_ray_depth=depth, diffuse_rays=gi, trace_mode=tm, collect_stats=2))
                assert cn["rays"] == ocn["rays"] and np.array_equal(_bits(rgb), _bits(ref)), (knob, mode)
                tris[(knob, mode)] = cn["tris"]
    for mode in ("group4", "stream"):                                  # half of this scene's queries are unlit: the rule fired in both engines
        assert tris[(None, mode)] < tris[("0", mode)], (mode, tris)
