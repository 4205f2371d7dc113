"""The GPU on the generated material scenes (tests/material_scenes.py): indices of refraction below 1, 0 and negative, exactly
normal incidence, glass inside glass, smooth refractive meshes, every texture kind with its edge cases, odd lights, and
max_ray_depth 16, which fills k_render's 16-entry frame stack.  Frames, radiance and occlusion answers are compared with what the
reference itself wrote for these inputs (tests/golden/ref_probe/material_*, tools/make_ref_probe_fixtures.py); multi-sample and
GI frames, non-default biases and first hits from inside the glass (cull = 0), which the reference's probe does not cover, with the
CPU oracle.

Everything is compared on bits (ref_probe_cases.same_frame: a NaN only has to be a NaN; no recorded array holds one), and every
ray counter exactly.  The frame is 48 x 32; tests/test_material_scenes.py shows on the CPU that the cases are not empty."""
import numpy as np
import pytest

import material_scenes as ms
import ref_probe_cases as rc
from test_gpu_radiance import _redone

pytestmark = pytest.mark.gpu

NAMES = rc.material_fixture_names()              # fixture name -> variant
W, H = ms.SIZE
_cache = {}


def _fixture(variant):
    if ("fx", variant) not in _cache:
        _cache["fx", variant] = rc.load_fixture(rc.MATERIAL_PREFIX + variant)
    return _cache["fx", variant]


def _flat(ora, variant):
    if ("flat", variant) not in _cache:
        _cache["flat", variant] = ms.make_scene(ora, variant)
    return _cache["flat", variant]


def _accel(rtk, ora, variant):
    if ("acc", variant) not in _cache:
        _cache["acc", variant] = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, _flat(ora, variant)))
    return _cache["acc", variant]


def _oacc(ora, variant):
    if ("oacc", variant) not in _cache:
        _cache["oacc", variant] = ora.Accel(ora.Scene(_flat(ora, variant)), ora.ACCEL_KD_SIMD)
    return _cache["oacc", variant]


def _frame_modes(rtk):
    return {"auto": rtk.TRACE_AUTO, "lane": rtk.TRACE_LANE, "wave": rtk.TRACE_WAVE, "group4": rtk.TRACE_GROUP4,
            "group8": rtk.TRACE_GROUP8, "group16": rtk.TRACE_GROUP16, "stream": rtk.TRACE_STREAM}


# ---------------------------------------------------------------- the scene reaches the library as generated

@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_scene_and_tree_are_the_recorded_ones(rtk, ora, variant):
    fx, acc = _fixture(variant), _accel(rtk, ora, variant)
    got = acc.scene.arrays()
    for k in ms.SCENE_ARRAYS:
        assert rc.same_bits(np.ascontiguousarray(got[k]).reshape(fx["scene_" + k].shape), fx["scene_" + k]), k
    box, link, refs = acc.tree_dump()
    assert rc.same_bits(box, fx["tree_box"]) and rc.same_bits(link, fx["tree_link"]) and rc.same_bits(refs, fx["tree_refs"])


# ---------------------------------------------------------------- frames against the recording

@pytest.mark.parametrize("depth", ms.DEPTHS)
@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_frames(rtk, ora, variant, depth):
    fx, acc = _fixture(variant), _accel(rtk, ora, variant)
    ref, (calls, _) = fx[f"frame_d{depth}"], fx[f"frame_calls_d{depth}"]
    for name, mode in _frame_modes(rtk).items():
        for rep in range(2):                                        # the second frame runs in cost-feedback order
            rgb, cn = acc.render_frame(rtk.RenderConfig(width=W, height=H, spp=1, max_ray_depth=depth, trace_mode=mode))
            print(variant, depth, name, rep, "rays", cn["rays"], "recorded", calls, "first difference", rc.first_difference(ref, rgb))
            assert rc.same_frame(rgb, ref), (name, rep, rc.first_difference(ref, rgb))
            assert cn["rays"] == calls, (name, rep)


# ---------------------------------------------------------------- radiance of the special rays and the view batch

def _radiance_device(rtk, acc, rays, cfg):
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda")
    d_rgb = torch.full((n * 3,), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    acc.radiance_device(d_rays.data_ptr(), 0, n, d_rgb.data_ptr(), cfg, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy().reshape(n, 3)


@pytest.mark.parametrize("depth", ms.RAD_DEPTHS)
@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_radiance(rtk, ora, variant, depth):
    fx, acc = _fixture(variant), _accel(rtk, ora, variant)
    rays, ref = fx["rad_rays"], fx[f"rad_rgb_d{depth}"]
    cfg = rtk.RadianceConfig(max_ray_depth=depth, cull=True)
    got, cn = acc.radiance(rays, None, cfg)
    print(variant, depth, "rays", cn["rays"], "recorded", fx[f"rad_calls_d{depth}"][0], "first difference", rc.first_difference(ref, got))
    assert rc.same_frame(got, ref), rc.first_difference(ref, got)
    assert cn["rays"] == fx[f"rad_calls_d{depth}"][0] and cn["primary"] == len(ref)
    dev = _radiance_device(rtk, acc, rays, cfg)
    assert rc.same_frame(dev, ref), ("device", rc.first_difference(ref, dev))


@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_radiance_through_the_fallback_kernel(rtk, ora, variant, monkeypatch, capfd):
    """With room for the batch's own rays only (tests/test_gpu_radiance.py::test_queue_overflow_is_redone_on_the_device) the
    children overflow the queues, and every chunk is shaded again by k_radiance_fallback, depth 16 included."""
    monkeypatch.setenv("RTK_STREAM_NODE_FACTOR", "1")              # environment knobs are read when an accel is built
    monkeypatch.setenv("RTK_STREAM_DEBUG", "1")
    fx = _fixture(variant)
    acc = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, _flat(ora, variant)))
    capfd.readouterr()
    for depth in ms.RAD_DEPTHS:
        rays, ref, calls = _unculled(ora, variant, depth)
        for what, rays, ref, calls, cull in (("recorded", fx["rad_rays"], fx[f"rad_rgb_d{depth}"], int(fx[f"rad_calls_d{depth}"][0]), True),
                                             ("unculled", rays, ref, calls, False)):
            # the queues hold the batch's rays + 4096 nodes: copies of the batch up to 16384 rays, so that the 4096 are little beside
            # its children
            k = -(-16384 // len(rays))
            rays, ref = np.tile(rays, (k, 1)), np.tile(ref, (k, 1))
            got, cn = acc.radiance(rays, None, rtk.RadianceConfig(max_ray_depth=depth, cull=cull))
            report = _redone(capfd)
            print(variant, depth, what, report, "first difference", rc.first_difference(ref, got))
            assert report[-1][0] == len(ref) and report[-1][2] >= 1 and report[-1][2] == report[-1][1], (what, depth, report)
            assert rc.same_frame(got, ref), (what, depth, rc.first_difference(ref, got))
            assert cn["rays"] == k * calls and cn["primary"] == len(ref), (what, depth)


def _unculled(ora, variant, depth):
    """material_scenes.unculled_radiance_rays and what the oracle sees along them without culling -> (rays, rgb, intersect calls)"""
    key = ("unculled", variant, depth)
    if key not in _cache:
        rays, _ = ms.unculled_radiance_rays(ora, _flat(ora, variant), _oacc(ora, variant))
        rgb, cn = _oacc(ora, variant).radiance(rays, depth, cull=False)
        _cache[key] = (rays, rgb, cn["rays"])
    return _cache[key]


@pytest.mark.parametrize("depth", ms.RAD_DEPTHS)
@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_radiance_from_inside_the_glass(rtk, ora, variant, depth):
    """cull = 0: first hits that meet the glass from inside, which the reference's culled probe cannot record: exactly normal
    incidence on the way out, origins inside the inner mesh, and the critical angle of the exit +- 1e-6 .. 1e-2 rad for every ior
    above 1.  Against the oracle's color_hit (ora_radiance with cull = 0)."""
    acc = _accel(rtk, ora, variant)
    rays, ref, calls = _unculled(ora, variant, depth)
    assert len(rays) >= 64 and not np.isnan(ref).any()
    cfg = rtk.RadianceConfig(max_ray_depth=depth, cull=False)
    got, cn = acc.radiance(rays, None, cfg)
    print(variant, depth, "rays", cn["rays"], "oracle", calls, "first difference", rc.first_difference(ref, got))
    assert rc.same_frame(got, ref), rc.first_difference(ref, got)
    assert cn["rays"] == calls and cn["primary"] == len(ref)
    dev = _radiance_device(rtk, acc, rays, cfg)
    assert rc.same_frame(dev, ref), ("device", rc.first_difference(ref, dev))
    culled, _ = acc.radiance(rays, None, rtk.RadianceConfig(max_ray_depth=depth, cull=True))
    assert not rc.same_frame(culled, ref)                            # the flag reaches the first hit


# ---------------------------------------------------------------- occlusion through stacked glass

@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_occluded(rtk, ora, variant):
    fx, acc = _fixture(variant), _accel(rtk, ora, variant)
    want = fx["occ_answer"]
    assert (want == 1).sum() >= 20 and (want == 0).sum() >= 20
    for mode in (rtk.TRACE_AUTO, rtk.TRACE_LANE, rtk.TRACE_WAVE):
        got, n_int = acc.occluded(fx["occ_rays"], fx["occ_max_t"], shadow_bias=rc.BIAS, trace_mode=mode, count=True)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (mode, bad[:8], got[bad[:8]], want[bad[:8]])
        assert n_int == fx["occ_calls"][0], mode


# ---------------------------------------------------------------- one accel walked through the variants

def test_live_materials_and_lights(rtk, ora):
    acc = rtk.KdTreeSimdAccel(ms.rtk_scene(rtk, _flat(ora, ms.VARIANTS[0])))
    for variant in ms.VARIANTS + (ms.VARIANTS[0],):
        acc.set_materials(**ms.material_rows(variant))
        acc.set_lights(*ms.light_rows(variant))
        fx = _fixture(variant)
        ref, (calls, _) = fx["frame_d10"], fx["frame_calls_d10"]
        for mode in (rtk.TRACE_GROUP4, rtk.TRACE_STREAM):
            rgb, cn = acc.render_frame(rtk.RenderConfig(width=W, height=H, spp=1, max_ray_depth=10, trace_mode=mode))
            assert rc.same_frame(rgb, ref), (variant, mode, rc.first_difference(ref, rgb))
            assert cn["rays"] == calls, (variant, mode)


# ---------------------------------------------------------------- textures through the other doors

def test_gbuffer_albedo_and_material(rtk, ora):
    """The albedo and material planes of the texture variant against the oracle's first hit: its own sample(texture, hit, uvs) on
    a texture material, the material's albedo elsewhere, the background on a miss (ora_first_hit_albedo)."""
    flat, oa = _flat(ora, "textured"), _oacc(ora, "textured")
    rays = oa.camera_rays(W, H).reshape(-1, 6)
    hits = oa.intersect(rays, True)
    hit = hits["mesh"] != ms.MISS
    mat = flat.mesh_material[np.where(hit, hits["mesh"], 0)]
    textured = hit & (flat.mat_kind[mat] == ms.TEXTURE)
    want = oa.first_hit_albedo(rays, True)
    assert textured.sum() >= 500 and (~hit).sum() >= 32
    assert {int(k) for k in flat.tex_kind[flat.mat_texture[mat[textured]]]} == {ms.ALBEDO, ms.EDGES, ms.CHECKER, ms.BITMAP}
    got = _accel(rtk, ora, "textured").render_gbuffer(rtk.RenderConfig(width=W, height=H), planes=("albedo", "material"))
    assert np.array_equal(got["material"][0].reshape(-1), np.where(hit, mat.astype(np.uint32), np.uint32(ms.MISS)).astype(np.uint32))
    alb = got["albedo"][0].reshape(-1, 3)
    bad = np.flatnonzero((rc.bits(alb) != rc.bits(want)).any(axis=1))
    assert bad.size == 0, (bad[:8], mat[bad[:8]], alb[bad[:8]], want[bad[:8]])


def _partition():
    """48 x 32 cut into twelve rectangles, no edge but the frame's own a multiple of 8"""
    xs, ys = (0, 5, 18, 31, W), (0, 7, 20, H)
    return [(xs[i], ys[j], xs[i + 1], ys[j + 1]) for j in range(3) for i in range(4)]


@pytest.mark.parametrize("mode", ["auto", "group4", "stream"])
def test_regions_of_the_texture_variant(rtk, ora, mode):
    from regions_checks import SENTINEL, check_in_frame, check_packed
    fx, acc = _fixture("textured"), _accel(rtk, ora, "textured")
    ref, (calls, _) = fx["frame_d10"], fx["frame_calls_d10"]
    rects = _partition()
    assert sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in rects) == W * H
    cfg = rtk.RenderConfig(width=W, height=H, spp=1, max_ray_depth=10, trace_mode=_frame_modes(rtk)[mode])
    views, cn = acc.render_regions(cfg, rects, rtk.REGIONS_PACKED)
    check_packed(views, rects, ref, f"packed {mode}")
    assert cn["rays"] == calls
    frame, cn = acc.render_regions(cfg, rects, rtk.REGIONS_IN_FRAME, np.full((H, W, 3), SENTINEL, np.float32))
    check_in_frame(frame, rects, ref, f"in frame {mode}")
    assert cn["rays"] == calls
    total = 0                                                       # and rectangle by rectangle the counters add up
    for r in rects[::5]:
        _, c1 = acc.render_regions(cfg, [r], rtk.REGIONS_PACKED)
        total += c1["rays"]
    rest = [r for i, r in enumerate(rects) if i % 5]
    total += acc.render_regions(cfg, rest, rtk.REGIONS_PACKED)[1]["rays"]
    assert total == calls


# ---------------------------------------------------------------- what the reference does not probe: against the oracle

def _against_oracle(rtk, ora, variant, what, **kw):
    acc, oa = _accel(rtk, ora, variant), _oacc(ora, variant)
    ref, ocn = oa.render(W, H, kw["spp"], kw["max_ray_depth"], kw.get("diffuse_rays", 0),
                         shadow_bias=kw.get("shadow_bias", 1e-4), reflection_bias=kw.get("reflection_bias", 1e-4),
                         refraction_bias=kw.get("refraction_bias", 1e-4))
    assert ocn["rays"] <= 4_000_000, ocn["rays"]
    for mode in (rtk.TRACE_GROUP4, rtk.TRACE_STREAM, rtk.TRACE_AUTO):
        rgb, cn = acc.render_frame(rtk.RenderConfig(width=W, height=H, trace_mode=mode, **kw))
        print(variant, what, mode, "rays", cn["rays"], "oracle", ocn["rays"], "first difference", rc.first_difference(ref, rgb))
        assert rc.same_frame(rgb, ref), (what, mode, rc.first_difference(ref, rgb))
        assert cn["rays"] == ocn["rays"], (what, mode)


@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_gi_samples(rtk, ora, variant):
    _against_oracle(rtk, ora, variant, "spp 3, 2 diffuse rays, depth 3", spp=3, max_ray_depth=3, diffuse_rays=2)


@pytest.mark.parametrize("variant", ms.VARIANTS)
def test_two_samples_at_depth_16(rtk, ora, variant):
    _against_oracle(rtk, ora, variant, "spp 2, depth 16", spp=2, max_ray_depth=16)


def test_biases(rtk, ora):
    _against_oracle(rtk, ora, "ior15_075", "biases 1e-2, 0, 1e-3", spp=1, max_ray_depth=10, shadow_bias=1e-2, reflection_bias=0.0,
                    refraction_bias=1e-3)
    # a negative refraction bias starts the refracted ray in front of the surface it left: it meets that surface again
    _against_oracle(rtk, ora, "ior075_15", "refraction bias -1e-3", spp=1, max_ray_depth=10, refraction_bias=-1e-3)
