"""The GPU against the reference itself, without the oracle in between: rtk_accel_tree_dump, rtk_accel_intersect,
rtk_accel_occluded, rtk_accel_radiance and a 96 x 54 rtk_render_frame must reproduce, bit for bit, the arrays that a build of
the reference's own code wrote (tests/golden/ref_probe/, recorded by tools/make_ref_probe_fixtures.py).  Reads nothing else.

NaN: a pixel or a normal component that is NaN in the recording has to be NaN here, whatever its sign and payload (x86 and the
GPU differ there, see tests/test_random_scenes._same_frame)."""
import numpy as np
import pytest

import ref_probe_cases as rc

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
_cache = {}


def _case(rtk, name):
    if name not in _cache:
        _cache[name] = (rtk.KdTreeSimdAccel(rtk.parse_scene_file(rc.scene_path(rc.FIXTURE_SCENES[name]))), rc.load_fixture(name))
    return _cache[name]


@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_tree_dump(rtk, name):
    acc, fx = _case(rtk, name)
    box, link, refs = acc.tree_dump()
    assert rc.same_bits(box, fx["tree_box"]) and rc.same_bits(link, fx["tree_link"]) and rc.same_bits(refs, fx["tree_refs"])


@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_intersect(rtk, name, cull):
    acc, fx = _case(rtk, name)
    ref = fx["hits"][int(cull)]
    hit = ref["hit"] == 1
    assert hit.sum() >= 100 and (~hit).sum() >= 100
    for mode in (rtk.TRACE_AUTO, rtk.TRACE_LANE, rtk.TRACE_WAVE):
        got = acc.intersect(fx["rays"], cull, mode)
        bad = np.flatnonzero((got["tri"] != MISS) != hit)
        assert bad.size == 0, (mode, "hit or miss", bad[:8], ref["t"][bad[:8]], got["t"][bad[:8]])
        assert np.array_equal(got["mesh"][hit], ref["mesh"][hit]), mode
        one = hit & (ref["owners"] == 1)                            # a duplicated triangle: either copy is the reference's hit
        assert np.array_equal(got["tri"][one], ref["tri"][one]), (mode, np.flatnonzero(one & (got["tri"] != ref["tri"]))[:8])
        for f in ("t", "u", "v"):
            bad = np.flatnonzero(hit & (rc.bits(got[f]) != rc.bits(ref[f])))
            assert bad.size == 0, (mode, f, bad[:8], got[f][bad[:8]], ref[f][bad[:8]])
        assert rc.same_frame(got["normal"][hit], ref["hit_normal"][hit]), (mode, rc.first_difference(ref["hit_normal"][hit], got["normal"][hit]))


def test_intersect_at_exactly_eps(rtk, ora):
    """eps = 0.25 on a generated scene: a hit exactly eps away is a miss (`eps < t`), as recorded from the reference."""
    import os
    from test_random_scenes import _make_scene, _rtk_scene
    with np.load(os.path.join(rc.FIXTURE_DIR, rc.EPS_FIXTURE + ".npz"), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    flat = _make_scene(ora, 100)
    assert rc.same_bits(np.ascontiguousarray(flat.vertices, np.float32), fx["scene_vertices"])
    assert rc.same_bits(np.ascontiguousarray(flat.indices, np.uint32), fx["scene_indices"])
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, flat), eps=0.25)
    for cull in (False, True):
        ref = fx["eps_hits"][int(cull)]
        hit = ref["hit"] == 1
        for mode in (rtk.TRACE_AUTO, rtk.TRACE_LANE, rtk.TRACE_WAVE):
            got = acc.intersect(fx["eps_rays"], cull, mode)
            bad = np.flatnonzero((got["tri"] != MISS) != hit)
            assert bad.size == 0, (cull, mode, bad[:8], got["t"][bad[:8]])
            assert np.array_equal(got["mesh"][hit], ref["mesh"][hit]), (cull, mode)
            for f in ("t", "u", "v"):
                assert np.array_equal(rc.bits(got[f][hit]), rc.bits(ref[f][hit])), (cull, mode, f)


@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_occluded(rtk, name):
    acc, fx = _case(rtk, name)
    want = fx["occ_answer"]
    assert (want == 1).sum() >= 100 and (want == 0).sum() >= 100
    for mode in (rtk.TRACE_AUTO, rtk.TRACE_LANE, rtk.TRACE_WAVE):
        got, n_int = acc.occluded(fx["occ_rays"], fx["occ_max_t"], shadow_bias=rc.BIAS, trace_mode=mode, count=True)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (mode, bad[:8], got[bad[:8]], want[bad[:8]])
        assert n_int == fx["occ_calls"][0], mode


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_radiance(rtk, name, depth):
    acc, fx = _case(rtk, name)
    got, cn = acc.radiance(fx["rad_rays"], None, rtk.RadianceConfig(max_ray_depth=depth, cull=True))
    ref = fx[f"rad_rgb_d{depth}"]
    assert rc.same_frame(got, ref), rc.first_difference(ref, got)
    assert cn["rays"] == fx[f"rad_calls_d{depth}"][0] and cn["primary"] == len(ref)


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_frame(rtk, name, depth):
    acc, fx = _case(rtk, name)
    ref, (calls, _) = fx[f"frame_d{depth}"], fx[f"frame_calls_d{depth}"]
    w, h = rc.FRAME
    for mode in (rtk.TRACE_AUTO, rtk.TRACE_GROUP4, rtk.TRACE_STREAM):
        for rep in range(2):                                        # the second frame runs in cost-feedback order
            rgb, cn = acc.render_frame(rtk.RenderConfig(width=w, height=h, spp=1, max_ray_depth=depth, trace_mode=mode))
            assert rc.same_frame(rgb, ref), (mode, rep, rc.first_difference(ref, rgb))
            assert cn["rays"] == calls, (mode, rep)                 # the reference's own count of intersect calls
