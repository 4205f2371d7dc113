"""Soundness of the bundle culling (trace.hip.hpp) on the CPU model (tests/cull_model.py): a triangle the culling drops
is never accepted by the exact per-ray test for ANY ray of the bundle -- hammered with random and adversarial cases
(rays aimed exactly at vertices and edges, degenerate and tiny triangles, wide and narrow bundles, noisy apexes)."""
import numpy as np
import pytest

import cull_cases as cc
import cull_model as cm
from cull_cases import bundle as _bundle, triangles as _triangles

f32 = np.float32


@pytest.mark.parametrize("kind", ["camera", "shadow", "raw"])
def test_culled_triangles_are_never_hit(kind):
    rng = np.random.default_rng({"camera": 1, "shadow": 2, "raw": 3}[kind])
    culled_p = culled_i = not_hit = total = 0
    for it in range(300):
        C, o, d = _bundle(rng, kind)
        v0, e1, e2 = _triangles(rng, o, d, 512)
        ol, oh, dl, dh = cm.bundle_boxes(o, d)
        delta, ok = cm.pencil_delta(o, d, C)
        for cull in (True, False):
            hit = cm.tri_accepts(o, d, v0, e1, e2, cull).any(0)
            mi = cm.interval_misses(ol, oh, dl, dh, cull, v0, e1, e2)
            assert not (mi & hit).any(), (kind, it, cull, "interval")
            if ok:
                mp = cm.pencil_misses(C, delta, ol, oh, dl, dh, cull, v0, e1, e2)
                assert not (mp & hit).any(), (kind, it, cull, "pencil", np.nonzero(mp & hit)[0][:5])
                culled_p += int((mp & ~hit).sum())
            culled_i += int((mi & ~hit).sum()); not_hit += int((~hit).sum()); total += hit.size
    # the culling must also be worth something on these near-miss-heavy sets (a sanity floor, not a performance claim)
    assert culled_p > 0.3 * not_hit or kind == "raw"
    assert culled_i > 0


def test_wrong_apex_only_loosens_the_culling():
    """The apex is a hint: rays that do not pass near it give a large delta, never a wrong answer."""
    rng = np.random.default_rng(7)
    for it in range(100):
        C, o, d = _bundle(rng, "shadow")
        wrong = (C + rng.normal(size=3).astype(f32) * f32(5.0)).astype(f32)
        v0, e1, e2 = _triangles(rng, o, d, 512)
        ol, oh, dl, dh = cm.bundle_boxes(o, d)
        delta, ok = cm.pencil_delta(o, d, wrong)
        if not ok:
            continue
        for cull in (True, False):
            hit = cm.tri_accepts(o, d, v0, e1, e2, cull).any(0)
            mp = cm.pencil_misses(wrong, delta, ol, oh, dl, dh, cull, v0, e1, e2)
            assert not (mp & hit).any(), (it, cull)


@pytest.mark.parametrize("kind", cc.KINDS)
def test_culled_triangles_are_never_hit_over_scales_and_epsilons(kind):
    """The same property over the coordinate range the culling claims (just under kBundleLimit down to 1e-3) and the epsilons a
    scene may set; per cell the set must have both hits and culled triangles, or it would prove nothing."""
    cells = [(t, e, 1.0) for t, e in cc.GRID] + ([(None, 1e-6, 1e-3), (None, 1e-6, 1e3)] if kind == "raw" else [])
    for target, eps, dscale in cells:
        hits = culled = 0
        for it, s in enumerate(cc.grid_sets(kind)):
            C, o, d, v0, e1, e2 = cc.rescale(*s, target, dscale)
            ol, oh, dl, dh = cm.bundle_boxes(o, d)
            delta, ok = cm.pencil_delta(o, d, C)
            for cull in (True, False):
                hit = cm.tri_accepts(o, d, v0, e1, e2, cull, eps).any(0)
                mi = cm.interval_misses(ol, oh, dl, dh, cull, v0, e1, e2, eps)
                assert not (mi & hit).any(), (kind, target, eps, dscale, it, cull, "interval", np.nonzero(mi & hit)[0][:5])
                mp = np.zeros_like(mi)
                if ok:
                    mp = cm.pencil_misses(C, delta, ol, oh, dl, dh, cull, v0, e1, e2, eps)
                    assert not (mp & hit).any(), (kind, target, eps, dscale, it, cull, "pencil", np.nonzero(mp & hit)[0][:5])
                hits += int(hit.sum()); culled += int((mi | mp).sum())
        assert hits > 0 and culled > 0, (kind, target, eps, dscale, hits, culled)


def _zero_axis(rng, d, it):
    """Every third bundle gets a zero direction component: in all its rays, or in some of them."""
    d = d.copy()
    if it % 3 == 1:
        d[:, rng.integers(0, 3)] = 0.0
    elif it % 3 == 2:
        d[rng.random(64) < 0.3, rng.integers(0, 3)] = 0.0
    return d


@pytest.mark.parametrize("kind", cc.KINDS)
def test_culled_boxes_are_never_hit(kind):
    """bundle_may_hit_box against slab(): a box the bundle test drops is missed by every ray of the bundle.  Boxes around
    points on the rays, flat boxes, faces through an origin, rays with a zero direction component (that axis gives no bound)."""
    rng = np.random.default_rng({"camera": 21, "shadow": 22, "raw": 23}[kind])
    dropped = missed = hit_n = 0
    for it in range(150):
        C, o, d = _bundle(rng, kind)
        d = _zero_axis(rng, d, it)
        lo, hi = cc.boxes(rng, o, d, 256)
        img = cm.bundle_image(o, d, True)
        flags = cm.image_flags(img)
        for a, bit in enumerate((cm.BUNDLE_INVX, cm.BUNDLE_INVY, cm.BUNDLE_INVZ)):
            if (d[:, a] == 0).any():
                assert not flags & bit, (kind, it, a)
        hit = cm.slab_hits(o, d, lo, hi)[0].any(0)
        may = cm.box_may_hit(img, lo, hi)
        assert not (~may & hit).any(), (kind, it, np.nonzero(~may & hit)[0][:5])
        dropped += int((~may).sum()); missed += int((~hit).sum()); hit_n += int(hit.sum())
    assert hit_n > 0 and dropped > 0, (hit_n, missed, dropped)          # (not vacuous: boxes are hit, boxes are dropped)
