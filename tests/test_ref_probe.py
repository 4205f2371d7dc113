"""The CPU oracle and the Python models against the reference itself, bit for bit.

oracle/ref_probe.cpp is a program over the reference's own headers (recipe: oracle/ref.mk, built by __graft_entry__.build()
where a checkout of the reference is present).  Two layers:

  * against tests/golden/ref_probe/ (arrays the probe wrote, tools/make_ref_probe_fixtures.py): always runs, needs neither
    the reference nor oracle/_ref/;
  * against the live probe, where oracle/_ref/ holds the binaries: the fixtures are what the probe writes now, then the
    sweep that is too big to commit -- every loadable scene and the generated ones, every tree shape and eps of
    tests/test_gpu_tree_params.py, packet widths 4 / 8 / 16 and the scalar kd_tree_accel; closest hits, occlusion queries,
    radiance and frames at max_ray_depth 5 and 10.

Nothing has a tolerance.  Two allowances for NaNs, none for numbers: a NaN pixel only has to be a NaN on both sides
(ref_probe_cases.same_frame); and for kd_tree_accel (--scalar) alone, whose `dist < eps` lets a NaN distance through as a hit,
a NaN hit field only has to be a NaN in the same component (ref_probe_cases.hits_differences, nan_sign_free).  Every hit
field of every kd_tree_simd_accel variant and of the fixtures is compared on plain bits.
Not covered: io/json/loader.hpp (the probe is fed arrays), the JPEG decode (tests/golden/jpeg/), GI and multi-sample frames
(the reference's RNG is a data race: statistical gate in tests/test_reference_outputs.py)."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ref_probe_cases as rc
from radiance_views import ViewBatch, interior_views, jittered_views, kind_counts, with_constant_material
from test_all_scenes import IDS as LOADABLE_IDS
from test_gpu_tree_params import EPS, TREES
from test_random_scenes import _make_scene

POOL = min(16, os.cpu_count() or 1)
GENERATED = tuple(range(8)) + (100, 101, 102)
TREE_VARIANTS = {"default": "default", **{t: t for t in TREES}, **{"eps_" + e: "eps_" + e for e in EPS}}


@pytest.fixture(scope="module")
def fixtures():
    return {name: rc.load_fixture(name) for name in rc.FIXTURE_SCENES}


_flats, _oaccs = {}, {}
_cache_lock = threading.RLock()        # the live layer asks from worker threads


def _flat(ora, key):
    """key: a scene's path below tests/golden/scenes without its suffix, or ("generated", seed)"""
    with _cache_lock:
        if key not in _flats:
            _flats[key] = _make_scene(ora, key[1]) if isinstance(key, tuple) else ora.load_crtscene(rc.scene_path(key))
        return _flats[key]


def _oacc(ora, key, W=8, tree="default", scalar=False):
    k = (key, W, tree, scalar)
    with _cache_lock:
        if k not in _oaccs:
            md, ml, eps = ora.REF_TREES[tree]
            _oaccs[k] = ora.Accel(ora.Scene(_flat(ora, key)), ora.ACCEL_KD_SCALAR if scalar else ora.ACCEL_KD_SIMD, eps=eps,
                                  max_depth=md, max_leaf=ml, W=W)
        return _oaccs[k]


# ================================================================ layer 1: against the committed fixtures

def test_variants_cover_the_tree_parameter_tests(ora):
    """The recipe's variants are the TREES and EPS of tests/test_gpu_tree_params.py, value for value."""
    for name, (md, ml) in TREES.items():
        assert ora.REF_TREES[name] == (md, ml, 1e-6)
    for name, eps in EPS.items():
        assert ora.REF_TREES["eps_" + name][:2] == (8, 64) and np.float32(ora.REF_TREES["eps_" + name][2]) == np.float32(eps)
    assert set(ora.REF_TREES) == set(TREE_VARIANTS)
    mk = open(os.path.join(os.path.dirname(ora.__file__), "ref.mk")).read()
    for name, (md, ml, eps) in ora.REF_TREES.items():
        line = [l for l in mk.splitlines() if l.startswith(f"TREE_{name} ")][0].split(":=")[1].split()
        assert (int(line[0]), int(line[1]), float(line[2])) == (md, ml, eps), name


def test_manifest_matches_the_files():
    import hashlib
    man = rc.manifest()
    assert set(man["scenes"]) == set(rc.FIXTURE_SCENES) | {rc.EPS_FIXTURE} | set(rc.material_fixture_names())
    for name, e in man["scenes"].items():
        for fn, meta in e["files"].items():
            data = open(os.path.join(rc.FIXTURE_DIR, fn), "rb").read()
            assert len(data) == meta["bytes"] <= 188775 and hashlib.sha256(data).hexdigest() == meta["sha256"], fn


@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_fixture_tree(ora, fixtures, name):
    fx = fixtures[name]
    for i, W in enumerate(rc.WIDTHS):
        oa = _oacc(ora, rc.FIXTURE_SCENES[name], W)
        box, link, refs = oa.dump()
        assert rc.same_bits(box, fx["tree_box"]) and rc.same_bits(link, fx["tree_link"]) and rc.same_bits(refs, fx["tree_refs"]), W
        assert oa.num_packets == fx["tree_packets"][i], W


@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_fixture_intersect(ora, fixtures, name):
    fx = fixtures[name]
    ref = fx["hits"]
    assert (ref["hit"] == 1).sum() >= 200 and (ref["hit"] == 0).sum() >= 200        # both outcomes are populated
    for W in rc.WIDTHS:
        got = rc.oracle_hits(ora, _oacc(ora, rc.FIXTURE_SCENES[name], W), fx["rays"])
        assert not rc.hits_differences(ref, got, what=f"{name} W={W}")


def test_fixture_intersect_at_exactly_eps(ora):
    """Recorded from the reference built with eps = 0.25: a hit at a distance of exactly eps is a miss for the packet test
    (`eps < t`, kd_tree_simd.hpp:57), the same ray started an eighth of its direction earlier hits."""
    with np.load(os.path.join(rc.FIXTURE_DIR, rc.EPS_FIXTURE + ".npz"), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    flat = _flat(ora, ("generated", 100))
    assert rc.same_bits(np.ascontiguousarray(flat.vertices, np.float32), fx["scene_vertices"])      # _make_scene gives the recorded scene
    assert rc.same_bits(np.ascontiguousarray(flat.indices, np.uint32), fx["scene_indices"])
    ref, n = fx["eps_hits"], len(fx["eps_rays"]) // 2
    assert n >= 200
    for cull in (0, 1):
        floor = (ref[cull]["hit"] == 1) & (ref[cull]["mesh"] == 2)
        assert not floor[:n].any()                                  # exactly eps away: not the floor
    assert ((ref[0]["hit"] == 1) & (ref[0]["mesh"] == 2))[n:].sum() >= n // 2 and (rc.bits(ref[0]["t"][n:]) == rc.bits(np.float32(0.375))).any()
    for W in rc.WIDTHS:
        got = rc.oracle_hits(ora, _oacc(ora, ("generated", 100), W, "eps_0.25"), fx["eps_rays"])
        assert not rc.hits_differences(ref, got, what=f"W={W}")


@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_fixture_occluded(ora, fixtures, name):
    fx = fixtures[name]
    flat = _flat(ora, rc.FIXTURE_SCENES[name])
    want, calls = rc.model_occluded(_oacc(ora, rc.FIXTURE_SCENES[name]), flat, fx["occ_rays"], fx["occ_max_t"])
    assert set(np.unique(fx["occ_answer"])) == {0, 1}
    diff = np.flatnonzero(want != fx["occ_answer"])
    assert diff.size == 0, (name, diff[:8], fx["occ_rays"][diff[:1]], fx["occ_max_t"][diff[:1]])
    assert calls == fx["occ_calls"][0]


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_fixture_radiance(ora, fixtures, name, depth):
    fx = fixtures[name]
    vb = rc.radiance_views(ora, _flat(ora, rc.FIXTURE_SCENES[name]), name, 2, 32, 32)
    assert rc.same_bits(vb.rays, fx["rad_rays"])                  # the model's camera rays are the recorded input
    rgb, rays = vb.frames(max_depth=depth)
    assert rc.same_frame(rgb, fx[f"rad_rgb_d{depth}"]), rc.first_difference(fx[f"rad_rgb_d{depth}"], rgb)
    assert rays == fx[f"rad_calls_d{depth}"][0]


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FIXTURE_SCENES))
def test_fixture_frame(ora, fixtures, name, depth):
    fx = fixtures[name]
    for W in rc.WIDTHS:
        rgb, cn = _oacc(ora, rc.FIXTURE_SCENES[name], W).render(*rc.FRAME, 1, depth, 0)
        assert rc.same_frame(rgb, fx[f"frame_d{depth}"]), (W, rc.first_difference(fx[f"frame_d{depth}"], rgb))
        assert (cn["rays"], cn["hits"]) == tuple(fx[f"frame_calls_d{depth}"]), W


# ================================================================ layer 2: against the live probe

def _live(ora):
    if not (ora.ref_available(8, 5) and ora.ref_available(8, 10) and ora.ref_available(4, 5)):
        pytest.skip("oracle/_ref/ holds no probe: __graft_entry__.build() makes it where a checkout of the reference is present")


def _widths(ora):
    return [w for w in rc.WIDTHS if ora.ref_available(w, 5)]


def _map(fn, items):
    """fn(item) -> (what is wrong or None, counts) from a pool of threads -> ([(item, what is wrong)], the counts summed)"""
    items = list(items)
    with ThreadPoolExecutor(POOL) as ex:
        out = list(ex.map(fn, items))
    total = {}
    for _, counts in out:
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    return [(i, bad) for i, (bad, _) in zip(items, out) if bad], total


def test_live_fixtures_are_what_the_probe_writes_now(ora, fixtures):
    _live(ora)
    if _widths(ora) != list(rc.WIDTHS):
        pytest.skip("this host cannot run the 16-wide probe that the fixtures' packet counts come from")
    for name, rel in rc.FIXTURE_SCENES.items():
        arrays, _ = rc.record(ora, _flat(ora, rel), name)
        assert set(arrays) == set(fixtures[name])
        for k, v in arrays.items():
            assert rc.same_bits(v, fixtures[name][k]), (name, k)


ALL_SCENES = list(LOADABLE_IDS) + [("generated", s) for s in GENERATED]


def test_live_trees(ora):
    """Every scene x every tree variant x every width, and kd_tree_accel with leaf size 64: boxes, links, leaf references
    and packet counts."""
    _live(ora)
    assert len(LOADABLE_IDS) == 24

    def one(case):
        key, tree, W, scalar = case
        p = ora.RefProbe(_flat(ora, key), W, 5, tree, scalar)
        box, link, refs, packets = p.tree()
        md, ml, eps = ora.REF_TREES[tree]
        oa = ora.Accel(ora.Scene(_flat(ora, key)), ora.ACCEL_KD_SCALAR if scalar else ora.ACCEL_KD_SIMD, eps=eps, max_depth=md, max_leaf=ml, W=W)
        ob, ol, orf = oa.dump()
        if not (rc.same_bits(box, ob) and rc.same_bits(link, ol) and rc.same_bits(refs, orf)):
            return "tree differs", {}
        if not scalar and (p.width != W or packets != oa.num_packets):
            return f"packets {packets} vs {oa.num_packets}, width {p.width}", {}
        return None, {}

    for k in ALL_SCENES:
        _flat(ora, k)
    cases = [(k, t, W, False) for k in ALL_SCENES for t in TREE_VARIANTS for W in _widths(ora)] + [(k, "default", 4, True) for k in ALL_SCENES]
    bad, _ = _map(one, cases)
    print(len(cases), "trees compared")
    assert not bad, bad[:10]


INTERSECT_SCENES = ["hw09/scene5", "hw11/scene8", "hw15/scene2", "hw12/scene4", "hw11/scene4", ("generated", 100), ("generated", 101), ("generated", 102)]


def test_live_intersect(ora):
    """cull on and off, six ray families, every field of hit<F>; default tree at every width and scalar on every scene here,
    every tree and eps variant on scene5 and hw15/scene2."""
    _live(ora)
    n = 1500
    cases = [(k, "default", W, False) for k in INTERSECT_SCENES for W in _widths(ora)] + [(k, "default", 4, True) for k in INTERSECT_SCENES]
    cases += [(k, t, 8, False) for k in ("hw09/scene5", "hw15/scene2") for t in TREE_VARIANTS if t != "default"]
    rays = {}
    for k in INTERSECT_SCENES:
        sets = rc.ray_sets(_flat(ora, k), _oacc(ora, k), n, seed=11)
        rays[k] = np.ascontiguousarray(np.concatenate(list(sets.values())))

    def one(case):
        key, tree, W, scalar = case
        ref = ora.RefProbe(_flat(ora, key), W, 5, tree, scalar).intersect(rays[key])
        got = rc.oracle_hits(ora, _oacc(ora, key, W, tree, scalar), rays[key])
        counts = {"rays": ref.size, "hits": int((ref["hit"] == 1).sum()), "ties": int((ref["owners"] > 1).sum())}
        return rc.hits_differences(ref, got, what=str(case), nan_sign_free=scalar), counts      # (the allowance: --scalar alone)

    bad, stats = _map(one, cases)
    print(len(cases), "cases", stats)
    assert stats["hits"] > stats["rays"] // 4 and stats["ties"] > 0
    assert not bad, bad[:5]


def test_live_intersect_at_exactly_eps(ora):
    """A hit at a distance of exactly eps: `eps < t` in the packet test (kd_tree_simd.hpp:57) says miss.  eps = 0.25, the one
    eps of the variants for which such rays can be built from exactly representable numbers."""
    _live(ora)
    key = ("generated", 100)
    edge = rc.at_eps_rays(ora, _flat(ora, key), 0.25, 4000, seed=3)
    assert len(edge) >= 1000
    for W in _widths(ora):
        ref = ora.RefProbe(_flat(ora, key), W, 5, "eps_0.25").intersect(edge)
        assert not ((ref["hit"] == 1) & (ref["mesh"] == 2)).any()           # the floor, exactly eps away, is not hit
        bad = rc.hits_differences(ref, rc.oracle_hits(ora, _oacc(ora, key, W, "eps_0.25"), edge), what=f"W={W}")
        assert not bad, bad


OCCLUDED_SCENES = ["hw09/scene5", "hw11/scene8", "hw15/scene2", "hw11/scene4", ("generated", 1), ("generated", 3)]   # all but the first hold glass


def test_live_occluded(ora):
    """is_occluded: tests/occlusion_model.py over the oracle's closest hit against the reference's own loop."""
    _live(ora)
    cases = [(k, W) for k in OCCLUDED_SCENES for W in _widths(ora)]
    q = {k: rc.occlusion_queries(_flat(ora, k), _oacc(ora, k), 6000, seed=1) for k in OCCLUDED_SCENES}

    def one(case):
        key, W = case
        rays, max_t = q[key]
        p = ora.RefProbe(_flat(ora, key), W, 5)
        ref = p.occluded(rays, max_t)
        flat = _flat(ora, key)
        want, calls = rc.model_occluded(_oacc(ora, key, W), flat, rays, max_t)
        counts = {"queries": len(ref), "stepped": calls - int((np.float32(0) < max_t).sum())}
        diff = np.flatnonzero(ref != want)
        if diff.size:
            return f"{diff.size} answers differ, first query {diff[0]}: reference {ref[diff[0]]}", counts
        return (None if calls == p.calls else f"intersect calls {calls} vs reference {p.calls}"), counts

    bad, total = _map(one, cases)
    print(total)
    assert total["stepped"] > 1000                                 # queries that went on behind a transmissive surface
    assert not bad, bad


def _radiance_batches(ora):
    """The ray sets of tests/test_gpu_radiance.py at a smaller size: interior views, views near the camera of the textured
    scenes (procedural and bitmap), a constant material, and a generated scene whose first light lies exactly on the floor."""
    hw = lambda rel: _flat(ora, rel)
    yield "interior hw09/scene5", ViewBatch(ora, interior_views(hw("hw09/scene5"), 6), 40, 40)
    yield "interior hw11/scene8", ViewBatch(ora, interior_views(hw("hw11/scene8"), 6), 40, 40)
    yield "interior hw15/scene2", ViewBatch(ora, interior_views(hw("hw15/scene2"), 6), 40, 40)
    for rel in ("hw12/scene4", "hw12/scene1", "hw12/scene3", "hw11/scene4"):
        yield "near camera " + rel, ViewBatch(ora, jittered_views(hw(rel), 4), 40, 40)
    yield "constant", ViewBatch(ora, interior_views(with_constant_material(ora, hw("hw09/scene5"), 1), 6), 40, 40)
    yield "light on a surface", ViewBatch(ora, jittered_views(_make_scene(ora, 3), 4), 40, 40)


def test_live_radiance(ora):
    _live(ora)
    batches = list(_radiance_batches(ora))
    kinds = {}
    for _, vb in batches:
        for k, c in kind_counts(vb.level0()[1]).items():
            kinds[k] = kinds.get(k, 0) + c
    print("level-0 material kinds", kinds)
    assert all(kinds.get(k, 0) >= 500 for k in (-1, 0, 1, 2, 3, 4)), kinds        # miss and all five material variants
    cases = [(i, d, W) for i in range(len(batches)) for d in rc.DEPTHS for W in _widths(ora) if ora.ref_available(W, d)]

    def one(case):
        i, depth, W = case
        name, vb = batches[i]
        p = ora.RefProbe(vb.views[0], W, depth)
        ref = p.radiance(vb.rays)
        got, rays = vb.frames(max_depth=depth)
        if not rc.same_frame(ref, got):
            return f"{name}: {rc.first_difference(ref, got)}", {}
        return (None if rays == p.calls else f"{name}: intersect calls {rays} vs reference {p.calls}"), {}

    bad, _ = _map(one, cases)
    print(len(cases), "cases,", sum(vb.n for _, vb in batches), "rays each depth and width")
    assert not bad, bad


def test_live_frames(ora):
    """render_frame of every scene at 64 x 36, max_ray_depth 5 and 10: the oracle's frame, its intersect and hit counts; and
    on the reference itself the packet widths give one and the same image."""
    _live(ora)
    size = (64, 36)
    cases = [(k, d) for k in ALL_SCENES for d in rc.DEPTHS]

    def one(case):
        key, depth = case
        flat = _flat(ora, key)
        frames = {}
        for W in _widths(ora):
            if not ora.ref_available(W, depth):
                continue
            p = ora.RefProbe(flat, W, depth, size=size)
            frames[W] = (p.frame(), p.calls, p.hits)
        ref, calls, hits = frames[8]
        for W, (f, c, h) in frames.items():
            if not (rc.same_bits(f, ref) and (c, h) == (calls, hits)):
                return f"the reference's own frames differ between widths 8 and {W}", {}
        got, cn = _oacc(ora, key).render(*size, 1, depth, 0)
        counts = {"pixels": got.shape[0] * got.shape[1]}
        if not rc.same_frame(ref, got):
            return f"{rc.first_difference(ref, got)}", counts
        return (None if (cn["rays"], cn["hits"]) == (calls, hits) else f"calls/hits {cn['rays']}/{cn['hits']} vs reference {calls}/{hits}"), counts

    bad, total = _map(one, cases)
    print(len(cases), "frames,", total["pixels"], "pixels")
    assert not bad, bad
