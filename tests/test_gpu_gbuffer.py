"""rtk_render_gbuffer[_device] on the GPU.  The comparison side is the CPU oracle: ora.Accel.camera_rays + ora.Accel.intersect(cull=True)
of the scene with the view's camera (views_checks.with_camera), and beside it the product's own camera_rays + intersect.  Every
plane is compared by its bits (hit normals: a NaN must meet a NaN, as everywhere in this suite).  The albedo plane is pinned to the
oracle's frames: in a pixel lit by the scene's one light a texture material leaves k * sample(texture, hit, uvs), and the same
scene with white diffuse materials leaves k (render.hpp:205, 235)."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import SCENE5, SCENE8, SCENES
from scene_state_checks import DIFFUSE, TEXTURE, set_materials, with_material
from texture_checks import BITMAP, CHECKER, EDGES, Tex, set_textures, textures_of, with_textures
from update_checks import _rtk_scene
from views_checks import cameras, with_camera

pytestmark = pytest.mark.gpu

SCENE4_TEX = SCENES + "/hw12/scene4.crtscene"
MISS = 0xFFFFFFFF
SENTINEL = 0xA5C3F00D
GUARD = 64                                     # dwords in front of and behind every plane
PLANES = ("depth", "position", "normal", "albedo", "bary", "tri", "mesh", "material")
COMPS = dict(depth=1, position=3, normal=3, albedo=3, bary=2, tri=1, mesh=1, material=1)

_FLATS = {}
_OACCS = {}


def _flat(ora, path):
    if path not in _FLATS:
        _FLATS[path] = ora.load_crtscene(path)
    return _FLATS[path]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_normals(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_u32(np.nan_to_num(a).astype(np.float32)), _u32(np.nan_to_num(b).astype(np.float32)))


# ---------------------------------------------------------------- the expected planes

def _expected(ora, flat, cam, w, h, spp=1, sample=0, oracle_kw=None, materials=None):
    """The planes of one view from the oracle: its camera rays of `sample`, its closest hits with culling.  `albedo` is what the
    contract says for materials that are no textures (the material's albedo, the background on a miss) and None where a texture
    material is hit (pinned elsewhere, to the oracle's frames)."""
    key = (id(flat), None if cam is None else cam.tobytes(), tuple(sorted((oracle_kw or {}).items())))
    if key not in _OACCS:                      # (the flat scene is kept with its accel, so its id stays its own)
        f = flat if cam is None else with_camera(flat, cam)
        _OACCS[key] = (flat, f, ora.Accel(ora.Scene(f), ora.ACCEL_KD_SIMD, **(oracle_kw or {})))
    _, f, oacc = _OACCS[key]
    rays = oacc.camera_rays(w, h, spp=spp, sample=sample).reshape(-1, 6)
    hits = oacc.intersect(rays, True)
    rest = oacc.intersect_rest(rays, True)
    hit = hits["tri"] != MISS
    assert np.array_equal(hit, hits["mesh"] != MISS)
    e = {"depth": hits["t"].copy(), "tri": hits["tri"].copy(), "mesh": hits["mesh"].copy(), "hit": hit}
    e["bary"] = np.stack([hits["u"], hits["v"]], axis=1)
    e["normal"] = np.where(hit[:, None], hits["normal"], np.float32(0.0)).astype(np.float32)
    # kd_tree_simd.hpp:254 in float: origin + (t * direction); the oracle's own hit<F>::position must be the same bits
    pos = (rays[:, 0:3] + (hits["t"][:, None] * rays[:, 3:6]).astype(np.float32)).astype(np.float32)
    e["position"] = np.where(hit[:, None], pos, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(_u32(e["position"][hit]), _u32(rest["position"][hit]))
    e["material"] = np.where(hit, f.mesh_material[np.where(hit, hits["mesh"], 0)].astype(np.uint32), np.uint32(MISS)).astype(np.uint32)
    assert (e["depth"][~hit] == -1.0).all() and not e["bary"][~hit].any()
    kind = f.mat_kind if materials is None else materials["kind"]
    alb = f.mat_albedo if materials is None else materials["albedo"]
    a = np.where(hit[:, None], alb[np.where(hit, e["material"], 0)], f.background[None, :]).astype(np.float32)
    e["albedo"] = a
    e["textured"] = hit & (kind[np.where(hit, e["material"], 0)] == TEXTURE)
    e["rays"] = rays
    return e


def _check_view(got, v, e, w, h, what, planes=PLANES, exact_normal=False):
    """view v of the planes `got` ([K, h, w(, c)]) against the expected planes `e` of that view"""
    n = w * h
    for name in planes:
        g = got[name][v].reshape(n, -1) if COMPS[name] > 1 else got[name][v].reshape(n)
        if name == "albedo":
            plain = ~e["textured"]
            assert np.array_equal(_u32(g[plain]), _u32(e["albedo"][plain])), (what, v, name)
        elif name == "normal" and not exact_normal:
            assert _same_normals(g, e["normal"]), (what, v, name)
        else:
            assert g.dtype == e[name].dtype and np.array_equal(_u32(g), _u32(e[name])), (what, v, name, int((_u32(g) != _u32(e[name])).sum()))


def _product_expected(rtk, acc, cfg, sample, flat=None):
    """the same planes from the product's own camera_rays + intersect(cull=True) under the accel's CURRENT camera"""
    rays = acc.camera_rays(cfg, sample).reshape(-1, 6)
    hits = acc.intersect(rays, True)
    hit = hits["tri"] != MISS
    e = {"depth": hits["t"], "tri": hits["tri"], "mesh": hits["mesh"], "bary": np.stack([hits["u"], hits["v"]], axis=1),
         "normal": hits["normal"], "hit": hit}
    pos = (rays[:, 0:3] + (hits["t"][:, None] * rays[:, 3:6]).astype(np.float32)).astype(np.float32)
    e["position"] = np.where(hit[:, None], pos, np.float32(0.0)).astype(np.float32)
    return e


def _check_product(rtk, acc_ref, got, v, cam, cfg, sample, what):
    if cam is not None:
        acc_ref.set_camera(cam[:3], cam[3:])
    e = _product_expected(rtk, acc_ref, cfg, sample)
    n = got["depth"][v].size
    for name in ("depth", "tri", "mesh", "bary", "normal", "position"):
        g = got[name][v].reshape(n, -1) if COMPS[name] > 1 else got[name][v].reshape(n)
        assert g.tobytes() == np.ascontiguousarray(e[name]).tobytes(), (what, v, name)       # rtk_hit's own bits, NaN payloads included


# ---------------------------------------------------------------- guarded buffers

def _guarded_host(k, h, w, names):
    bufs, views = {}, {}
    for name in names:
        n = k * h * w * COMPS[name]
        raw = np.full(GUARD + n + GUARD, SENTINEL, np.uint32)
        bufs[name] = raw
        body = raw[GUARD:GUARD + n]
        views[name] = (body.view(np.float32) if name in ("depth", "position", "normal", "albedo", "bary") else body).reshape(
            (k, h, w) + ((COMPS[name],) if COMPS[name] > 1 else ()))
    return bufs, views


def _guards_intact(raw):
    return (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()


def _host_call(rtk, acc, cfg, sample, views, k, wanted, allocated=PLANES):
    """rtk_render_gbuffer through the C-ABI into guarded buffers: all of `allocated` exist, only `wanted` are in the plane table"""
    w, h = cfg.width, cfg.height
    bufs, out = _guarded_host(k, h, w, allocated)
    gb = rtk.GBuffer(**{n: out[n].ctypes.data for n in wanted})
    p = cfg.to_c()
    vptr = None if views is None else np.ascontiguousarray(views, np.float32).ctypes.data
    rc = rtk.lib().rtk_render_gbuffer(acc._h, ctypes.byref(p), sample, vptr, k, ctypes.byref(gb))
    assert rc == rtk.RTK_OK, rtk.lib().rtk_last_error()
    for n in allocated:
        assert _guards_intact(bufs[n]), n
        if n not in wanted:
            assert (bufs[n] == SENTINEL).all(), n
    return {n: out[n] for n in wanted}


def _device_call(rtk, acc, cfg, sample, views, k, wanted, allocated=PLANES, stream=None):
    """rtk_render_gbuffer_device on a non-default torch stream; every plane starts 4 bytes behind a 16-byte boundary"""
    import torch
    w, h = cfg.width, cfg.height
    s = stream or torch.cuda.Stream()
    sent = int(np.array(SENTINEL, np.uint32).view(np.int32))
    raws, ptrs, sizes = {}, {}, {}
    for name in allocated:
        n = k * h * w * COMPS[name]
        raw = torch.full((GUARD + 1 + n + GUARD,), sent, dtype=torch.int32, device="cuda")
        assert raw.data_ptr() % 16 == 0
        raws[name], sizes[name] = raw, n
        ptrs[name] = raw.data_ptr() + 4 * (GUARD + 1)
        assert ptrs[name] % 16 == 4
    d_views = None
    if views is not None:
        pad = torch.zeros(1 + k * 12, dtype=torch.float32, device="cuda")
        pad[1:] = torch.from_numpy(np.ascontiguousarray(views, np.float32).reshape(-1)).cuda()
        d_views = pad
    torch.cuda.synchronize()
    acc.render_gbuffer_device(cfg, {n: ptrs[n] for n in wanted}, sample=sample,
                              d_views_ptr=0 if d_views is None else d_views.data_ptr() + 4, n_views=k, stream=s.cuda_stream)
    s.synchronize()
    out = {}
    for name in allocated:
        raw = raws[name].cpu().numpy().view(np.uint32)
        n = sizes[name]
        assert (raw[:GUARD + 1] == SENTINEL).all() and (raw[GUARD + 1 + n:] == SENTINEL).all(), name
        body = raw[GUARD + 1:GUARD + 1 + n]
        if name not in wanted:
            assert (body == SENTINEL).all(), name
            continue
        out[name] = (body.view(np.float32) if name in ("depth", "position", "normal", "albedo", "bary") else body).reshape(
            (k, h, w) + ((COMPS[name],) if COMPS[name] > 1 else ()))
    return out


# ---------------------------------------------------------------- 1. shapes

SIZES = [(70, 45), (9, 7), (8, 8), (1, 1), (16, 16)]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_shapes_views_and_samples(rtk, ora, size):
    """Cameras A, B, C of hw09/scene5 (C looks away: every wave ends at the root).  One view and three (at 70x45 a view has 54
    units: the workgroups straddle the views), views = NULL after set_camera, spp = 4 with samples 0 and 3."""
    w, h = size
    flat = _flat(ora, SCENE5)
    cams = cameras(flat)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    acc_ref = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    own = [x.copy() for x in acc.camera()]
    hits_seen = 0
    for spp, sample in ((1, 0), (4, 0), (4, 3)):
        cfg = rtk.RenderConfig(width=w, height=h, spp=spp)
        exp = {n: _expected(ora, flat, cams[n], w, h, spp, sample) for n in "ABC"}
        assert not exp["C"]["hit"].any()
        hits_seen += int(exp["A"]["hit"].sum()) + int(exp["B"]["hit"].sum())
        for names in ("A", "B", "C", "ABC", "CAB"):
            views = np.stack([cams[n] for n in names])
            got = acc.render_gbuffer(cfg, sample=sample, views=views)
            assert set(got) == set(PLANES)
            for v, n in enumerate(names):
                assert got["depth"].shape == (len(names), h, w) and got["position"].shape == (len(names), h, w, 3)
                _check_view(got, v, exp[n], w, h, (size, spp, sample, names))
                _check_product(rtk, acc_ref, got, v, cams[n], cfg, sample, (size, spp, sample, names))
        # a call with views leaves the accel's camera alone
        assert all(a.tobytes() == b.tobytes() for a, b in zip(own, acc.camera()))
        # views = NULL: the accel's camera, after set_camera
        acc.set_camera(cams["B"][:3], cams["B"][3:])
        got = acc.render_gbuffer(cfg, sample=sample)
        _check_view(got, 0, exp["B"], w, h, (size, spp, sample, "set_camera"))
        acc.set_camera(own[0], own[1])
        got = acc.render_gbuffer(cfg, sample=sample)
        _check_view(got, 0, exp["A"], w, h, (size, spp, sample, "own camera"))
    if w * h >= 256:
        assert hits_seen > 50, hits_seen
    # the jitter is in the rays: samples 0 and 3 of spp = 4 differ from each other and from the pixel centres
    if (w, h) == (70, 45):
        e0, e3, c = _expected(ora, flat, cams["A"], w, h, 4, 0), _expected(ora, flat, cams["A"], w, h, 4, 3), _expected(ora, flat, cams["A"], w, h, 1, 0)
        assert not np.array_equal(e0["depth"], e3["depth"]) and not np.array_equal(e0["depth"], c["depth"])


# ---------------------------------------------------------------- 2. plane subsets, guards, alignment

@pytest.mark.parametrize("variant", ["host", "device"])
def test_plane_subsets_guards_and_alignment(rtk, ora, variant):
    """Each plane alone, and all eight: the guards in front of and behind every buffer and the planes not asked for keep their
    bytes.  The device variant runs on a non-default stream into planes (and views) 4 bytes behind a 16-byte boundary."""
    w, h = 70, 45
    flat = _flat(ora, SCENE5)
    cams = cameras(flat)
    names = "BAC"
    views = np.stack([cams[n] for n in names])
    exp = [_expected(ora, flat, cams[n], w, h) for n in names]
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h)
    call = _host_call if variant == "host" else _device_call
    for wanted in [(p,) for p in PLANES] + [PLANES, ("depth", "mesh"), ("albedo", "material", "bary")]:
        got = call(rtk, acc, cfg, 0, views, 3, wanted)
        assert set(got) == set(wanted)
        for v in range(3):
            _check_view(got, v, exp[v], w, h, (variant, wanted), planes=wanted)
    # the accel's own camera through the same door (views = NULL, n_views = 1)
    got = call(rtk, acc, cfg, 0, None, 1, PLANES)
    _check_view(got, 0, exp[1], w, h, (variant, "own camera"))


# ---------------------------------------------------------------- 3. walks

def test_walk_of_a_tree_above_the_leaf_list_limit(rtk, ora):
    """scene5 built with max_depth = 12, max_leaf_size = 4 has more than 512 leaves (the oracle's tree: 631): trace() keeps the
    hierarchical walk there."""
    w, h = 70, 45
    flat = _flat(ora, SCENE5)
    cams = cameras(flat)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5), max_depth=12, max_leaf_size=4)
    assert acc.tree_info().n_leaves > 512, acc.tree_info().n_leaves
    kw = dict(max_depth=12, max_leaf=4)
    got = acc.render_gbuffer(rtk.RenderConfig(width=w, height=h), views=np.stack([cams["A"], cams["B"]]))
    for v, n in enumerate("AB"):
        e = _expected(ora, flat, cams[n], w, h, oracle_kw=kw)
        assert e["hit"].sum() > 100
        _check_view(got, v, e, w, h, ("deep tree", n))


def test_unnormalized_hit_normals(rtk, ora):
    """normalize_hit_normal = 0: the normal plane is rtk_hit.normal of such an accel, bit for bit, and no longer the oracle's
    normalised one; every other plane is the oracle's."""
    w, h = 70, 45
    flat = _flat(ora, SCENE5)
    cfg = rtk.RenderConfig(width=w, height=h)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5), normalize_hit_normal=False)
    acc_ref = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5), normalize_hit_normal=False)
    got = acc.render_gbuffer(cfg)
    e = _expected(ora, flat, None, w, h)
    _check_view(got, 0, e, w, h, "unnormalised", planes=tuple(p for p in PLANES if p != "normal"))
    _check_product(rtk, acc_ref, got, 0, None, cfg, 0, "unnormalised")
    hit = e["hit"]
    n = got["normal"][0].reshape(-1, 3)
    length = np.linalg.norm(n[hit].astype(np.float64), axis=1)
    assert hit.sum() > 100 and (np.abs(length - 1.0) > 1e-3).sum() > 50          # smooth-shaded: interpolated, not unit length
    assert not n[~hit].any()


def test_scene8(rtk, ora):
    w, h = 70, 45
    flat = _flat(ora, SCENE8)
    cams = cameras(flat)
    cfg = rtk.RenderConfig(width=w, height=h)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    acc_ref = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE8))
    got = acc.render_gbuffer(cfg, views=np.stack([cams["A"], cams["B"]]))
    for v, n in enumerate("AB"):
        e = _expected(ora, flat, cams[n], w, h)
        assert e["hit"].sum() > 100 and not e["textured"].any()
        _check_view(got, v, e, w, h, ("scene8", n))                                # (albedo: materials()[material] gathered, the background on a miss)
        _check_product(rtk, acc_ref, got, v, cams[n], cfg, 0, ("scene8", n))
    assert len(np.unique(got["material"][got["material"] != MISS])) >= 2


@pytest.mark.parametrize("path", [SCENE5, SCENE8], ids=["scene5", "scene8"])
def test_fast_traversal_depth_and_miss_mask(rtk, ora, path):
    """An RTK_TRAVERSAL_FAST accel: depth and the hit / miss pattern are the parity accel's, bit for bit (the other planes carry the
    tie caveat and are not asserted)."""
    w, h = 70, 45
    cams = cameras(_flat(ora, path))
    views = np.stack([cams["A"], cams["B"]])
    cfg = rtk.RenderConfig(width=w, height=h)
    parity = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path)).render_gbuffer(cfg, views=views)
    fast = rtk.KdTreeSimdAccel(rtk.parse_scene_file(path), traversal=rtk.TRAVERSAL_FAST).render_gbuffer(cfg, views=views)
    assert (parity["tri"] != MISS).sum() > 200
    assert np.array_equal(_u32(fast["depth"]), _u32(parity["depth"]))
    for name in ("tri", "mesh", "material"):
        assert np.array_equal(fast[name] == MISS, parity[name] == MISS), name


# ---------------------------------------------------------------- 4. albedo, pinned to the oracle's frames

def _white(flat):
    f = flat
    for m in range(len(flat.mat_kind)):
        f = with_material(f, m, kind=DIFFUSE, albedo=[1.0, 1.0, 1.0])
    return f


def _check_albedo_against_frames(ora, flat, got, w, h, what, min_pixels=500, kinds=None):
    """k * albedo_plane == the oracle's frame, per channel and by bits, on every pixel whose material plane names a texture material
    and whose k (the same pixel of the all-white-diffuse scene) is non-zero.  Returns {texture kind: such pixels}."""
    frame = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(w, h, 1, 5, 0)[0].reshape(-1, 3)
    k3 = ora.Accel(ora.Scene(_white(flat)), ora.ACCEL_KD_SIMD).render(w, h, 1, 5, 0)[0].reshape(-1, 3)
    mat = got["material"][0].reshape(-1)
    alb = got["albedo"][0].reshape(-1, 3)
    hit = mat != MISS
    textured = hit & (flat.mat_kind[np.where(hit, mat, 0)] == TEXTURE)
    kt = k3[textured]                                            # white: one k for the three channels of a hit
    assert np.array_equal(_u32(kt[:, 0]), _u32(kt[:, 1])) and np.array_equal(_u32(kt[:, 0]), _u32(kt[:, 2]))
    lit = textured & (k3[:, 0] != 0.0)
    prod = (k3[lit] * alb[lit]).astype(np.float32)
    assert np.array_equal(_u32(prod), _u32(frame[lit])), (what, int((_u32(prod) != _u32(frame[lit])).any(axis=1).sum()))
    tex_kind = flat.tex_kind[flat.mat_texture[np.where(textured, mat, 0)]]
    counts = {}
    for kind in (kinds if kinds is not None else sorted(set(flat.tex_kind.tolist()))):
        sel = lit & (tex_kind == kind)
        counts[kind] = int(sel.sum())
        assert counts[kind] >= min_pixels, (what, kind, counts)
    return lit, tex_kind, alb


def test_albedo_of_texture_materials_is_what_color_hit_lights(rtk, ora):
    """hw12/scene4 at 160x90: one light, four texture materials, one per texture kind."""
    w, h = 160, 90
    flat = _flat(ora, SCENE4_TEX)
    assert len(flat.light_intensity) == 1 and (flat.mat_kind == TEXTURE).sum() == 4
    assert sorted(flat.tex_kind[flat.mat_texture[flat.mat_kind == TEXTURE]].tolist()) == [0, EDGES, CHECKER, BITMAP]
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE4_TEX))
    got = acc.render_gbuffer(rtk.RenderConfig(width=w, height=h))
    e = _expected(ora, flat, None, w, h)
    _check_view(got, 0, e, w, h, "scene4")                       # every other plane, the background on the misses
    assert (~e["hit"]).sum() > 5000 and e["textured"].sum() > 2000
    lit, tex_kind, alb = _check_albedo_against_frames(ora, flat, got, w, h, "scene4")
    for kind in (EDGES, CHECKER, BITMAP):
        assert len(np.unique(_u32(alb[lit & (tex_kind == kind)]), axis=0)) >= 2, kind
    assert len(np.unique(_u32(alb[lit & (tex_kind == 0)]), axis=0)) == 1


def test_albedo_of_plain_materials_and_of_misses(rtk, ora):
    """scene5: albedo == materials()[material] gathered, and background() on the misses, as the accel itself reports them."""
    w, h = 70, 45
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    got = acc.render_gbuffer(rtk.RenderConfig(width=w, height=h), planes=("albedo", "material"))
    mat = got["material"][0].reshape(-1)
    hit = mat != MISS
    assert hit.sum() > 100 and (~hit).sum() > 100
    table = acc.materials()["albedo"]
    want = np.where(hit[:, None], table[np.where(hit, mat, 0)], acc.background()[None, :]).astype(np.float32)
    assert np.array_equal(_u32(got["albedo"][0].reshape(-1, 3)), _u32(want))


# ---------------------------------------------------------------- 5. live state

def test_planes_follow_the_live_state(rtk, ora):
    """One accel of hw12/scene4 walked through set_materials, set_textures / set_texture_pixels, set_background, update_vertices,
    update_geometry and update_vertices_device on one stream with the g-buffer call on another: after each step the planes are
    those of the changed scene."""
    import torch
    w, h = 160, 90
    cfg = rtk.RenderConfig(width=w, height=h)
    base = _flat(ora, SCENE4_TEX)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE4_TEX))
    seen = []

    def check(flat, what, frames=True, min_pixels=20):
        got = acc.render_gbuffer(cfg)
        e = _expected(ora, flat, None, w, h)
        _check_view(got, 0, e, w, h, what)
        if frames:
            kinds = sorted(set(flat.tex_kind[flat.mat_texture[flat.mat_kind == TEXTURE]].tolist()))
            _check_albedo_against_frames(ora, flat, got, w, h, what, min_pixels=min_pixels, kinds=kinds)
        seen.append({n: got[n].copy() for n in PLANES})
        return got

    check(base, "built")
    # a texture material becomes diffuse
    tm = int(np.flatnonzero(base.mat_kind == TEXTURE)[0])
    s1 = with_material(base, tm, kind=DIFFUSE, albedo=[0.25, 0.5, 0.75])
    set_materials(acc, s1)
    got = check(s1, "set_materials")
    sel = got["material"][0] == tm
    assert sel.sum() > 100 and (got["albedo"][0][sel] == np.array([0.25, 0.5, 0.75], np.float32)).all()
    # the texture table, then the texels of the bitmap
    texs = textures_of(s1)
    texs[1] = Tex(EDGES, (0.9, 0.8, 0.1), (0.1, 0.2, 0.7), 0.11)
    texs[2] = Tex(CHECKER, (0.2, 0.9, 0.9), (0.6, 0.1, 0.4), 0.3)
    s2 = with_textures(s1, texs)
    set_textures(acc, s2)
    check(s2, "set_textures")
    texs[3] = Tex(BITMAP, pixels=np.random.default_rng(21).integers(0, 256, (9, 13, 3), dtype=np.uint8))
    s3 = with_textures(s2, texs)
    acc.set_texture_pixels(3, texs[3].pixels)
    check(s3, "set_texture_pixels")
    # the background
    s4 = dataclasses.replace(s3, background=np.array([0.125, -0.0, 3.0], np.float32))
    acc.set_background(s4.background)
    got = check(s4, "set_background")
    miss = got["material"][0] == MISS
    assert miss.sum() > 5000 and np.array_equal(_u32(got["albedo"][0][miss]), np.broadcast_to(_u32(s4.background), (int(miss.sum()), 3)))
    # moved vertices: the oracle rebuilt from them
    moved = (base.vertices + 0.15 * np.sin(np.arange(base.vertices.size, dtype=np.float32)).reshape(-1, 3)).astype(np.float32)
    s5 = dataclasses.replace(s4, vertices=moved)
    acc.update_vertices(moved)
    check(s5, "update_vertices")
    # 3/4 of the triangles of every mesh
    ntris = (base.mesh_ntris * 3 // 4).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(base.mesh_ntris)[:-1]])
    idx = np.ascontiguousarray(np.concatenate([base.indices[f:f + n] for f, n in zip(first, ntris)]).astype(np.uint32))
    s6 = dataclasses.replace(s5, indices=idx, mesh_ntris=ntris)
    acc.update_geometry(moved, idx, ntris)
    check(s6, "update_geometry")
    # update_vertices_device on one stream, the g-buffer on another: it waits for the geometry on the device
    moved2 = (moved + np.array([0.0, 0.2, -0.1], np.float32)).astype(np.float32)
    s7 = dataclasses.replace(s6, vertices=moved2)
    d_v = torch.from_numpy(moved2).cuda()
    torch.cuda.synchronize()
    s_up, s_gb = torch.cuda.Stream(), torch.cuda.Stream()
    acc.update_vertices_device(d_v.data_ptr(), s_up.cuda_stream)
    got = _device_call(rtk, acc, cfg, 0, None, 1, PLANES, stream=s_gb)
    s_up.synchronize()
    e = _expected(ora, s7, None, w, h)
    _check_view(got, 0, e, w, h, "update_vertices_device")
    seen.append(got)
    # no step was a no-op: consecutive states differ in some plane
    for a, b in zip(seen, seen[1:]):
        assert any(a[n].tobytes() != b[n].tobytes() for n in PLANES)


# ---------------------------------------------------------------- 6. frames are left alone

def test_frames_counters_and_camera_are_left_alone(rtk, ora):
    """GROUP4 frame x 3, a g-buffer call, a frame: the last frame is the third's bits and `rays`, issues no counter fill (the steady
    state survived), and the g-buffer call issued none either; camera() is unchanged after a call with views."""
    import torch
    w, h = 320, 180
    flat = _flat(ora, SCENE5)
    cams = cameras(flat)
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=rtk.TRACE_GROUP4)
    s = torch.cuda.current_stream()

    def frame():
        buf = torch.full((acc.output_floats(cfg),), float("nan"), dtype=torch.float32, device="cuda")
        before = acc.counter_fills()
        acc.render_frame_device(cfg, buf.data_ptr(), s.cuda_stream)
        cn = acc.last_counters()
        return buf.cpu().numpy(), cn, acc.counter_fills() - before

    frames = [frame() for _ in range(3)]
    assert [f[2] for f in frames] == [1, 1, 0]
    own = [x.copy() for x in acc.camera()]
    fills = acc.counter_fills()
    views = np.stack([cams["B"], cams["C"], cams["A"]])
    got = acc.render_gbuffer(cfg, views=views)
    d = _device_call(rtk, acc, cfg, 0, views, 3, ("depth", "mesh"))
    assert acc.counter_fills() == fills
    assert all(a.tobytes() == b.tobytes() for a, b in zip(own, acc.camera()))
    assert acc.last_counters() == frames[2][1]                       # rtk_render_last_counters still reports the frame
    assert np.array_equal(_u32(d["depth"]), _u32(got["depth"])) and (got["mesh"] != MISS).sum() > 1000
    last = frame()
    assert last[2] == 0                                              # still steady: no fill for the frame behind the g-buffer call
    assert np.array_equal(_u32(last[0]), _u32(frames[2][0])) and last[1]["rays"] == frames[2][1]["rays"]
    ref, ocn = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(w, h, 1, 5, 0)
    assert np.array_equal(_u32(last[0]), _u32(ref).reshape(-1)) and last[1]["rays"] == ocn["rays"]
