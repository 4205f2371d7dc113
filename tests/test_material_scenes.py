"""The generated material scenes (tests/material_scenes.py) without a GPU: the generator still makes the recorded scenes, the
CPU oracle reproduces what the reference wrote for them (tests/golden/ref_probe/material_*), and the recorded data reach the
cases they were made for.

Nothing has a tolerance; the one allowance is ref_probe_cases.same_frame, where a NaN only has to be a NaN (none of the recorded
arrays holds one, see test_recorded_nans).  The census conditions are floors that keep a case from being empty, not measurements.

Rays exactly along a glass face's normal: normalized(i + cos_i_n * n) normalises a zero vector there, so the refraction ray's
direction is NaN.  The reference then finds no hit for that ray (every comparison of the triangle test rejects a NaN), a miss
adds nothing, and the Fresnel factor at cos = 1 is 0, which removes the reflection: the recorded radiance of these rays is
exactly zero, not NaN.  test_normal_incidence asserts both halves, the NaN direction from the restated arithmetic and the zeros
from the recording, and the call counts pin that the NaN ray was traced.

The reference's probe finds first hits with back-face culling, so no recorded ray meets a flat glass face from inside.  Normal
incidence from inside, origins inside the inner mesh and the critical angles of the exit are material_scenes.unculled_radiance_rays:
the census here shows what they reach, and the GPU is compared on them with the oracle (cull = 0), not with a recording."""
import dataclasses

import numpy as np
import pytest

import material_scenes as ms
import ref_probe_cases as rc
from occlusion_model import dot3, normalized3

NAMES = rc.material_fixture_names()              # fixture name -> variant
_flats, _oaccs = {}, {}


@pytest.fixture(scope="module")
def fixtures():
    return {name: rc.load_fixture(name) for name in NAMES}


def _flat(ora, variant):
    if variant not in _flats:
        _flats[variant] = ms.make_scene(ora, variant)
    return _flats[variant]


def _oacc(ora, variant, W=8):
    if (variant, W) not in _oaccs:
        _oaccs[variant, W] = ora.Accel(ora.Scene(_flat(ora, variant)), ora.ACCEL_KD_SIMD, W=W)
    return _oaccs[variant, W]


# ================================================================ the generator

@pytest.mark.parametrize("name", list(NAMES))
def test_generator_makes_the_recorded_scene(ora, fixtures, name):
    fx, flat = fixtures[name], _flat(ora, NAMES[name])
    arrays = ms.scene_arrays(flat)
    assert set(arrays) == {k for k in fx if k.startswith("scene_")}
    for k, v in arrays.items():
        assert rc.same_bits(v, fx[k]), (name, k)
    rays, masks = ms.radiance_rays(ora, flat, _oacc(ora, NAMES[name]))
    assert rc.same_bits(rays, fx["rad_rays"]), name
    q, t, _ = ms.stacked_glass_queries()
    assert rc.same_bits(q, fx["occ_rays"]) and rc.same_bits(t, fx["occ_max_t"]), name


def test_variants_are_what_the_issue_lists(ora):
    assert [ms.IORS[v] for v in ms.GLASS_VARIANTS[:5]] == [(1.5, 0.75), (0.75, 1.5), (1.0, 0.0), (2.4, 1.0), (1.5, -1.5)]
    base, swapped, tex = (_flat(ora, v) for v in ("ior15_075", "swapped", "textured"))
    assert (base.mat_smooth[ms.M_OUTER], base.mat_smooth[ms.M_INNER]) == (0, 1)
    assert (swapped.mat_smooth[ms.M_OUTER], swapped.mat_smooth[ms.M_INNER]) == (1, 0)
    assert not base.mat_albedo[ms.M_BLACK].any() and base.mat_kind[ms.M_BLACK] == ms.DIFFUSE and base.mat_kind[ms.M_CONST] == ms.CONSTANT
    for v in ms.VARIANTS:                           # one geometry, texture table and camera: set_materials / set_lights walk them
        f = _flat(ora, v)
        for k in ("vertices", "indices", "uvs", "mesh_has_uvs", "tex_kind", "tex_param", "tex_pixels", "tex_bitmap", "cam_pos", "cam_mat"):
            assert rc.same_bits(getattr(f, k), getattr(base, k)), (v, k)
        assert 10 <= int(f.mesh_ntris.sum()) <= 400
    # textures: every kind, the edge widths, a power-of-two square, the bitmap sizes; uvs past [0, 1], grid lines at 0 and 1
    assert sorted(tex.tex_param[tex.tex_kind == ms.EDGES].tolist()) == [0.0, np.float32(0.05), np.float32(0.4)]
    assert tex.tex_param[ms.T_CHECKER] == 0.25
    assert sorted((int(w), int(h)) for _, w, h in tex.tex_bitmap[tex.tex_kind == ms.BITMAP]) == [(1, 1), (3, 5), (16, 16)]
    used = tex.mat_texture[tex.mat_kind == ms.TEXTURE]
    assert set(used.tolist()) == set(range(8))
    assert tex.mat_kind[ms.M_PYRAMID] == ms.TEXTURE and tex.mesh_has_uvs[ms.PYRAMID] == 0
    uv = tex.uvs
    assert uv.min() < 0 and uv.max() > 1 and (uv == 0).any() and (uv == 1).any()
    assert uv[:, 0].min() * 16 > -1 and (1.0 - uv[:, 1].max()) * 16 > -1          # bitmap lookups stay where the reference is defined
    # lights
    pos = {v: ms.light_rows(v) for v in ms.VARIANTS}
    assert any((i == 0).any() for _, i in pos.values()) and any((i < 0).any() for _, i in pos.values())
    assert any((p[:, 1] == ms.FLOOR_Y).any() for p, _ in pos.values())
    inside = lambda p: ((ms.BOX_LO < p) & (p < ms.BOX_HI)).all(axis=1)
    assert any(inside(p).any() for p, _ in pos.values())
    assert max(len(i) for _, i in pos.values()) >= 9


def test_first_hit_albedo_is_what_color_hit_lights(ora):
    """ora_first_hit_albedo (the oracle's own sample_texture behind an entry point) against the oracle's frames: under one light a
    texture material leaves k * sample(texture, hit, uvs), and the same scene with white diffuse materials leaves k
    (render.hpp:205, 235); depth 1 keeps mirrors and glass out of it."""
    flat = _flat(ora, "textured")
    seen = set()
    for light in ((3.0, 8.0, 6.0), (-4.0, 6.0, 2.0)):
        one = dataclasses.replace(flat, light_pos=np.array([light], np.float32), light_intensity=np.array([700.0], np.float32))
        white = dataclasses.replace(one, mat_kind=np.zeros_like(flat.mat_kind), mat_albedo=np.ones_like(flat.mat_albedo))
        oa = ora.Accel(ora.Scene(one), ora.ACCEL_KD_SIMD)
        frame = oa.render(*ms.SIZE, 1, 1, 0)[0].reshape(-1, 3)
        k3 = ora.Accel(ora.Scene(white), ora.ACCEL_KD_SIMD).render(*ms.SIZE, 1, 1, 0)[0].reshape(-1, 3)
        rays = oa.camera_rays(*ms.SIZE).reshape(-1, 6)
        hits = oa.intersect(rays, True)
        hit = hits["mesh"] != ms.MISS
        mat = one.mesh_material[np.where(hit, hits["mesh"], 0)]
        rgb = oa.first_hit_albedo(rays, True)
        textured = hit & (one.mat_kind[mat] == ms.TEXTURE)
        plain = hit & ~textured
        assert rc.same_bits(rgb[plain], one.mat_albedo[mat[plain]]) and rc.same_bits(rgb[~hit], np.tile(one.background, ((~hit).sum(), 1)))
        lit = textured & (k3[:, 0] != 0)
        assert lit.sum() >= 300
        assert rc.same_bits((k3[lit] * rgb[lit]).astype(np.float32), frame[lit])
        tex = one.mat_texture[mat[lit]]
        seen |= set(tex.tolist())
        for t in (ms.T_EDGE005, ms.T_CHECKER, ms.T_BMP3X5, ms.T_BMP16):     # (an edge width of 0.4 >= 1/3 is all edge, 0 is none)
            if (tex == t).sum() >= 8:
                assert len(np.unique(rgb[lit][tex == t], axis=0)) >= 2, t           # the lookup varies over the quad
    assert seen == set(range(8))


# ================================================================ the oracle against the recording

@pytest.mark.parametrize("name", list(NAMES))
def test_oracle_tree(ora, fixtures, name):
    fx = fixtures[name]
    for i, W in enumerate(rc.WIDTHS):
        oa = _oacc(ora, NAMES[name], W)
        box, link, refs = oa.dump()
        assert rc.same_bits(box, fx["tree_box"]) and rc.same_bits(link, fx["tree_link"]) and rc.same_bits(refs, fx["tree_refs"]), W
        assert oa.num_packets == fx["tree_packets"][i], W


@pytest.mark.parametrize("depth", ms.DEPTHS)
@pytest.mark.parametrize("name", list(NAMES))
def test_oracle_frame(ora, fixtures, name, depth):
    fx = fixtures[name]
    for W in rc.WIDTHS:
        rgb, cn = _oacc(ora, NAMES[name], W).render(*ms.SIZE, 1, depth, 0)
        assert rc.same_frame(rgb, fx[f"frame_d{depth}"]), (W, rc.first_difference(fx[f"frame_d{depth}"], rgb))
        assert (cn["rays"], cn["hits"]) == tuple(fx[f"frame_calls_d{depth}"]), W


@pytest.mark.parametrize("depth", ms.RAD_DEPTHS)
@pytest.mark.parametrize("name", list(NAMES))
def test_oracle_radiance(ora, fixtures, name, depth):
    """The special rays and the view batch through the oracle's color_hit (ora_radiance: intersect<true>, then color_hit)."""
    fx = fixtures[name]
    for W in rc.WIDTHS:
        rgb, cn = _oacc(ora, NAMES[name], W).radiance(fx["rad_rays"], depth)
        assert rc.same_frame(rgb, fx[f"rad_rgb_d{depth}"]), (W, rc.first_difference(fx[f"rad_rgb_d{depth}"], rgb))
        assert cn["rays"] == fx[f"rad_calls_d{depth}"][0] and cn["primary"] == len(rgb), W


def test_oracle_radiance_is_the_oracles_frame(ora):
    """ora_radiance against the frame path it was cut from: a frame with spp = 1 is the radiance of its camera rays."""
    for v in ("ior15_075", "textured"):
        oa = _oacc(ora, v)
        frame, fcn = oa.render(*ms.SIZE, 1, 10, 0)
        rgb, cn = oa.radiance(oa.camera_rays(*ms.SIZE).reshape(-1, 6), 10)
        assert rc.same_bits(rgb, frame.reshape(-1, 3)) and cn["rays"] == fcn["rays"]
    oa = _oacc(ora, "ior15_075")                     # and with GI: the keys are those of the frame's pixels
    frame, fcn = oa.render(*ms.SIZE, 1, 3, 2)
    rgb, cn = oa.radiance(oa.camera_rays(*ms.SIZE).reshape(-1, 6), 3, diffuse_rays=2)
    assert rc.same_bits(rgb, frame.reshape(-1, 3)) and cn["rays"] == fcn["rays"]


@pytest.mark.parametrize("name", list(NAMES))
def test_oracle_occluded(ora, fixtures, name):
    fx, flat = fixtures[name], _flat(ora, NAMES[name])
    for W in rc.WIDTHS:
        want, calls = rc.model_occluded(_oacc(ora, NAMES[name], W), flat, fx["occ_rays"], fx["occ_max_t"])
        assert np.array_equal(want, fx["occ_answer"]), (W, np.flatnonzero(want != fx["occ_answer"])[:8])
        assert calls == fx["occ_calls"][0], W


# ================================================================ the census: the recorded cases are not empty

def _census(ora, variant, special):
    flat, oa = _flat(ora, variant), _oacc(ora, variant)
    if not special:
        return ms.census(ora, flat, oacc=oa)
    rays, masks = ms.radiance_rays(ora, flat, oa)
    return ms.census(ora, flat, rays[~masks["view"]], oa)


def test_census_every_kind_is_a_first_hit(ora, fixtures):
    for v in ms.GLASS_VARIANTS:
        c = _census(ora, v, False)
        print(v, c)
        for kind in (ms.DIFFUSE, ms.REFLECTIVE, ms.REFRACTIVE, ms.CONSTANT):
            assert c[f"kind_{kind}"] >= 32, (v, kind, c)
    c = _census(ora, "textured", False)
    print("textured", c)
    assert c[f"kind_{ms.TEXTURE}"] >= 32
    for kind in (ms.ALBEDO, ms.EDGES, ms.CHECKER, ms.BITMAP):
        assert c[f"tex_{kind}"] >= 32, (kind, c)


def test_census_refraction_branches(ora):
    """TIR and refraction, entering and leaving, and smooth refractive hits whose two normals differ: at least 16 primary or
    special rays each, summed over the variants; printed per variant."""
    total = {}
    for v in ms.VARIANTS:
        for special in (False, True):
            c = _census(ora, v, special)
            print(v, "special" if special else "camera", {k: c[k] for k in ("tir_entry", "tir_exit", "refract_entry", "refract_exit", "smooth_differs")})
            if not special:
                assert c["tir_exit"] + c["refract_exit"] == 0 or ms.material_rows(v)["smooth"][ms.M_OUTER] == 1     # flat faces: culled
            for k, n in c.items():
                total[k] = total.get(k, 0) + n
    for k in ("tir_entry", "tir_exit", "refract_entry", "refract_exit", "smooth_differs"):
        assert total[k] >= 16, (k, total)
    # what each ior pair is there for (refract_at: eta_r / eta_i < sin_i_n)
    assert _census(ora, "ior075_15", True)["tir_entry"] >= 16 and _census(ora, "ior075_15", True)["tir_exit"] >= 16
    assert _census(ora, "ior15_m15", True)["tir_entry"] >= 16          # a negative ior: every entry is total reflection
    assert _census(ora, "ior10_00", True)["refract_exit"] >= 16         # ior 0 on the way out: eta_r / eta_i is +inf
    assert _census(ora, "swapped", False)["smooth_differs"] >= 32       # the smooth box in front of the camera


def _critical_rows(ora, variant, side):
    """-> [(mesh, ratio, refractive [6, 8], leaving [6, 8], tir [6, 8], on the aimed mesh [6, 8])] per group of critical rays"""
    flat, oa = _flat(ora, variant), _oacc(ora, variant)
    cull = side == "entry"
    rays, masks = (ms.special_radiance_rays if cull else ms.unculled_radiance_rays)(ora, flat, oa)
    r = rays[masks["critical" if cull else "critical_exit"]]
    groups = ms.critical_groups(flat, side)
    shape = (len(ms.DELTAS), ms.N_AZ)
    assert len(r) == len(groups) * shape[0] * shape[1]
    if not groups:
        return []
    hits, rest = oa.intersect(r, cull), oa.intersect_rest(r, cull)
    refractive, leaving, tir = ms.refraction_case(flat, r, hits, rest)
    n = shape[0] * shape[1]
    return [(mesh, ratio) + tuple(a[g * n:(g + 1) * n].reshape(shape) for a in (refractive, leaving, tir, hits["mesh"] == mesh))
            for g, (mesh, ratio) in enumerate(groups)]


def test_census_critical_rays_straddle_the_critical_angle(ora):
    """Per (ior, face) group: every ray's first hit is the aimed glass face; the rows with delta < 0 refract and the rows with
    delta > 0 take total reflection, down to +-1e-6 rad.  On entry for every ior in (0, 1), on exit for every ior above 1; and
    every variant has the groups its iors allow (ior 1, 0 and -1.5 have no critical angle)."""
    expected = {"ior15_075": (2, 2), "ior075_15": (2, 2), "ior10_00": (0, 0), "ior24_10": (0, 2), "ior15_m15": (0, 2),
                "swapped": (2, 2), "textured": (2, 2)}                  # groups on entry, on exit
    below = np.array(ms.DELTAS) < 0
    assert below.sum() == 3 and (~below).sum() == 3 and min(abs(d) for d in ms.DELTAS) == 1e-6
    for v in ms.VARIANTS:
        for k, side in enumerate(("entry", "exit")):
            rows = _critical_rows(ora, v, side)
            assert len(rows) == expected[v][k], (v, side)
            for mesh, ratio, refractive, leaving, tir, on_mesh in rows:
                print(v, side, "mesh", mesh, "ratio", ratio, "TIR per row", tir.sum(axis=1))
                assert on_mesh.all() and refractive.all() and (leaving == (side == "exit")).all(), (v, side, mesh)
                assert not tir[below].any() and tir[~below].all(), (v, side, mesh, tir.sum(axis=1))
    # both exit ratios and the entry ratio are there, on the flat and on the smooth mesh
    ratios = {(side, round(r[1], 3)) for v in ms.VARIANTS for side in ("entry", "exit") for r in _critical_rows(ora, v, side)}
    assert ratios == {("entry", 0.75), ("exit", round(1 / 1.5, 3)), ("exit", round(1 / 2.4, 3))}


def test_census_unculled_rays_start_inside_the_glass(ora):
    """Without culling the first hit of normal_inside is the box from inside at exactly normal incidence (the refraction
    direction restated here is NaN), and that of inside_inner the octahedron from inside."""
    for v in ms.VARIANTS:
        flat, oa = _flat(ora, v), _oacc(ora, v)
        rays, masks = ms.unculled_radiance_rays(ora, flat, oa)
        hits, rest = oa.intersect(rays, False), oa.intersect_rest(rays, False)
        refractive, leaving, tir = ms.refraction_case(flat, rays, hits, rest)
        m = masks["normal_inside"]
        assert m.sum() >= 16 and (hits["mesh"][m] == ms.BOX).all() and leaving[m].all(), v
        if v != "swapped":
            with np.errstate(all="ignore"):
                n = -normalized3(ms.shading_normal(flat, hits, rest)[m])
                i = normalized3(rays[m][:, 3:6])
                cos_i = -dot3(i, n)
                assert (cos_i == 1).all() and np.isnan(normalized3(i + cos_i[:, None] * n)).all(), v
        m = masks["inside_inner"]
        assert m.sum() >= 32 and (hits["mesh"][m] == ms.OCTA).all() and leaving[m].all(), v
        culled = oa.intersect(rays[m | masks["normal_inside"]], True)      # why the probe cannot record them: culled, they pass
        assert not np.isin(culled["mesh"], (ms.BOX, ms.OCTA)).any(), v


def test_census_into_inner_enters_glass_from_glass(ora):
    for v in ms.VARIANTS:
        flat, oa = _flat(ora, v), _oacc(ora, v)
        rays, masks = ms.special_radiance_rays(ora, flat, oa)
        r = rays[masks["into_inner"]]
        hits, rest = oa.intersect(r, True), oa.intersect_rest(r, True)
        refractive, leaving, _ = ms.refraction_case(flat, r, hits, rest)
        assert len(r) >= 32 and (hits["mesh"] == ms.OCTA).all() and (refractive & ~leaving).sum() >= 32, v
        assert ((ms.BOX_LO < r[:, :3]) & (r[:, :3] < ms.BOX_HI)).all()


def test_normal_incidence(ora, fixtures):
    """See the module's docstring: a NaN refraction direction (restated here), and exact zeros in the recording."""
    for name, v in NAMES.items():
        flat, oa = _flat(ora, v), _oacc(ora, v)
        rays, masks = ms.radiance_rays(ora, flat, oa)
        r = rays[masks["normal_outside"]]
        hits, rest = oa.intersect(r, True), oa.intersect_rest(r, True)
        assert (hits["mesh"] == ms.BOX).all() and len(r) >= 64
        with np.errstate(all="ignore"):
            n = normalized3(ms.shading_normal(flat, hits, rest))
            i = normalized3(r[:, 3:6])
            cos_i = -dot3(i, n)
            tangent = normalized3(i + cos_i[:, None] * n)
        if v != "swapped":                                  # (the smooth box's hit normals lean away from the face normal)
            assert (cos_i == 1).all() and np.isnan(tangent).all(), v
            for d in ms.RAD_DEPTHS:
                rgb = fixtures[name][f"rad_rgb_d{d}"][masks["normal_outside"]]
                assert rc.same_bits(rgb, np.zeros_like(rgb)), (v, d)


def test_census_depth(fixtures):
    for name in NAMES:
        fx = fixtures[name]
        rays = [int(fx[f"frame_calls_d{d}"][0]) for d in ms.DEPTHS]
        print(name, "rays by depth", rays)
        assert rays[0] < rays[1] < rays[2] < rays[3] <= 1_000_000, (name, rays)
        assert not rc.same_frame(fx["frame_d16"], fx["frame_d10"]), name
        assert not rc.same_frame(fx["frame_d10"], fx["frame_d5"]) and not rc.same_frame(fx["frame_d5"], fx["frame_d1"]), name


def test_recorded_nans(fixtures):
    """The NaN allowance of same_frame cannot hide a frame: at most 2 % of a recorded frame is NaN, and no view batch holds one."""
    for name in NAMES:
        fx = fixtures[name]
        for d in ms.DEPTHS:
            assert np.isnan(fx[f"frame_d{d}"]).mean() <= 0.02, (name, d)
        n_view = 32 * 32
        for d in ms.RAD_DEPTHS:
            assert not np.isnan(fx[f"rad_rgb_d{d}"][-n_view:]).any(), (name, d)


def test_census_stacked_glass(ora, fixtures):
    """The queries cross 0 to 4 glass surfaces before the opaque quad; for each count some end between the surfaces (clear after
    that many steps or fewer) and some reach the quad (occluded)."""
    from occlusion_model import occluded_ref
    rays, max_t, surfaces = ms.stacked_glass_queries()
    flat = _flat(ora, "ior15_075")
    answer, steps = occluded_ref(_oacc(ora, "ior15_075"), flat, rays, max_t, rc.BIAS)
    assert np.array_equal(answer, fixtures["material_ior15_075"]["occ_answer"])
    assert (steps <= surfaces).all()
    for k in range(5):
        sel = surfaces == k
        assert ((answer == 1) & sel & (steps == k)).sum() >= 2, k                   # through k glass surfaces onto the quad
        assert set(steps[sel & (answer == 0)].tolist()) >= set(range(k + 1)), k     # max_t ends after 0, 1, .., k of them


# ================================================================ against the live probe

def test_live_fixtures_are_what_the_probe_writes_now(ora, fixtures):
    if not all(ora.ref_available(8, d) for d in ms.DEPTHS):
        pytest.skip("oracle/_ref/ holds no probe: __graft_entry__.build() makes it where a checkout of the reference is present")
    if [w for w in rc.WIDTHS if ora.ref_available(w, 5)] != list(rc.WIDTHS):
        pytest.skip("this host cannot run the 16-wide probe that the fixtures' packet counts come from")
    for name, v in NAMES.items():
        arrays, _ = rc.record_material(ora, _flat(ora, v))
        assert set(arrays) == set(fixtures[name])
        for k, a in arrays.items():
            assert rc.same_bits(a, fixtures[name][k]), (name, k)


def test_live_widths_agree(ora):
    """On the reference itself the packet widths give one and the same frame and radiance at depth 16."""
    widths = [w for w in rc.WIDTHS if ora.ref_available(w, 16)]
    if len(widths) < 2:
        pytest.skip("oracle/_ref/ holds no depth-16 probes for two widths")
    for v in ("ior075_15", "textured"):
        flat = _flat(ora, v)
        rays, _ = ms.radiance_rays(ora, flat, _oacc(ora, v))
        got = []
        for w in widths:
            p = ora.RefProbe(flat, w, 16, size=ms.SIZE)
            got.append((p.frame(), p.calls, p.radiance(rays), p.calls))
        for g in got[1:]:
            assert rc.same_bits(g[0], got[0][0]) and rc.same_bits(g[2], got[0][2]) and (g[1], g[3]) == (got[0][1], got[0][3]), v
