"""tests/occlusion_model.py (the reference's is_occluded loop in numpy) pinned to the oracle's own renders, and the
host-side behaviour of the batched occlusion entry points that needs no device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENE2, SCENE5, SCENE8
from occlusion_model import MISS, camera_hits, dot3, normalized3, occluded_ref, shadow_queries

W, H = 480, 270
PI_F = np.float32(3.14159265358979323846)


def _face_normals(flat, tri):
    """triangle::normal (scene/object/triangle.hpp:20-30) of the global triangles `tri`: normalized(cross(v1 - v0, v2 - v0))."""
    vbase = np.concatenate([[0], np.cumsum(flat.mesh_nverts)[:-1]])
    tri_mesh = np.repeat(np.arange(len(flat.mesh_ntris)), flat.mesh_ntris)
    ix = flat.indices[tri].astype(np.int64) + vbase[tri_mesh[tri]][:, None]
    v0, v1, v2 = flat.vertices[ix[:, 0]], flat.vertices[ix[:, 1]], flat.vertices[ix[:, 2]]
    a, b = v1 - v0, v2 - v0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    return normalized3(c)


def diffuse_pixels_from_the_model(ora, scene, depth):
    """-> (colour float32[m,3] from the helper, the oracle's pixels float32[m,3], stepped bool[m], shadowed bool[m])
    over every pixel whose camera hit lies on a diffuse material."""
    flat = ora.load_crtscene(scene)
    oacc = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD)
    frame, _ = oacc.render(W, H, 1, depth, 0)
    _, hits, P = camera_hits(oacc, W, H)
    hit = hits["mesh"] != MISS
    mat = flat.mesh_material[np.where(hit, hits["mesh"], 0)]
    sel = np.flatnonzero(hit & (flat.mat_kind[mat] == ora.MAT_DIFFUSE))
    P, mat = P[sel], mat[sel]
    smooth = flat.mat_smooth[mat] != 0
    ncos = np.where(smooth[:, None], hits["normal"][sel], _face_normals(flat, hits["tri"][sel]))
    albedo = flat.mat_albedo[mat]
    colour = np.zeros((sel.size, 3), np.float32)
    stepped = np.zeros(sel.size, bool)
    shadowed = np.zeros(sel.size, bool)
    for k in range(len(flat.light_intensity)):
        rays, radius, ld = shadow_queries(flat, P, k)
        answer, steps = occluded_ref(oacc, flat, rays, radius, 1e-4)
        assert not (answer == 2).any()
        area = np.float32(4.0) * PI_F * radius * radius
        d = dot3(ld, ncos)
        cosine = np.where(np.float32(0.0) < d, d, np.float32(0.0))              # std::max(0, dot)
        contrib = ((flat.light_intensity[k] / area) * cosine)[:, None] * albedo
        colour = np.where((answer == 0)[:, None], colour + contrib, colour)
        stepped |= steps > 0
        shadowed |= answer == 1
    assert colour.dtype == np.float32
    return colour, frame.reshape(-1, 3)[sel], stepped, shadowed


def test_model_reproduces_the_bits_of_the_oracles_diffuse_pixels(ora):
    """Pixels whose camera hit is diffuse are lit by the light loop of render.hpp:184-208 alone: summing, in light order and
    in float32, the lights the helper reports as not occluded must give the bits the oracle rendered -- the oracle whose
    hw11/scene8 frame is the reference's refractive_dragon.png byte for byte.  Every diffuse-hit pixel of both frames is
    compared.  hw11/scene8 (a glass dragon over a diffuse floor) supplies the queries that step through transmissive
    surfaces and has nothing opaque to cast a shadow; hw15/scene2 supplies the occluded lights."""
    n_stepped = n_shadowed = 0
    for scene, depth in ((SCENE8, 10), (SCENE2, 5)):
        colour, want, stepped, shadowed = diffuse_pixels_from_the_model(ora, scene, depth)
        print(f"{os.path.basename(scene)}: {len(colour)} diffuse-hit pixels, {stepped.sum()} with a stepped query, "
              f"{shadowed.sum()} with an occluded light")
        assert len(colour) >= 10000
        bad = np.flatnonzero((colour.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert bad.size == 0, (scene, bad.size, len(colour), colour[bad[:4]], want[bad[:4]])
        n_stepped += int(stepped.sum())
        n_shadowed += int(shadowed.sum())
    # not vacuous: among the compared pixels the loop was stepped through, and did occlude
    assert n_stepped >= 1000, n_stepped
    assert n_shadowed >= 1000, n_shadowed


def test_occluded_without_a_device_reports_no_device(rtk):
    if rtk.device_count() > 0:
        pytest.skip("a HIP device is present")
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    with pytest.raises(rtk.RtkError) as e:
        acc.occluded(np.zeros((4, 6), np.float32), np.ones(4, np.float32))
    assert e.value.code == rtk.RTK_ERR_NO_DEVICE


def test_empty_batch_returns_an_empty_array_and_touches_nothing(rtk):
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    out = acc.occluded(np.zeros((0, 6), np.float32), np.zeros(0, np.float32))
    assert out.dtype == np.uint8 and out.shape == (0,)
    out, n = acc.occluded(np.zeros((0, 6), np.float32), np.zeros(0, np.float32), count=True)
    assert out.shape == (0,) and n == 0
    acc.occluded_device(0, 0, 0, 0)


def test_bad_arguments_are_refused_before_any_device_is_needed(rtk):
    acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    rays, max_t = np.zeros((4, 6), np.float32), np.ones(4, np.float32)
    for mode in (rtk.TRACE_GROUP4, rtk.TRACE_STREAM, rtk.TRACE_TWOPASS, rtk.TRACE_REPACK, 99):
        with pytest.raises(rtk.RtkError) as e:
            acc.occluded(rays, max_t, trace_mode=mode)
        assert e.value.code == rtk.RTK_ERR_INVALID
    for bias in (float("nan"), float("inf")):
        with pytest.raises(rtk.RtkError) as e:
            acc.occluded(rays, max_t, shadow_bias=bias)
        assert e.value.code == rtk.RTK_ERR_INVALID
    with pytest.raises(rtk.RtkError) as e:
        acc.occluded_device(0, 0, 4, 0)
    assert e.value.code == rtk.RTK_ERR_INVALID and "null" in str(e.value)


def test_occlusion_constants_match_the_header(rtk):
    text = open(os.path.join(ROOT, "include", "rtk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    header = {name: int(value) for name, value in re.findall(r"\bRTK_OCC_([A-Z_]+)\s*=\s*(\d+)", text)}
    assert header == {"CLEAR": rtk.OCC_CLEAR, "OCCLUDED": rtk.OCC_OCCLUDED, "STEP_LIMIT": rtk.OCC_STEP_LIMIT}
    assert (rtk.OCC_CLEAR, rtk.OCC_OCCLUDED, rtk.OCC_STEP_LIMIT) == (0, 1, 2)
    steps = re.search(r"#define\s+RTK_OCCLUDED_MAX_STEPS\s+(\d+)", text)
    assert steps and int(steps.group(1)) == rtk.OCCLUDED_MAX_STEPS == 1024
