"""rtk_render_motion without a GPU: the numpy model of the contract (tests/motion_model.py) against the scalar C++ of
csrc/motion_math.hpp (tests/cpp/motion_math_check.cpp, built with the library's float flags, and as a stand-alone program under the
host sanitizers), bit for bit; what keeps the shared fixture honest; the two constants the GPU tests take from here, measured; and
the moving-mesh chain through tests/temporal_model.py."""
import os
import subprocess

import numpy as np
import pytest

import motion_model as mm
import plan_check
import temporal_model as tm
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "motion_math_check.cpp")
DEPS = [SRC] + plan_check.csrc("motion_math.hpp", "temporal_math.hpp")
FLOAT_FLAGS = ("-ffp-contract=off", "-fno-fast-math")
HONEST_SIZES = ((64, 64), (130, 70))


def _exe(build):
    if build == "sanitized":
        return plan_check.build("motion_math_check_san", SRC, DEPS, FLOAT_FLAGS, plan_check.SANITIZE)
    os.makedirs(plan_check.BUILD, exist_ok=True)
    exe = os.path.join(plan_check.BUILD, "motion_math_check")
    if plan_check.stale(exe, DEPS):
        # the float flags of the library's Makefile: no contraction, no fast-math
        subprocess.check_call(["g++", "-std=c++17", "-O3", *FLOAT_FLAGS, "-Wall", "-Wextra", "-Werror",
                               "-I" + os.path.join(plan_check.PKG, "csrc"), SRC, "-o", exe])
    return exe


def _run_check(exe, tmp_path, tri, bary, index, verts, view, outputs, fov=mm.FOV):
    h, w = tri.shape
    aspect, th, wf, hf = tm.scalars(w, h, fov)
    cam, mat = view if view is not None else (np.zeros(3, np.float32), np.zeros(9, np.float32))
    consts = np.concatenate([np.asarray(cam, np.float32).reshape(3), np.asarray(mat, np.float32).reshape(9),
                             np.array([th, aspect, wf, hf, 0, 0, 0, 0], np.float32)])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([w, h, index.shape[0], verts.shape[0], "prev_position" in outputs, "motion" in outputs, 0, 0], np.int32).tofile(f)
        consts.astype(np.float32).tofile(f)
        np.ascontiguousarray(tri, np.uint32).tofile(f)
        np.ascontiguousarray(bary, np.float32).tofile(f)
        np.ascontiguousarray(index, np.uint32).tofile(f)
        np.ascontiguousarray(verts, np.float32).tofile(f)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    plan_check.assert_sanitizers_quiet(res)
    got = np.fromfile(dst, np.float32)
    n = w * h
    assert got.size == n * (3 * ("prev_position" in outputs) + 2 * ("motion" in outputs))
    out = {}
    if "prev_position" in outputs:
        out["prev_position"] = got[:3 * n].reshape(h, w, 3)
    if "motion" in outputs:
        out["motion"] = got[-2 * n:].reshape(h, w, 2)
    return out


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("w,h", mm.SIZES)
def test_model_and_scalar_cpp_agree_in_every_bit(ora, tmp_path, w, h, build):
    """scene5's planes with the vertices of a moved pose and a previous camera that stood elsewhere; each output alone and both"""
    flat, _, index, view = mm.scene5(ora)
    base = mm.planes(ora, w, h)
    verts = mm.moved_vertices(flat)
    prev_view = (view[0] + np.array((0.5, -0.25, 1.0), np.float32), view[1])
    exe = _exe(build)
    want = mm.render_motion(base["tri"], base["bary"], index, verts, prev_view)
    assert want["computed"].sum() == base["hit"].sum()
    for outputs in mm.OUTPUTS:
        got = _run_check(exe, tmp_path, base["tri"], base["bary"], index, verts, prev_view, outputs)
        assert sorted(got) == sorted(outputs)
        mm.assert_same(got, want, outputs, (w, h, outputs))
    # without a view the positions are the same bits
    alone = mm.render_motion(base["tri"], base["bary"], index, verts, None)
    assert alone["motion"] is None and np.array_equal(mm.bits(alone["prev_position"]), mm.bits(want["prev_position"]))


def test_hostile_planes_on_the_model_and_the_scalar_cpp(ora, tmp_path):
    """ids at and beyond the triangle count, non-finite and huge barycentrics, a previous camera behind the surfaces: the
    sanitized program finishes and equals the model; a miss is zeros and the miss bits, a non-finite barycentric is not a miss"""
    flat, _, index, view = mm.scene5(ora)
    base = mm.planes(ora, 64, 64)
    verts = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    exe = _exe("sanitized")
    nt = index.shape[0]
    for name, tri, bary in mm.hostile_planes(base, nt):
        want = mm.render_motion(tri, bary, index, verts, view)
        got = _run_check(exe, tmp_path, tri, bary, index, verts, view, ("prev_position", "motion"))
        mm.assert_same(got, want, what=name)
        miss = tri >= nt
        assert (miss == ~want["hit"]).all()
        assert not mm.bits(want["prev_position"])[miss].any() and (mm.bits(want["motion"])[miss] == mm.MISS_BITS).all()
        if name != "barycentrics":
            for value in (nt, 0xFFFFFFFE, mm.MISS):
                assert (tri == value).sum() >= 100
            assert (want["hit"] & ~base["hit"]).sum() >= 100
        if name != "ids":
            assert not np.isfinite(want["prev_position"][want["hit"]]).all()
            assert np.isnan(bary).any() and np.isinf(bary).any() and (np.abs(np.nan_to_num(bary, posinf=0, neginf=0)) == np.float32(1e30)).any()
    # every surface behind the previous camera: all motion is the miss bits, the positions are as before
    behind = (view[0] + np.array((0.0, -60.0, -120.0), np.float32), view[1])
    want = mm.render_motion(base["tri"], base["bary"], index, verts, behind)
    assert not want["computed"].any() and (mm.bits(want["motion"]) == mm.MISS_BITS).all()
    mm.assert_same(_run_check(exe, tmp_path, base["tri"], base["bary"], index, verts, behind, ("prev_position", "motion")), want, what="behind")


@pytest.mark.parametrize("w,h", HONEST_SIZES)
def test_the_fixture_is_honest(ora, w, h):
    base = mm.planes(ora, w, h)
    share = float(base["hit"].mean())
    distinct = np.unique(base["tri"][base["hit"]]).size
    print(f"{w}x{h}: hit share {share:.3f}, {distinct} distinct triangles, meshes {np.unique(base['mesh'][base['hit']])}")
    assert share >= 0.1 and 1.0 - share >= 0.1
    assert distinct >= 50
    assert (base["tri"][~base["hit"]] == mm.MISS).all()


def test_reconstruction_error_and_own_motion_are_the_recorded_constants(ora):
    """With the scene's own vertices P' is the g-buffer's position up to rounding (that one is o + t * d, P' the barycentric sum),
    and with the scene's own camera the motion is zero up to rounding.  Both are measured here; motion_model.py records them."""
    flat, _, index, view = mm.scene5(ora)
    verts = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    err = move = 0.0
    for w, h in mm.SIZES:
        base = mm.planes(ora, w, h)
        got = mm.render_motion(base["tri"], base["bary"], index, verts, view)
        hit = base["hit"]
        assert hit.any() and got["computed"][hit].all()
        e = float(np.abs(got["prev_position"].astype(np.float64) - base["position"])[hit].max())
        m = float(np.abs(got["motion"].astype(np.float64))[hit].max())
        print(f"{w}x{h}: max |P' - position| = {e:.4g}, max |motion| = {m:.4g} px")
        err, move = max(err, e), max(move, m)
    print(f"recorded: {mm.RECONSTRUCTION_ERR:.4g} and {mm.MOTION_BOUND:.4g}")
    # the constants are the measurement, rounded up by less than a tenth
    assert err <= mm.RECONSTRUCTION_ERR <= 1.1 * err
    assert move <= mm.MOTION_BOUND <= 1.1 * move
    assert mm.POSITION_TOL == 4.0 * mm.RECONSTRUCTION_ERR


def test_a_rigid_translation_comes_back_as_position_minus_d(ora):
    flat, _, index, _ = mm.scene5(ora)
    d = np.array((0.25, -0.5, 0.125), np.float32)
    verts = (np.asarray(flat.vertices, np.float32).reshape(-1, 3) + d).astype(np.float32)
    base = mm.planes(ora, 130, 70)
    got = mm.render_motion(base["tri"], base["bary"], index, verts)
    hit = base["hit"]
    assert float(np.abs(got["prev_position"].astype(np.float64) - (base["position"].astype(np.float64) + d))[hit].max()) <= mm.POSITION_TOL
    assert not mm.bits(got["prev_position"])[~hit].any()


@pytest.mark.parametrize("w,h", HONEST_SIZES)
def test_a_moved_mesh_keeps_its_history_through_prev_position_only(ora, w, h):
    """Mesh MOVED_MESH translated by MOVE under the standing camera: temporal_model fed the new frame's own position throws the
    mesh's history away, fed prev_position it keeps it."""
    flat, oacc, index, view = mm.scene5(ora)
    old = np.asarray(flat.vertices, np.float32).reshape(-1, 3)
    new = mm.moved_vertices(flat)
    prev = mm.planes(ora, w, h)
    cur = mm.first_hits(mm.moved_oracle(ora, flat, new), w, h)
    assert (cur["tri"] != prev["tri"]).mean() > 0.02                          # the mesh did move on the screen
    back = mm.render_motion(cur["tri"], cur["bary"], index, old)
    params = dict(tm.PARAMS, fov_degrees=mm.FOV)
    shares = []
    for position in (back["prev_position"], cur["position"]):
        c, p = mm.temporal_inputs(cur, position, prev, view)
        res = tm.accumulate(c, p, noise=False, mesh=True, **params)
        shares.append(mm.kept_share(res["length"], cur))
    print(f"{w}x{h}: kept with prev_position {shares[0]:.3f}, with position {shares[1]:.3f}")
    assert shares[0] >= mm.SHARE_WITH
    assert shares[1] <= mm.SHARE_WITHOUT
    # the ground plane did not move: its pixels fare the same either way, up to those the mesh now covers or uncovers
    on = cur["hit"] & (cur["mesh"] != mm.MOVED_MESH)
    assert np.abs(back["prev_position"].astype(np.float64) - cur["position"])[on].max() <= mm.POSITION_TOL
