"""The textures and uvs of a live accel on the GPU: rtk_accel_set_textures, _set_texture_pixels[_device], _set_texture_frame_device
and _set_uvs[_device].  The comparison side is that of test_gpu_scene_state.py: the CPU oracle's frame of the flat scene with the
part replaced (texture_checks.py), every float by its bits, `rays` and `primary` as counts; for RTK_TRAVERSAL_FAST, which is not
the parity mode, a fresh product accel of the modified scene.  Every sequence asserts that the states whose pictures should differ
give different oracle frames, so a call that does nothing cannot pass."""
import dataclasses

import numpy as np
import pytest

from conftest import SCENE5
from scene_state_checks import DIFFUSE, TEXTURE, same, set_lights, set_materials, with_lights, with_material
from test_gpu_scene_state import MODES, SCENE4_TEX, _differ, _flat, _frames, _mode, _scene, _states
from texture_checks import ALBEDO, BITMAP, CHECKER, EDGES, Tex, check_table, dense_uvs, set_textures, textures_of, with_textures, with_uvs
from update_checks import _rtk_scene
from views_checks import cameras, with_camera

pytestmark = pytest.mark.gpu

SMALL = ((70, 45),)


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _quantise(ora, rgb):
    """write_ppm's bytes of a float frame [h, w, 3] (io/image/ppm.hpp:17-19), read back from the oracle's P3 text"""
    h, w, _ = rgb.shape
    return np.array(ora.write_ppm(rgb).split()[4:], dtype=np.uint8).reshape(h, w, 3)


# ---------------------------------------------------------------- 1. the table replaced, every engine

def _table_states(flat):
    """hw12/scene4: albedo, edges, checker, the dragon bitmap.  Colours and edge_width / square_size changed; then the kinds
    permuted: the bitmap's slot becomes a checker and the checker's the bitmap."""
    own = textures_of(flat)
    assert [t.kind for t in own] == [ALBEDO, EDGES, CHECKER, BITMAP]
    colours = [Tex(ALBEDO, (0.1, 0.8, 0.3)), Tex(EDGES, (0.9, 0.9, 0.1), (0.1, 0.2, 0.7), 0.11), Tex(CHECKER, (0.2, 0.9, 0.9), (0.6, 0.1, 0.4), 0.3),
               own[3]]
    permuted = [colours[1], colours[0], own[3], Tex(CHECKER, (1.0, 0.5, 0.0), (0.0, 0.25, 1.0), 0.0625)]
    return [("X own", flat), ("X colours", with_textures(flat, colours)), ("X permuted", with_textures(flat, permuted)), ("X own", flat)]


@pytest.mark.parametrize("mode", MODES)
def test_set_textures_every_engine(rtk, ora, mode):
    S = _states(ora)
    seq = _table_states(_flat(ora, SCENE4_TEX))
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    for i, (key, flat) in enumerate(seq):
        if i > 0:
            set_textures(acc, flat)
        _frames(rtk, acc, S, key, flat, mode, key, reps=2)
        check_table(acc, flat)
    _differ(S, seq)


# ---------------------------------------------------------------- 2. bitmaps of awkward sizes

def _awkward_states(flat):
    """A 1 x 1 bitmap, a 3 x 5 one behind it (dense byte offset 3), the dragon's texels, the scene's checker; then the 3 x 5 becomes
    a 7 x 2 and a 64 x 64, which outgrows whatever its slot had."""
    own = textures_of(flat)
    rng = np.random.default_rng(5)
    px = {s: rng.integers(0, 256, (s[1], s[0], 3), dtype=np.uint8) for s in ((1, 1), (3, 5), (7, 2), (64, 64))}
    out = []
    for size in ((3, 5), (7, 2), (64, 64)):
        texs = [Tex(BITMAP, pixels=px[(1, 1)]), Tex(BITMAP, pixels=px[size]), own[3], own[2]]
        out.append(("W %dx%d" % size, with_textures(flat, texs)))
    return out


def _to_awkward(acc, seq, upto=None):
    set_textures(acc, seq[0][1])
    for key, flat in seq[1:upto]:
        acc.set_texture_pixels(1, textures_of(flat)[1].pixels)


def test_bitmaps_of_awkward_sizes(rtk, ora):
    S = _states(ora)
    seq = _awkward_states(_flat(ora, SCENE4_TEX))
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    _frames(rtk, acc, S, "X own", _flat(ora, SCENE4_TEX), "auto", "resident", shapes=SMALL, reps=1)
    for i, (key, flat) in enumerate(seq):
        if i == 0:
            set_textures(acc, flat)
        else:
            acc.set_texture_pixels(1, textures_of(flat)[1].pixels)
        check_table(acc, flat)
        for mode in ("auto", "stream", "lane"):
            _frames(rtk, acc, S, key, flat, mode, key, reps=2)
    _differ(S, [("X own", _flat(ora, SCENE4_TEX))] + seq)


# ---------------------------------------------------------------- 3. from none to some and back

def _none_to_some(base):
    """hw09/scene5 has no textures and no uvs; material 1 is the dragon.  Planar uvs (x, z) scaled into [-0.5, 1.5], so that the
    out-of-range branches of sample_texture run."""
    assert base.tex_kind is None or len(base.tex_kind) == 0
    assert base.mat_kind.tolist() == [1, DIFFUSE] and base.mesh_material.tolist() == [0, 1]
    v = base.vertices.astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    uv = np.stack([(v[:, 0] - lo[0]) / (hi[0] - lo[0]), (v[:, 2] - lo[2]) / (hi[2] - lo[2])], axis=1) * 2.0 - 0.5
    with_uv = with_uvs(base, uv.astype(np.float32))
    texs = [Tex(CHECKER, (0.9, 0.1, 0.1), (0.1, 0.1, 0.9), 0.07), Tex(BITMAP, pixels=_noise(7, 4, 4))]
    with_tex = dataclasses.replace(with_textures(with_uv, texs), mat_texture=np.array([-1, -1], np.int32))
    return with_uv, with_tex, with_material(with_tex, 1, kind=TEXTURE, texture=0), with_material(with_tex, 1, kind=TEXTURE, texture=1)


def test_from_none_to_some_and_back(rtk, ora):
    S = _states(ora)
    base = _flat(ora, SCENE5)
    with_uv, with_tex, checker, bitmap = _none_to_some(base)
    modes = ("auto", "stream", "group4")

    def frames(acc, key, flat, what):
        for mode in modes:
            _frames(rtk, acc, S, key, flat, mode, what, shapes=SMALL, reps=2)

    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    frames(acc, "M own", base, "resident")
    acc.set_uvs(with_uv.uvs)                                          # stored: there is no texture to look it up in
    assert acc.uvs().tobytes() == with_uv.uvs.tobytes()
    frames(acc, "M own", base, "uvs")
    set_textures(acc, with_tex)                                       # the per-triangle uvs are made here
    check_table(acc, with_tex)
    frames(acc, "M own", base, "textures nobody uses")
    set_materials(acc, checker)
    frames(acc, "N checker", checker, "checker")
    set_materials(acc, bitmap)
    frames(acc, "N bitmap", bitmap, "bitmap")
    set_materials(acc, base)
    acc.set_textures([])
    assert len(acc.textures()["kind"]) == 0
    frames(acc, "M own", base, "back")
    set_textures(acc, with_tex)                                       # ... and from none to some a second time
    set_materials(acc, bitmap)
    frames(acc, "N bitmap", bitmap, "bitmap again")
    _differ(S, [("M own", base), ("N checker", checker), ("N bitmap", bitmap), ("M own", base)], 70, 45)
    # the uvs matter: with the zeros of a mesh without uvs the checker is one colour
    flat_checker = dataclasses.replace(checker, uvs=base.uvs, mesh_has_uvs=base.mesh_has_uvs)
    assert not same(S.frame("N checker zero uvs", flat_checker, 70, 45)[0], S.frame("N checker", checker, 70, 45)[0])
    # the same calls on an accel that has never rendered: host stores only, then one frame
    cold = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cold.set_uvs(with_uv.uvs)
    set_textures(cold, with_tex)
    set_materials(cold, bitmap)
    check_table(cold, with_tex)
    frames(cold, "N bitmap", bitmap, "never resident")


# ---------------------------------------------------------------- 4. uvs, from the host and from the device

def _uv_states(flat):
    uv = dense_uvs(flat)
    rotated = np.stack([1.0 - uv[:, 1], uv[:, 0]], axis=1).astype(np.float32)
    wild = np.random.default_rng(9).uniform(-2.0, 2.0, uv.shape).astype(np.float32)
    return [("U own", flat), ("U rotated", with_uvs(flat, rotated)), ("U random", with_uvs(flat, wild)), ("U own", flat)]


def test_set_uvs_host_and_device(rtk, ora):
    import torch
    S = _states(ora)
    seq = _uv_states(_flat(ora, SCENE4_TEX))
    host = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    dev = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))               # not resident yet: the first device call puts it there
    side = torch.cuda.Stream()
    w, h = SMALL[0]
    for key, flat in seq[1:]:
        uv = dense_uvs(flat)
        host.set_uvs(uv)
        assert host.uvs().tobytes() == uv.tobytes()
        for mode in ("auto", "stream", "lane"):
            _frames(rtk, host, S, key, flat, mode, ("host", key), reps=2)
        d_uv = torch.from_numpy(uv).cuda()
        torch.cuda.current_stream().synchronize()
        dev.set_uvs_device(d_uv.data_ptr(), side.cuda_stream)
        # a frame on ANOTHER stream right after the call sees the new uvs
        ref, ocn = S.frame(key, flat, w, h)
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        acc_stream = torch.cuda.current_stream().cuda_stream
        dev.render_frame_device(rtk.RenderConfig(width=w, height=h), out.data_ptr(), acc_stream)
        cn = dev.last_counters()
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), ref) and cn["rays"] == ocn["rays"], key
        assert dev.uvs().tobytes() == uv.tobytes(), key
        for mode in ("stream", "group4"):
            _frames(rtk, dev, S, key, flat, mode, ("device", key), shapes=SMALL, reps=2)
    _differ(S, seq)


# ---------------------------------------------------------------- 5. the state survives the updates

def _three_quarters(flat):
    """3/4 of each mesh's triangles (hw12/scene4: one of two), as update_geometry takes them"""
    ntris = (flat.mesh_ntris * 3 // 4).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(flat.mesh_ntris)[:-1]])
    idx = np.concatenate([flat.indices[f:f + n] for f, n in zip(first, ntris)]).astype(np.uint32)
    return np.ascontiguousarray(idx), ntris


def test_textures_and_uvs_survive_updates(rtk, ora):
    import torch
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    uv = np.random.default_rng(9).uniform(-0.3, 1.3, dense_uvs(base).shape).astype(np.float32)
    texs = textures_of(base)
    texs[3] = Tex(BITMAP, pixels=_noise(21, 9, 13))
    idx, ntris = _three_quarters(base)
    assert ntris.tolist() == [1, 1, 1, 1]
    moved = (base.vertices + 0.15 * np.sin(np.arange(base.vertices.size, dtype=np.float32)).reshape(-1, 3)).astype(np.float32)
    lights = (base.light_pos + np.array([1.5, 0.5, -1.0], np.float32), base.light_intensity * np.float32(0.5))
    s1 = with_textures(with_uvs(base, uv), texs)
    s2 = dataclasses.replace(s1, indices=idx, mesh_ntris=ntris)
    s3 = dataclasses.replace(s2, vertices=moved)
    s4 = with_lights(s3, *lights)
    seq = [("V own", base), ("V uvs texels", s1), ("V geometry", s2), ("V vertices", s3), ("V lights", s4)]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    modes = ("auto", "stream")

    def frames(a, key, flat, what):
        for mode in modes:
            _frames(rtk, a, S, key, flat, mode, what, reps=2)

    frames(acc, *seq[0], "built")
    acc.set_uvs(uv)
    acc.set_texture_pixels(3, texs[3].pixels)
    frames(acc, *seq[1], "set")
    acc.update_geometry(base.vertices, idx, ntris)                    # regathers the per-triangle uvs from the CURRENT uvs
    frames(acc, *seq[2], "update_geometry")
    acc.update_vertices(moved)
    frames(acc, *seq[3], "update_vertices")
    set_lights(acc, s4)
    frames(acc, *seq[4], "set_lights")
    check_table(acc, s4)
    assert acc.uvs().tobytes() == uv.tobytes()
    _differ(S, seq)
    # the other order: update_geometry first, so that the vertex ids exist on the device only, then the uvs from the device
    other = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    other.update_geometry(base.vertices, idx, ntris)
    d_uv = torch.from_numpy(uv).cuda()
    torch.cuda.synchronize()
    other.set_uvs_device(d_uv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    other.set_texture_pixels(3, texs[3].pixels)
    frames(other, *seq[2], "update_geometry, then uvs")
    other.update_vertices(moved)
    frames(other, *seq[3], "... then update_vertices")
    assert other.uvs().tobytes() == uv.tobytes()


# ---------------------------------------------------------------- 6. texels from the device, and render to texture

def test_set_texture_pixels_device(rtk, ora):
    import torch
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    host, dev = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX)), rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    side = torch.cuda.Stream()
    seq = [("X own", base)]
    for step, (w, h) in enumerate(((33, 17), (33, 17), (600, 400), (2, 3))):      # a smaller one, the same size again, one that outgrows the slot
        px = _noise(30 + step, h, w)
        texs = textures_of(base)
        texs[3] = Tex(BITMAP, pixels=px)
        flat = with_textures(base, texs)
        key = "D %d" % step
        seq.append((key, flat))
        host.set_texture_pixels(3, px)
        d_px = torch.from_numpy(px).cuda()
        torch.cuda.synchronize()
        dev.set_texture_pixels_device(3, w, h, d_px.data_ptr(), side.cuda_stream)
        for acc in (host, dev):
            for mode in ("auto", "stream"):
                _frames(rtk, acc, S, key, flat, mode, (key, acc is dev), shapes=SMALL, reps=2)
            check_table(acc, flat)
    _differ(S, seq, *SMALL[0])


def _float_frame(seed, h, w):
    """random in [-0.5, 1.5]; then, as far as there is room: a NaN, -0.0, exactly 0 and 1, and the floats either side of k / 255.999"""
    f = np.random.default_rng(seed).uniform(-0.5, 1.5, h * w * 3).astype(np.float32)
    special = [np.nan, -0.0, 0.0, 1.0]
    for k in (1, 2, 127, 128, 254, 255):
        x = np.float32(k / 255.999)
        special += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(2))]
    n = min(len(special), f.size)
    f[:n] = np.array(special[:n], np.float32)
    return f.reshape(h, w, 3)


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (7, 2), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_set_texture_frame_device(rtk, ora, size):
    """The texture sits behind a 1 x 1 bitmap (3 bytes), so that on the first call, into the dense upload of the scene, its bytes
    begin at an address that is no multiple of four."""
    import torch
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    w, h = size
    own = textures_of(base)
    start = with_textures(base, [Tex(BITMAP, pixels=_noise(1, 1, 1)), own[1], own[2], Tex(BITMAP, pixels=_noise(2, 48, 64))])
    acc = rtk.KdTreeSimdAccel(_rtk_scene(rtk, start))
    frame = _float_frame(40 + w, h, w)
    want = _quantise(ora, frame)
    d_frame = torch.from_numpy(frame).cuda()
    d_rgb8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rtk.frame_to_rgb8_device(d_frame.data_ptr(), frame.size, d_rgb8.data_ptr(), stream)
    for rep in range(2):                                              # the second time the accel is resident and the size is the slot's
        acc.set_texture_frame_device(3, w, h, d_frame.data_ptr(), stream)
        got = acc.texture_pixels(3)
        assert got.tobytes() == d_rgb8.cpu().numpy().tobytes() == want.tobytes(), (size, rep)
    texs = textures_of(start)
    texs[3] = Tex(BITMAP, pixels=want)
    flat = with_textures(base, texs)
    check_table(acc, flat)
    for mode in ("auto", "stream"):
        _frames(rtk, acc, S, "F %dx%d" % size, flat, mode, size, shapes=SMALL, reps=1)
    assert not same(S.frame("F %dx%d" % size, flat, *SMALL[0])[0], S.frame("F start", start, *SMALL[0])[0])


def test_a_view_on_a_quad_without_leaving_the_device(rtk, ora):
    import torch
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    w, h = 64, 48
    cam = cameras(base)["B"]
    cfg = rtk.RenderConfig(width=w, height=h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    d_view = torch.from_numpy(np.ascontiguousarray(cam[None, :], np.float32)).cuda()
    d_out = torch.full((1, h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    acc.render_views_device(cfg, d_view.data_ptr(), 1, d_out.data_ptr(), stream)
    acc.set_texture_frame_device(3, w, h, d_out.data_ptr(), stream)
    # the same steps on the host: the oracle's frame under that camera, write_ppm's bytes, the scene with those as the bitmap
    view, _ = S.frame(("X own", "B"), with_camera(base, cam), w, h)
    texs = textures_of(base)
    texs[3] = Tex(BITMAP, pixels=_quantise(ora, view))
    flat = with_textures(base, texs)
    for mode in ("auto", "stream"):
        _frames(rtk, acc, S, "Q screen", flat, mode, "screen", reps=2)
    check_table(acc, flat)
    _differ(S, [("X own", base), ("Q screen", flat)])


# ---------------------------------------------------------------- 7. views, regions, radiance and RTK_TRAVERSAL_FAST

def test_views_regions_and_radiance_follow(rtk, ora):
    S = _states(ora)
    seq = _awkward_states(_flat(ora, SCENE4_TEX))
    key, flat = seq[-1]
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    acc.render_frame(rtk.RenderConfig(width=70, height=45))
    _to_awkward(acc, seq)
    w, h = 96, 54
    ref, ocn = S.frame(key, flat, w, h)
    cams = cameras(flat)
    for mode in ("auto", "stream"):
        cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_mode(rtk, mode))
        rgb, cn = acc.render_views(cfg, np.stack([cams["A"], cams["B"]]))
        rb, ob = S.frame((key, "B"), with_camera(flat, cams["B"]), w, h)
        assert same(rgb[0], ref) and same(rgb[1], rb) and cn["rays"] == ocn["rays"] + ob["rays"], mode
        rects = np.array([[3, 2, 50, 31], [50, 20, 96, 54]], np.int32)
        out, _ = acc.render_regions(cfg, rects)
        for x0, y0, x1, y1 in rects.tolist():
            assert same(out[y0:y1, x0:x1], ref[y0:y1, x0:x1]), (mode, x0, y0)
    rays = acc.camera_rays(rtk.RenderConfig(width=w, height=h)).reshape(-1, 6)
    rgb, cn = acc.radiance(rays)
    assert same(rgb.reshape(h, w, 3), ref) and cn["rays"] == ocn["rays"]
    assert not same(ref, S.frame("X own", _flat(ora, SCENE4_TEX), w, h)[0])


def test_fast_accel_follows(rtk, ora, monkeypatch):
    """RTK_TRAVERSAL_FAST is not the parity mode: the live accel against a fresh FAST accel of the modified scene."""
    base = _flat(ora, SCENE4_TEX)
    seq = _awkward_states(base)
    uv = dense_uvs(_uv_states(base)[2][1])
    final = with_uvs(seq[-1][1], uv)
    monkeypatch.setenv("RTK_TRAVERSAL_FAST", "1")
    live = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    fresh = rtk.KdTreeSimdAccel(_rtk_scene(rtk, final))
    start = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    monkeypatch.delenv("RTK_TRAVERSAL_FAST")
    w, h = 96, 54
    cfgs = [rtk.RenderConfig(width=w, height=h, trace_mode=_mode(rtk, m)) for m in ("auto", "stream", "group4")]
    live.render_frame(cfgs[0])
    _to_awkward(live, seq)
    live.set_uvs(uv)
    for cfg in cfgs:
        (a, ca), (b, cb) = live.render_frame(cfg), fresh.render_frame(cfg)
        assert same(a, b) and ca["rays"] == cb["rays"], cfg.trace_mode
        assert not same(a, start.render_frame(cfg)[0])
    cams = cameras(base)
    views = np.stack([cams["A"], cams["B"]])
    (a, ca), (b, cb) = live.render_views(cfgs[0], views), fresh.render_views(cfgs[0], views)
    assert same(a, b) and ca["rays"] == cb["rays"]
    rays = live.camera_rays(cfgs[0]).reshape(-1, 6)
    (a, ca), (b, cb) = live.radiance(rays), fresh.radiance(rays)
    assert same(a, b) and ca["rays"] == cb["rays"]


# ---------------------------------------------------------------- 8. refusals on a resident accel

def test_refused_calls_on_a_resident_accel(rtk, ora):
    import ctypes
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    _frames(rtk, acc, S, "X own", base, "auto", "before", shapes=SMALL, reps=2)
    L, INV = rtk.lib(), rtk.RTK_ERR_INVALID
    tab = np.zeros(4, rtk.TEXTURE_DTYPE)
    n = ctypes.c_int32(0)
    assert L.rtk_accel_get_textures(acc._h, tab.ctypes.data, 4, ctypes.byref(n)) == rtk.RTK_OK
    px = np.ascontiguousarray(acc.texture_pixels(3))
    f32 = np.zeros(64, np.float32)
    ptrs = (ctypes.c_void_p * 4)(None, None, None, px.ctypes.data)
    bad_kind, bad_size, huge = tab.copy(), tab.copy(), tab.copy()
    bad_kind["kind"][1] = 7
    bad_size["width"][3] = 0
    huge["width"][3], huge["height"][3] = 16385, 16384
    calls = [
        lambda: L.rtk_accel_set_textures(acc._h, tab.ctypes.data, -1, ptrs),
        lambda: L.rtk_accel_set_textures(acc._h, None, 4, ptrs),
        lambda: L.rtk_accel_set_textures(acc._h, tab.ctypes.data, 4, None),
        lambda: L.rtk_accel_set_textures(acc._h, tab.ctypes.data, 4, (ctypes.c_void_p * 4)()),
        lambda: L.rtk_accel_set_textures(acc._h, bad_kind.ctypes.data, 4, ptrs),
        lambda: L.rtk_accel_set_textures(acc._h, bad_size.ctypes.data, 4, ptrs),
        lambda: L.rtk_accel_set_textures(acc._h, huge.ctypes.data, 4, ptrs),
        lambda: L.rtk_accel_set_textures(acc._h, tab.ctypes.data, 3, ptrs),           # material 3 uses texture 3
        lambda: L.rtk_accel_set_textures(acc._h, None, 0, None),
        lambda: L.rtk_accel_set_texture_pixels(acc._h, 4, 2, 2, px.ctypes.data),
        lambda: L.rtk_accel_set_texture_pixels(acc._h, -1, 2, 2, px.ctypes.data),
        lambda: L.rtk_accel_set_texture_pixels(acc._h, 3, 0, 2, px.ctypes.data),
        lambda: L.rtk_accel_set_texture_pixels(acc._h, 3, 2, 2, None),
        lambda: L.rtk_accel_set_texture_pixels(acc._h, 2, 2, 2, px.ctypes.data),      # a checker
        lambda: L.rtk_accel_set_texture_pixels_device(acc._h, 2, 2, 2, px.ctypes.data, None),
        lambda: L.rtk_accel_set_texture_pixels_device(acc._h, 3, 2, -2, px.ctypes.data, None),
        lambda: L.rtk_accel_set_texture_pixels_device(acc._h, 3, 2, 2, None, None),
        lambda: L.rtk_accel_set_texture_frame_device(acc._h, 0, 2, 2, f32.ctypes.data, None),
        lambda: L.rtk_accel_set_texture_frame_device(acc._h, 3, 16385, 16384, f32.ctypes.data, None),
        lambda: L.rtk_accel_set_texture_frame_device(acc._h, 3, 2, 2, None, None),
        lambda: L.rtk_accel_set_uvs(acc._h, None),
        lambda: L.rtk_accel_set_uvs_device(acc._h, None, None),
    ]
    for i, call in enumerate(calls):
        assert call() == INV, i
        for mode in ("auto", "stream"):
            _frames(rtk, acc, S, "X own", base, mode, ("refused", i), shapes=SMALL, reps=1)
    check_table(acc, base)
    assert acc.uvs().tobytes() == dense_uvs(base).tobytes()
    key, flat = _table_states(base)[1]
    set_textures(acc, flat)                                           # ... and it stays usable
    _frames(rtk, acc, S, key, flat, "auto", "after", shapes=SMALL, reps=2)


# ---------------------------------------------------------------- 9. the launch order is kept

def test_same_size_texels_under_the_learnt_order(rtk, ora):
    """Three group4 frames teach the accel a launch order; a same-size replacement keeps it (rtk.h), and the frames under it have
    the new texels.  (The order cannot be seen from outside: this tests the result.)"""
    S = _states(ora)
    base = _flat(ora, SCENE4_TEX)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE4_TEX))
    _frames(rtk, acc, S, "X own", base, "group4", "learning", shapes=((200, 120),), reps=3)
    own = textures_of(base)
    px = _noise(77, *own[3].pixels.shape[:2])
    flat = with_textures(base, own[:3] + [Tex(BITMAP, pixels=px)])
    acc.set_texture_pixels(3, px)
    _frames(rtk, acc, S, "O noise", flat, "group4", "same size", shapes=((200, 120),), reps=2)
    check_table(acc, flat)
    _differ(S, [("X own", base), ("O noise", flat)])
