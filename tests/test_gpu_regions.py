"""rtk_render_regions[_device] on the GPU against the CPU oracle: every pixel inside a rectangle is, by its bits, the pixel of the
oracle's frame (views_checks.Oracle, camera "A" = the scene's own); `rays` and `primary` are compared as counts.  Frames are
200x120 and 70x45 (ragged blocks and a ragged bucket); rectangles are ragged against their own 8x8 blocks as well."""
import numpy as np
import pytest

from conftest import SCENE5, SCENE8
from regions_checks import SENTINEL, area, around, check_in_frame, check_packed, crop, grid_rects, inside_mask
from views_checks import Oracle, bits, same, with_camera

pytestmark = pytest.mark.gpu

_ORACLES = {}
_SCENES = {}
SHAPES = {(200, 120): (13, 7, 77, 50), (70, 45): (13, 7, 61, 38)}       # frame -> the rectangle R of the partition


def _oracle(ora, path):
    if path not in _ORACLES:
        _ORACLES[path] = Oracle(ora, path)
    return _ORACLES[path]


def _scene(rtk, path):
    if path not in _SCENES:
        _SCENES[path] = rtk.parse_scene_file(path)
    return _SCENES[path]


def _modes(rtk):
    return {"auto": rtk.TRACE_AUTO, "group4": rtk.TRACE_GROUP4, "group8": rtk.TRACE_GROUP8, "group16": rtk.TRACE_GROUP16,
            "stream": rtk.TRACE_STREAM}


def _sentinel_frame(w, h):
    return np.full((h, w, 3), SENTINEL, np.float32)


# ---------------------------------------------------------------- 1. a partition of the frame

@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", ["auto", "group4", "group8", "group16", "stream"])
def test_partition_adds_up_to_the_frame(rtk, ora, mode, shape):
    w, h = shape
    R = SHAPES[shape]
    o = _oracle(ora, SCENE5)
    ref, ocn = o.frame("A", w, h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    five = [R] + around(w, h, R)
    assert area(five) == w * h
    views, cn = acc.render_regions(cfg, five, rtk.REGIONS_PACKED)
    check_packed(views, five, ref, (mode, shape, "five"))
    assert (cn["rays"], cn["primary"]) == (ocn["rays"], w * h), (mode, shape)
    # R alone and the other four: the two calls' rays add up to the frame's
    v1, c1 = acc.render_regions(cfg, [R], rtk.REGIONS_PACKED)
    v4, c4 = acc.render_regions(cfg, five[1:], rtk.REGIONS_PACKED)
    check_packed(v1, [R], ref, (mode, shape, "R"))
    check_packed(v4, five[1:], ref, (mode, shape, "four"))
    assert c1["rays"] + c4["rays"] == ocn["rays"], (mode, shape, c1["rays"], c4["rays"])
    assert c1["primary"] == area([R]) and c4["primary"] == w * h - area([R])
    # R's rays are those of the radiance batch over R's camera rays with the frame's pixel indices (a parity pinned elsewhere)
    x0, y0, x1, y1 = R
    rays = np.ascontiguousarray(crop(acc.camera_rays(cfg), R)).reshape(-1, 6)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    rgb, rc = acc.radiance(rays, (ys * w + xs).reshape(-1).astype(np.uint32))
    assert same(rgb.reshape(y1 - y0, x1 - x0, 3), crop(ref, R))
    assert rc["rays"] == c1["rays"], (mode, shape)


# ---------------------------------------------------------------- 2. IN_FRAME leaves the rest alone

@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", ["auto", "group8", "stream"])
def test_in_frame_leaves_every_other_float_alone(rtk, ora, mode, shape):
    import torch
    w, h = shape
    o = _oracle(ora, SCENE5)
    ref, _ = o.frame("A", w, h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    # one pixel in the far corner, a one-pixel row across the width, an aligned block, a one-pixel column
    rects = [(w - 1, h - 1, w, h), (0, 41, w, 42), (8, 8, 16, 16), (5, 3, 6, 40)]
    frame, cn = acc.render_regions(cfg, rects, rtk.REGIONS_IN_FRAME, _sentinel_frame(w, h))
    check_in_frame(frame, rects, ref, (mode, shape, "host"))
    assert cn["primary"] == area(rects) == 1 + w + 64 + 37
    n, guard = w * h * 3, 256
    buf = torch.full((n + guard,), float(SENTINEL), dtype=torch.float32, device="cuda")
    acc.render_regions_device(cfg, rects, rtk.REGIONS_IN_FRAME, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    c2 = acc.last_counters()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    check_in_frame(got[:n].reshape(h, w, 3), rects, ref, (mode, shape, "device"))
    assert np.array_equal(bits(got[n:]), bits(np.full(guard, SENTINEL, np.float32)))
    assert c2 == cn


# ---------------------------------------------------------------- 3. the whole frame as one rectangle, and the cost feedback

@pytest.mark.parametrize("mode", ["auto", "group4"])
def test_whole_frame_rectangle_and_the_order_tables(rtk, ora, monkeypatch, mode):
    w, h = 200, 120
    o = _oracle(ora, SCENE5)
    ref, ocn = o.frame("A", w, h)
    monkeypatch.setenv("RTK_COST_RESORT_EVERY", "1")               # every call re-sorts: the measured order and the packed workgroups are in play
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    monkeypatch.delenv("RTK_COST_RESORT_EVERY")
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    rgb, fcn = acc.render_frame(cfg)
    assert same(rgb, ref) and fcn["rays"] == ocn["rays"]
    whole = [(0, 0, w, h)]
    for rep in range(3):
        for layout in (rtk.REGIONS_PACKED,):
            views, cn = acc.render_regions(cfg, whole, layout)
            assert same(views[0], rgb), (mode, rep)
            assert (cn["rays"], cn["primary"]) == (fcn["rays"], fcn["primary"]), (mode, rep)
    # another list on the same accel must not run under the old one's order (it has other units altogether)
    R = SHAPES[(w, h)]
    other = around(w, h, R) + [R]
    for rep in range(2):
        views, cn = acc.render_regions(cfg, other, rtk.REGIONS_PACKED)
        check_packed(views, other, ref, (mode, "other list", rep))
        assert cn["rays"] == ocn["rays"]
    frame, cn = acc.render_regions(cfg, whole, rtk.REGIONS_IN_FRAME, _sentinel_frame(w, h))
    assert same(frame, rgb) and cn["rays"] == ocn["rays"]
    # the plain frame's own feedback is intact
    for rep in range(2):
        again, c2 = acc.render_frame(cfg)
        assert same(again, ref) and c2 == fcn, (mode, rep)


# ---------------------------------------------------------------- 4. many rectangles, and the cut into launches

@pytest.mark.parametrize("limit", [None, 150], ids=["one_launch", "launches_of_150"])
@pytest.mark.parametrize("mode", ["group4", "stream"])
def test_three_hundred_rectangles(rtk, ora, monkeypatch, mode, limit):
    w, h = 320, 240                                                # 20 x 15 cells of 16 pixels
    o = _oracle(ora, SCENE5)
    ref, _ = o.frame("A", w, h)
    rects = grid_rects(w, h, seed=11)
    assert len(rects) == 300 and sum(1 for r in rects if area([r]) == 0) >= 5 and sum(1 for r in rects if r[2] - r[0] == 1) >= 20
    blocks = sum(((r[2] - r[0] + 7) // 8) * ((r[3] - r[1] + 7) // 8) for r in rects)
    assert blocks > 4 * 150                                        # the limit of 150 units cuts this list into several launches
    if limit is not None:
        monkeypatch.setenv("RTK_VIEWS_LAUNCH_UNITS", str(limit))
    monkeypatch.setenv("RTK_COST_RESORT_EVERY", "1")
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    monkeypatch.delenv("RTK_COST_RESORT_EVERY")
    if limit is not None:
        monkeypatch.delenv("RTK_VIEWS_LAUNCH_UNITS")
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    counts = []
    for rep in range(3 if mode == "group4" else 1):               # the natural order, then the measured one, twice
        views, cn = acc.render_regions(cfg, rects, rtk.REGIONS_PACKED)
        check_packed(views, rects, ref, (mode, limit, "packed", rep))
        assert cn["primary"] == area(rects)
        counts.append(cn["rays"])
    frame, cn = acc.render_regions(cfg, rects, rtk.REGIONS_IN_FRAME, _sentinel_frame(w, h))
    check_in_frame(frame, rects, ref, (mode, limit, "in frame"))
    assert cn["primary"] == area(rects)
    counts.append(cn["rays"])
    assert len(set(counts)) == 1 and counts[0] > area(rects)


# ---------------------------------------------------------------- 5. forking ray trees

@pytest.mark.parametrize("mode", ["auto", "group4", "stream"])
def test_refractive_scene(rtk, ora, mode):
    w, h, depth = 96, 54, 5
    o = _oracle(ora, SCENE8)
    ref, ocn = o.frame("A", w, h, 1, depth)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE8))
    cfg = rtk.RenderConfig(width=w, height=h, max_ray_depth=depth, trace_mode=_modes(rtk)[mode])
    R = (13, 7, 61, 38)
    five = [R] + around(w, h, R)
    for rep in range(2):
        views, cn = acc.render_regions(cfg, five, rtk.REGIONS_PACKED)
        check_packed(views, five, ref, (mode, rep))
        assert (cn["rays"], cn["primary"]) == (ocn["rays"], w * h), (mode, rep)
    rects = [R, (70, 3, 71, 50), (0, 40, 13, 54)]
    frame, cn = acc.render_regions(cfg, rects, rtk.REGIONS_IN_FRAME, _sentinel_frame(w, h))
    check_in_frame(frame, rects, ref, (mode, "in frame"))


@pytest.mark.parametrize("mode", ["auto", "group8"])
def test_diffuse_gi(rtk, ora, mode):
    w, h, spp, gi = 48, 27, 2, 2
    o = _oracle(ora, SCENE5)
    ref, ocn = o.frame("A", w, h, spp, 5, gi)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, spp=spp, diffuse_rays=gi, trace_mode=_modes(rtk)[mode])
    R = (5, 3, 30, 20)
    five = [R] + around(w, h, R)
    views, cn = acc.render_regions(cfg, five, rtk.REGIONS_PACKED)
    check_packed(views, five, ref, (mode, "packed"))
    assert (cn["rays"], cn["primary"]) == (ocn["rays"], w * h * spp), mode
    frame, cn = acc.render_regions(cfg, [R, (31, 0, 48, 27)], rtk.REGIONS_IN_FRAME, _sentinel_frame(w, h))
    check_in_frame(frame, [R, (31, 0, 48, 27)], ref, (mode, "in frame"))


# ---------------------------------------------------------------- 6. progressive passes

@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_progressive_passes(rtk, ora, mode):
    w, h, spp = 70, 45, 4
    o = _oracle(ora, SCENE5)
    ref, _ = o.frame("A", w, h, spp)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    tm = _modes(rtk)[mode]
    rects = [(13, 7, 61, 38), (0, 0, 9, 7), (62, 40, 70, 45)]
    whole = rtk.RenderConfig(width=w, height=h, spp=spp, trace_mode=tm)
    passes = [rtk.RenderConfig(width=w, height=h, spp=spp, trace_mode=tm, sample_begin=b, sample_count=2) for b in (0, 2)]
    one, c1 = acc.render_regions(whole, rects, rtk.REGIONS_PACKED)
    check_packed(one, rects, ref, (mode, "one call"))
    assert c1["primary"] == area(rects) * spp
    buf, rays = None, 0
    for p in passes:
        views, cn = acc.render_regions(p, rects, rtk.REGIONS_PACKED, buf)
        buf = views[0].base if views[0].base is not None else buf
        assert cn["primary"] == area(rects) * 2
        rays += cn["rays"]
    check_packed(views, rects, ref, (mode, "two passes, packed"))
    assert rays == c1["rays"]
    frame, rays = _sentinel_frame(w, h), 0
    for i, p in enumerate(passes):
        frame, cn = acc.render_regions(p, rects, rtk.REGIONS_IN_FRAME, frame)
        rays += cn["rays"]
        m = inside_mask(w, h, rects)
        assert (bits(frame)[~m] == bits(SENTINEL)).all(), (mode, "outside after pass", i)
        if i == 0:
            assert (bits(frame)[m] != bits(ref)[m]).any()          # sums of two samples, not colours yet
    check_in_frame(frame, rects, ref, (mode, "two passes, in frame"))
    assert rays == c1["rays"]


# ---------------------------------------------------------------- 7. with the live-scene calls

def test_after_camera_lights_and_vertices(rtk, ora):
    from test_gpu_update import _twist
    o = _oracle(ora, SCENE5)
    w, h = 96, 54
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h)
    rects = [(13, 7, 61, 38), (70, 3, 71, 50)]
    before, _ = acc.render_regions(cfg, rects, rtk.REGIONS_PACKED)
    cam = o.cams["B"]
    acc.set_camera(cam[:3], cam[3:])
    pos, inten = acc.lights()
    pos, inten = pos[::-1][:max(1, len(inten) - 1)] + np.float32(0.25), inten[:max(1, len(inten) - 1)] * np.float32(1.5)
    acc.set_lights(pos, inten)
    verts = _twist(o.flat, 0.5)
    acc.update_vertices(verts)
    frame, fcn = acc.render_frame(cfg)
    import dataclasses
    flat = dataclasses.replace(with_camera(o.flat, cam, verts), light_pos=np.ascontiguousarray(pos, np.float32),
                               light_intensity=np.ascontiguousarray(inten, np.float32))
    ref, ocn = ora.Accel(ora.Scene(flat), ora.ACCEL_KD_SIMD).render(w, h, 1, 5, 0)
    assert same(frame, ref) and fcn["rays"] == ocn["rays"]          # the accel's own frame is the oracle's of the changed scene
    for rep in range(2):
        views, _ = acc.render_regions(cfg, rects, rtk.REGIONS_PACKED)
        check_packed(views, rects, frame, ("live", rep))
    assert not same(views[0], before[0])
    five = [rects[0]] + around(w, h, rects[0])
    _, cn = acc.render_regions(cfg, five, rtk.REGIONS_PACKED)
    assert cn["rays"] == fcn["rays"]


def test_fast_traversal_accel_equals_its_own_frame(rtk, ora):
    w, h = 96, 54
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5), traversal=rtk.TRAVERSAL_FAST)
    cfg = rtk.RenderConfig(width=w, height=h)
    frame, fcn = acc.render_frame(cfg)
    R = (13, 7, 61, 38)
    five = [R] + around(w, h, R)
    views, cn = acc.render_regions(cfg, five, rtk.REGIONS_PACKED)
    check_packed(views, five, frame, "fast, packed")
    assert (cn["rays"], cn["primary"]) == (fcn["rays"], w * h)
    aligned = [(8, 8, 48, 40), (64, 0, 96, 54)]
    got, _ = acc.render_regions(cfg, aligned, rtk.REGIONS_IN_FRAME, _sentinel_frame(w, h))
    check_in_frame(got, aligned, frame, "fast, in frame")


# ---------------------------------------------------------------- 8. the device variant is stream-ordered

@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_device_variant_on_a_side_stream(rtk, ora, mode):
    import torch
    w, h = 70, 45
    o = _oracle(ora, SCENE5)
    ref, ocn = o.frame("A", w, h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    R = SHAPES[(w, h)]
    five = [R] + around(w, h, R)
    n, guard = w * h * 3, 64
    side = torch.cuda.Stream()
    for rep in range(3):
        # the buffer is filled on the current stream; the call on the side stream is ordered behind the fill by the wait alone
        buf = torch.full((n + guard,), float("nan"), dtype=torch.float32, device="cuda")
        buf[n:] = float(SENTINEL)
        side.wait_stream(torch.cuda.current_stream())
        acc.render_regions_device(cfg, five, rtk.REGIONS_PACKED, buf.data_ptr(), side.cuda_stream)
        cn = acc.last_counters()                                   # (synchronises the stream the call ran on)
        side.synchronize()
        got = buf.cpu().numpy()
        assert not np.isnan(got[:n]).any() and (got[n:] == SENTINEL).all(), (mode, rep)
        at = 0
        for r in five:
            k = area([r]) * 3
            assert same(got[at:at + k].reshape(r[3] - r[1], r[2] - r[0], 3), crop(ref, r)), (mode, rep, r)
            at += k
        assert (cn["rays"], cn["primary"]) == (ocn["rays"], w * h), (mode, rep)


# ---------------------------------------------------------------- 9. PACKED overlaps

@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_packed_overlaps_get_a_copy_each(rtk, ora, mode):
    w, h = 70, 45
    o = _oracle(ora, SCENE5)
    ref, _ = o.frame("A", w, h)
    acc = rtk.KdTreeSimdAccel(_scene(rtk, SCENE5))
    cfg = rtk.RenderConfig(width=w, height=h, trace_mode=_modes(rtk)[mode])
    rects = [(10, 5, 50, 30), (30, 20, 70, 45), (10, 5, 50, 30), (35, 22, 36, 23), (0, 0, w, h)]
    views, cn = acc.render_regions(cfg, rects, rtk.REGIONS_PACKED)
    check_packed(views, rects, ref, mode)
    assert cn["primary"] == area(rects) > w * h
    with pytest.raises(rtk.RtkError) as e:
        acc.render_regions(cfg, rects, rtk.REGIONS_IN_FRAME)
    assert e.value.code == rtk.RTK_ERR_INVALID
    views, _ = acc.render_regions(cfg, rects[:2], rtk.REGIONS_PACKED)       # the refused call left the accel usable
    check_packed(views, rects[:2], ref, (mode, "after the refusal"))
