"""rtk_render_regions[_device] without a GPU: the symbols and the Python door, the order of the argument checks (what a frame
refuses, the refused engines and flags, the pointers, the rectangles' bounds, overlaps under RTK_REGIONS_IN_FRAME, then lists
without pixels, then the missing device), and an accel that stays usable after every refusal."""
import ctypes

import numpy as np
import pytest

from conftest import SCENE5

SYMBOLS = ("rtk_render_regions", "rtk_render_regions_device")
W, H = 40, 24
SENTINEL = np.float32(-7.0)


def _accel(rtk):
    sc = rtk.parse_scene_file(SCENE5)
    return sc, rtk.KdTreeSimdAccel(sc)


def _rects(*rows):
    return np.ascontiguousarray(np.array(rows, np.int32).reshape(-1, 4))


def test_library_exports_the_region_symbols(rtk):
    lib = ctypes.CDLL(rtk.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in rtk.ABI_SYMBOLS
    assert rtk.abi_version() == 4
    for name in ("render_regions", "render_regions_device"):
        assert hasattr(rtk.KdTreeSimdAccel, name)
    assert (rtk.REGIONS_IN_FRAME, rtk.REGIONS_PACKED) == (0, 1) and rtk.MAX_REGIONS == 65536
    r = rtk.Rect(3, 4, 10, 6)
    assert (r.width, r.height, r.area) == (7, 2, 14)


def test_header_declares_what_the_library_exports():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "rtk.h")).read()
    assert "#define RTK_ABI_VERSION 4" in text
    assert "typedef struct { int32_t x0, y0, x1, y1; } rtk_rect;" in text
    assert "enum { RTK_REGIONS_IN_FRAME = 0, RTK_REGIONS_PACKED = 1 };" in text
    for name in SYMBOLS:
        assert f"int {name}(" in text


def _calls(rtk, acc):
    L = rtk.lib()

    def host(p, r, n, layout, o):
        return L.rtk_render_regions(acc._h, ctypes.byref(p), r, n, layout, o, None)

    def dev(p, r, n, layout, o):
        return L.rtk_render_regions_device(acc._h, ctypes.byref(p), r, n, layout, o, None)

    return host, dev


def test_region_argument_errors_in_their_order(rtk):
    _, acc = _accel(rtk)
    L = rtk.lib()
    INV, OK = rtk.RTK_ERR_INVALID, rtk.RTK_OK
    IN_FRAME, PACKED = rtk.REGIONS_IN_FRAME, rtk.REGIONS_PACKED
    out = np.full((H, W, 3), SENTINEL, np.float32)
    O = out.ctypes.data
    good = _rects((1, 2, 9, 7), (20, 3, 31, 4))
    G = good.ctypes.data
    ok = rtk.RenderConfig(width=W, height=H)
    before = acc.tree_dump()
    for call in _calls(rtk, acc):
        # 1. a NULL accel or p, then what a frame refuses for *p -- whatever the rectangles are
        assert L.rtk_render_regions(None, ctypes.byref(ok.to_c()), G, 2, PACKED, O, None) == INV
        assert L.rtk_render_regions_device(None, ctypes.byref(ok.to_c()), G, 2, PACKED, O, None) == INV
        assert L.rtk_render_regions(acc._h, None, G, 2, PACKED, O, None) == INV
        assert L.rtk_render_regions_device(acc._h, None, G, 2, PACKED, O, None) == INV
        for bad in (rtk.RenderConfig(width=W, height=H, spp=0), rtk.RenderConfig(width=70000, height=H),
                    rtk.RenderConfig(width=W, height=H, trace_mode=99), rtk.RenderConfig(width=W, height=H, max_ray_depth=17),
                    rtk.RenderConfig(width=W, height=H, spp=2, sample_begin=2)):
            assert call(bad.to_c(), G, 2, PACKED, O) == INV
            assert call(bad.to_c(), None, 0, PACKED, None) == INV
        # 2. the refused engines and flags, the count, the layout -- before n_rects == 0 and before the pointers
        for mode in (rtk.TRACE_LANE, rtk.TRACE_WAVE, rtk.TRACE_TWOPASS):
            assert call(rtk.RenderConfig(width=W, height=H, trace_mode=mode).to_c(), G, 2, PACKED, O) == INV
            assert call(rtk.RenderConfig(width=W, height=H, trace_mode=mode).to_c(), None, 0, PACKED, None) == INV
        for stats in (1, 2):
            assert call(rtk.RenderConfig(width=W, height=H, collect_stats=stats).to_c(), G, 0, PACKED, O) == INV
        assert call(rtk.RenderConfig(width=W, height=H, world_size=2).to_c(), G, 2, PACKED, O) == INV
        assert call(rtk.RenderConfig(width=W, height=H, world_size=2).to_c(), G, 0, PACKED, O) == INV      # before n_rects == 0
        assert call(ok.to_c(), G, -1, PACKED, O) == INV
        assert call(ok.to_c(), G, 65537, PACKED, O) == INV
        for layout in (-1, 2, 99):
            assert call(ok.to_c(), G, 2, layout, O) == INV
            assert call(ok.to_c(), None, 0, layout, None) == INV
        # 3. NULL rects or output with n_rects > 0
        assert call(ok.to_c(), None, 2, PACKED, O) == INV
        assert call(ok.to_c(), G, 2, PACKED, None) == INV
        # 4. a rectangle outside the frame or inside out; x1 == width and y1 == height are inside
        for row in ((-1, 0, 4, 4), (0, -1, 4, 4), (5, 0, 4, 4), (0, 5, 4, 4), (0, 0, W + 1, 4), (0, 0, 4, H + 1),
                    (W + 1, 0, W + 1, 4), (-2, 3, -2, 3)):
            bad = _rects((1, 2, 9, 7), row)
            for layout in (IN_FRAME, PACKED):
                assert call(ok.to_c(), bad.ctypes.data, 2, layout, O) == INV, row
        # 5. overlap: refused under IN_FRAME only (a bad rectangle is reported before it: it comes first in the order)
        over = _rects((1, 2, 9, 7), (8, 6, 12, 10))
        assert call(ok.to_c(), over.ctypes.data, 2, IN_FRAME, O) == INV
        assert b"overlap" in L.rtk_last_error()
        both = _rects((1, 2, 9, 7), (8, 6, 12, 10), (0, 0, W + 1, 4))
        assert call(ok.to_c(), both.ctypes.data, 3, IN_FRAME, O) == INV
        assert b"overlap" not in L.rtk_last_error()
        # then lists without pixels: nothing to do, device or not -- overlapping empties and empties at the frame's far edge included
        assert call(ok.to_c(), None, 0, PACKED, None) == OK
        assert call(ok.to_c(), G, 0, IN_FRAME, O) == OK
        hollow = _rects((3, 3, 3, 9), (3, 3, 3, 9), (0, 5, W, 5), (W, H, W, H), (W, 0, W, H))
        for layout in (IN_FRAME, PACKED):
            assert call(ok.to_c(), hollow.ctypes.data, 5, layout, O) == OK
    assert np.array_equal(out.view(np.uint32), np.full(out.shape, SENTINEL, np.float32).view(np.uint32))     # nothing was written
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()


def test_valid_calls_reach_the_device_check(rtk):
    """What is accepted: the frame's far edge, touching rectangles under IN_FRAME, overlaps under PACKED, 65,536 rectangles.
    Without a device "accepted" is RTK_ERR_NO_DEVICE; with one the call renders."""
    _, acc = _accel(rtk)
    L = rtk.lib()
    want = rtk.RTK_OK if rtk.device_count() > 0 else rtk.RTK_ERR_NO_DEVICE
    IN_FRAME, PACKED = rtk.REGIONS_IN_FRAME, rtk.REGIONS_PACKED
    ok = rtk.RenderConfig(width=W, height=H)
    edge = _rects((W - 3, H - 2, W, H), (0, 0, W - 3, H - 2), (W - 3, 0, W, H - 2), (0, 0, 0, 0))      # x1 == width, y1 == height, touching
    over = _rects((1, 2, 9, 7), (8, 6, 12, 10), (1, 2, 9, 7))
    many = np.zeros((65536, 4), np.int32)
    many[0] = (0, 0, 1, 1)
    # (the buffers are host memory: the device variant takes them only where no device can be handed them -- with a device its
    # accepted calls are tests/test_gpu_regions.py's, on device buffers)
    host, dev = _calls(rtk, acc)
    for call in ((host,) if rtk.device_count() > 0 else (host, dev)):
        frame = np.full((H, W, 3), SENTINEL, np.float32)
        assert call(ok.to_c(), edge.ctypes.data, 4, IN_FRAME, frame.ctypes.data) == want
        packed = np.full((40 + 16 + 40) * 3, SENTINEL, np.float32)
        assert call(ok.to_c(), over.ctypes.data, 3, PACKED, packed.ctypes.data) == want
        assert call(ok.to_c(), many.ctypes.data, 65536, IN_FRAME, frame.ctypes.data) == want
    assert acc.tree_info().n_nodes > 0 and len(acc.tree_dump()[2]) > 0            # the accel still answers


def test_python_door_shapes_and_refusals(rtk):
    _, acc = _accel(rtk)
    ok = rtk.RenderConfig(width=W, height=H)
    # lists without pixels need no device: the frame comes back as it went in, the packed list as views without pixels
    frame = np.full((H, W, 3), SENTINEL, np.float32)
    got, cn = acc.render_regions(ok, [rtk.Rect(3, 3, 3, 9), (0, 5, W, 5)], rtk.REGIONS_IN_FRAME, frame)
    assert got is frame and (frame == SENTINEL).all() and cn["rays"] == 0 and cn["primary"] == 0
    views, cn = acc.render_regions(ok, _rects((3, 3, 3, 9), (0, 5, W, 5)), rtk.REGIONS_PACKED)
    assert [v.shape for v in views] == [(6, 0, 3), (0, W, 3)] and cn["rays"] == 0
    views, _ = acc.render_regions(ok, [], rtk.REGIONS_PACKED)
    assert views == []
    acc.render_regions_device(ok, np.zeros((0, 4), np.int32), rtk.REGIONS_PACKED, 0)
    for bad in (np.zeros((2, 3), np.int32), np.zeros((2, 4), np.float32), np.zeros(8, np.int32), [(0, 0, 2**31, 1)]):
        with pytest.raises(ValueError):
            acc.render_regions(ok, bad, rtk.REGIONS_PACKED)
    with pytest.raises(ValueError):                                                # the wrong buffer for the layout
        acc.render_regions(ok, [(0, 0, 4, 4)], rtk.REGIONS_PACKED, frame)
    with pytest.raises(ValueError):                                                # a later pass needs the sums of the earlier ones
        acc.render_regions(rtk.RenderConfig(width=W, height=H, spp=2, sample_begin=1, sample_count=1), [(0, 0, 4, 4)], rtk.REGIONS_PACKED)
    with pytest.raises(rtk.RtkError) as e:
        acc.render_regions(ok, [(0, 0, 4, 4), (3, 3, 6, 6)], rtk.REGIONS_IN_FRAME)
    assert e.value.code == rtk.RTK_ERR_INVALID
    with pytest.raises(rtk.RtkError) as e:
        acc.render_regions(rtk.RenderConfig(width=W, height=H, world_size=2), [], rtk.REGIONS_PACKED)
    assert e.value.code == rtk.RTK_ERR_INVALID


def test_without_a_device_a_valid_call_is_no_device_and_the_accel_stays_usable(rtk):
    _, acc = _accel(rtk)
    before = acc.tree_dump()
    if rtk.device_count() == 0:
        for layout in (rtk.REGIONS_IN_FRAME, rtk.REGIONS_PACKED):
            with pytest.raises(rtk.RtkError) as e:
                acc.render_regions(rtk.RenderConfig(width=W, height=H), [(1, 2, 9, 7)], layout)
            assert e.value.code == rtk.RTK_ERR_NO_DEVICE
            with pytest.raises(rtk.RtkError) as e:
                acc.render_regions_device(rtk.RenderConfig(width=W, height=H), [(1, 2, 9, 7)], layout, before[0].ctypes.data)   # (never dereferenced)
            assert e.value.code == rtk.RTK_ERR_NO_DEVICE
    else:
        views, cn = acc.render_regions(rtk.RenderConfig(width=W, height=H), [(1, 2, 9, 7)], rtk.REGIONS_PACKED)
        assert views[0].shape == (5, 8, 3) and cn["primary"] == 40
    for x, y in zip(before, acc.tree_dump()):
        assert x.tobytes() == y.tobytes()
    acc.set_camera(np.ones(3, np.float32), np.eye(3, dtype=np.float32))           # and goes on taking the calls that need no device
    assert acc.camera()[0].tolist() == [1.0, 1.0, 1.0]
