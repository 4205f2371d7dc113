"""Keep or take on the device (csrc/order_judge.hpp, k_stamp / k_judge_order): a newly sorted launch order is judged behind its
first frame against the order before it, and the slower one's lists are dropped -- by a copy inside the set the frames read.  None
of that may show: 70 consecutive frames of one accel, across the sorts at frames 2, 18, 34 and 66 and the judges behind 18, 34 and
66, are each the frame of a fresh accel bit for bit with the same ray count; with a wait after every frame and with none at all
(the host then is frames ahead of the device and launches over every block until it has seen the list's length again); by the
scores and with the verdict forced either way (RTK_COST_JUDGE_FORCE).  The lists themselves are read out through
rtk_debug_order_lists: behind a judge that keeps the champion the set the frames read holds the champion's words, and whatever
the verdict the lists name every unit exactly once.  The same for a views call and a regions call, whose launches have tables of
their own.

Shapes: scene5 at 320x180 with four waves per block (920 blocks: the background's are packed four to a workgroup, the dragon's
have one each) and at 64x64 under RTK_TRACE_AUTO (64 blocks: eight waves, nothing packed)."""
import numpy as np
import pytest

from conftest import SCENE5

pytestmark = pytest.mark.gpu

DEPTH = 5
FRAMES = 70
AUTO, GROUP4 = 0, 3
BY_SCORE, ALWAYS_TAKE, ALWAYS_KEEP = 0, 1, 2
SORT_FRAMES = (2, 18, 34, 66)                 # 1-based: resort_every 16, doubling from the third sort on (frame_plan.hpp)
JUDGE_FRAMES = (18, 34, 66)
CASES = {"scene5_320_group4": (320, 180, GROUP4), "scene5_64_auto": (64, 64, AUTO)}
FORCES = {"by_score": BY_SCORE, "always_take": ALWAYS_TAKE, "always_keep": ALWAYS_KEEP}
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _accel(rtk, monkeypatch, force):
    """(the knobs are read when the accel is built)"""
    monkeypatch.setenv("RTK_COST_JUDGE_FORCE", str(force))
    return rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))


def _cfg(rtk, case):
    w, h, mode = CASES[case]
    return rtk.RenderConfig(width=w, height=h, max_ray_depth=DEPTH, trace_mode=mode)


def _fresh(rtk, case):
    """(frame, rays) of a fresh accel's first frame, made once per shape; never modified."""
    if case not in _cache:
        import torch
        cfg = _cfg(rtk, case)
        acc = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
        buf = torch.full((acc.output_floats(cfg),), float("nan"), dtype=torch.float32, device="cuda")
        acc.render_frame_device(cfg, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rays = acc.last_counters()["rays"]
        out = buf.cpu().numpy()
        out.setflags(write=False)
        assert np.isfinite(out).all() and rays > 0
        _cache[case] = (out, rays)
    return _cache[case]


def _units(w, h):
    """The units of a frame's lists: the 8x8 blocks of whole buckets (scene5's are 64x64: 960 for 320x180, 920 of them in the frame)."""
    return (-(-w // 64)) * (-(-h // 64)) * 64


def _check_lists(lists, units, packs):
    """order is a permutation of all units; the single and packed workgroups of the workgroup list cover every unit exactly once;
    the header says how many workgroups and units there are."""
    order, hdr, wg_list = lists
    assert order.size == units and wg_list.size == units
    assert int(hdr[1]) == units, hdr
    assert np.array_equal(np.sort(order), np.arange(units, dtype=np.uint32))
    n_wgs = int(hdr[0])
    assert 0 < n_wgs <= units
    wgs = wg_list[:n_wgs]
    packed = (wgs >> 31) == 1
    if not packs:
        assert not packed.any()
    seen = np.zeros(units, np.int64)
    np.add.at(seen, wgs[~packed], 1)
    for at in (wgs[packed] & 0x7FFFFFFF).tolist():
        assert at < units
        np.add.at(seen, order[at:min(at + 4, units)], 1)
    assert (seen == 1).all(), (int((seen == 0).sum()), int((seen > 1).sum()))
    # order[0, n_single): a workgroup each; the rest four to a workgroup
    n_single = int((~packed).sum())
    assert n_wgs == n_single + (units - n_single + 3) // 4
    return n_wgs


def _check_stats(st, force, units):
    assert st["sorts"] == len(SORT_FRAMES) and st["judges"] == len(JUDGE_FRAMES), st
    assert st["taken"] + st["rejected"] == len(JUDGE_FRAMES), st
    assert st["units"] == units, st
    if force == ALWAYS_TAKE:
        assert st["taken"] == len(JUDGE_FRAMES) and st["rejected"] == 0, st
    if force == ALWAYS_KEEP:
        assert st["taken"] == 0 and st["rejected"] == len(JUDGE_FRAMES), st
    # every scored frame took some microseconds and no second: the clock counts at 100 MHz
    assert 100 < st["challenger_ticks"] < 100_000_000 and 100 < st["champion_ticks"] < 100_000_000, st


@pytest.mark.parametrize("force", list(FORCES))
@pytest.mark.parametrize("case", list(CASES))
def test_seventy_frames_with_a_wait_after_each(rtk, monkeypatch, case, force):
    """Every frame is the fresh frame with its ray count.  Behind every judge the lists the frames read name every unit once; a judge
    that keeps the champion (forced, or by the scores) leaves the champion's lists there word for word, header included."""
    import torch
    cfg, (want, rays) = _cfg(rtk, case), _fresh(rtk, case)
    w, h, mode = CASES[case]
    units = _units(w, h)
    acc = _accel(rtk, monkeypatch, FORCES[force])
    s = torch.cuda.current_stream()
    buf = torch.empty((acc.output_floats(cfg),), dtype=torch.float32, device="cuda")
    champion = None
    for f in range(1, FRAMES + 1):
        if f in JUDGE_FRAMES:
            before = acc.order_judge()
            champion = np.concatenate(acc.order_lists(before["read_set"]))     # (the frame before left the challenger in the other set)
        buf.fill_(float("nan"))
        acc.render_frame_device(cfg, buf.data_ptr(), s.cuda_stream)
        assert acc.last_counters()["rays"] == rays, f
        assert np.array_equal(_bits(buf.cpu().numpy()), _bits(want)), f
        if f in JUDGE_FRAMES:
            st = acc.order_judge()
            assert st["read_set"] == before["read_set"] ^ 1, (f, st)
            assert st["judges"] == before["judges"] + 1 and st["taken"] + st["rejected"] == st["judges"], (f, st)
            lists = acc.order_lists(st["read_set"])
            _check_lists(lists, units, mode == GROUP4)
            kept = st["rejected"] == before["rejected"] + 1
            if FORCES[force] == ALWAYS_KEEP:
                assert kept, (f, st)
            if FORCES[force] == ALWAYS_TAKE:
                assert not kept, (f, st)
            if kept:
                assert np.array_equal(np.concatenate(lists), champion), f
                assert st["champion_ticks"] == before["champion_ticks"], (f, st, before)
            else:
                assert st["champion_ticks"] == st["challenger_ticks"], (f, st)
    _check_stats(acc.order_judge(), FORCES[force], units)
    # (the other set holds the list sorted behind no frame yet: whatever is there, the read set is whole)
    _check_lists(acc.order_lists(acc.order_judge()["read_set"]), units, mode == GROUP4)


@pytest.mark.parametrize("force", list(FORCES))
@pytest.mark.parametrize("case", list(CASES))
def test_seventy_frames_enqueued_without_a_wait(rtk, monkeypatch, case, force):
    """The host ahead of the device: 70 frames into 70 buffers with no wait in between.  The length of a list is not seen before the
    wait at the end, so behind a judge no launch may go by the length read back behind the sort: a kept champion's list can be longer."""
    import torch
    cfg, (want, rays) = _cfg(rtk, case), _fresh(rtk, case)
    w, h, mode = CASES[case]
    units = _units(w, h)
    acc = _accel(rtk, monkeypatch, FORCES[force])
    s = torch.cuda.current_stream()
    bufs = torch.full((FRAMES, acc.output_floats(cfg)), float("nan"), dtype=torch.float32, device="cuda")
    for i in range(FRAMES):
        acc.render_frame_device(cfg, bufs[i].data_ptr(), s.cuda_stream)
    assert acc.last_counters()["rays"] == rays
    out = bufs.cpu().numpy()
    for i in range(FRAMES):
        assert np.array_equal(_bits(out[i]), _bits(want)), i
    st = acc.order_judge()
    _check_stats(st, FORCES[force], units)
    _check_lists(acc.order_lists(st["read_set"]), units, mode == GROUP4)
    assert acc.counter_fills() == 2                             # the judge fills no counters: none from the third frame on


def _orbit_views(n):
    views = np.zeros((n, 12), np.float32)
    views[:, 3:] = np.eye(3, dtype=np.float32).reshape(-1)
    for i in range(n):
        views[i, :3] = [0.25 * i, 0.125 * i, 0.5 * (i % 2)]
    return views


def _check_table(rtk, acc, table, units):
    """The launch's own table after 40 calls under "always keep": sorted in front of call 2 and behind calls 17 and 33, judged behind
    18 and 34, both challengers rejected; a launch the calls never had reports zeros, and so does the frames' table."""
    st = acc.order_judge(table, 0)
    assert st["sorts"] == 3 and st["judges"] == 2 and st["taken"] == 0 and st["rejected"] == 2 and st["units"] == units, st
    assert 100 < st["champion_ticks"] < 100_000_000 and 100 < st["challenger_ticks"] < 100_000_000, st
    for other in (acc.order_judge(table, 1), acc.order_judge(rtk.ORDER_TABLE_FRAMES, 0)):
        assert all(other[k] == 0 for k in ("sorts", "judges", "taken", "rejected", "champion_ticks", "challenger_ticks")), other


def test_forty_views_calls_keep_their_champion(rtk, monkeypatch):
    """One rtk_render_views_device call of 4 views at 128x128 (1,024 units in one launch, its own tables), 40 times under "always
    keep": the sorts behind calls 17 and 33 are judged behind 18 and 34 and their lists dropped; every call is the first call by bits."""
    import torch
    cfg = rtk.RenderConfig(width=128, height=128, max_ray_depth=DEPTH, trace_mode=GROUP4)
    acc = _accel(rtk, monkeypatch, ALWAYS_KEEP)
    s = torch.cuda.current_stream()
    d_views = torch.from_numpy(_orbit_views(4)).cuda()
    n = 4 * acc.output_floats(cfg)
    first = None
    for i in range(40):
        out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        acc.render_views_device(cfg, d_views.data_ptr(), 4, out.data_ptr(), s.cuda_stream)
        rays = acc.last_counters()["rays"]
        got = out.cpu().numpy()
        if first is None:
            first = (got, rays)
            assert np.isfinite(got).all() and rays >= 4 * 128 * 128
        assert rays == first[1] and np.array_equal(_bits(got), _bits(first[0])), i
    _check_table(rtk, acc, rtk.ORDER_TABLE_VIEWS, 4 * 256)


def test_forty_regions_calls_keep_their_champion(rtk, monkeypatch):
    """The same for one rtk_render_regions_device call of 8 rectangles of 64x64 (at odd corners of a 320x180 frame; 512 units)."""
    import torch
    cfg = rtk.RenderConfig(width=320, height=180, max_ray_depth=DEPTH, trace_mode=GROUP4)
    rects = np.array([[3 + 70 * (k % 4), 5 + 95 * (k // 4), 3 + 70 * (k % 4) + 64, 5 + 95 * (k // 4) + 64] for k in range(8)], np.int32)
    acc = _accel(rtk, monkeypatch, ALWAYS_KEEP)
    s = torch.cuda.current_stream()
    n = 8 * 64 * 64 * 3
    first = None
    for i in range(40):
        out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        acc.render_regions_device(cfg, rects, rtk.REGIONS_PACKED, out.data_ptr(), s.cuda_stream)
        rays = acc.last_counters()["rays"]
        got = out.cpu().numpy()
        if first is None:
            first = (got, rays)
            assert np.isfinite(got).all() and rays >= 8 * 64 * 64
        assert rays == first[1] and np.array_equal(_bits(got), _bits(first[0])), i
    _check_table(rtk, acc, rtk.ORDER_TABLE_REGIONS, 8 * 64)


def _one_frame(acc, cfg, buf):
    import torch
    buf.fill_(float("nan"))
    acc.render_frame_device(cfg, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rays = acc.last_counters()["rays"]
    return buf.cpu().numpy(), rays


def test_lights_moved_at_an_equal_count_restart_the_schedule(rtk, monkeypatch):
    """40 frames (sorts at 2, 18, 34; the next would be in front of frame 66), then rtk_accel_set_lights with every light moved: the
    costs of the blocks under the shadow edges change, the order stays in use.  The intervals start over at 16 and the list keeps
    its age: the sort comes behind frame 49 with the champion's score taken under the new lights, the judge behind frame 50, and every
    frame is the frame of a fresh accel with those lights.  Then the lights move before EVERY frame (an animated light), back and
    forth between the two tables: the sorts stay 16 frames apart -- the call never puts one off."""
    import torch
    case = "scene5_320_group4"
    cfg = _cfg(rtk, case)
    acc = _accel(rtk, monkeypatch, BY_SCORE)
    buf = torch.empty((acc.output_floats(cfg),), dtype=torch.float32, device="cuda")
    want = _fresh(rtk, case)
    for f in range(1, 41):
        out, rays = _one_frame(acc, cfg, buf)
        assert rays == want[1] and np.array_equal(_bits(out), _bits(want[0])), f
    st40 = acc.order_judge()
    assert st40["sorts"] == 3 and st40["judges"] == 2, st40
    pos, inten = acc.lights()
    moved = pos + np.array([0.75, 0.25, -0.5], np.float32)
    ref = rtk.KdTreeSimdAccel(rtk.parse_scene_file(SCENE5))
    ref.set_lights(moved, inten)
    want_moved = _one_frame(ref, cfg, torch.empty_like(buf))
    assert not np.array_equal(_bits(want_moved[0]), _bits(want[0]))
    acc.set_lights(moved, inten)
    for f in range(41, 61):
        out, rays = _one_frame(acc, cfg, buf)
        assert rays == want_moved[1] and np.array_equal(_bits(out), _bits(want_moved[0])), f
        st = acc.order_judge()
        assert st["sorts"] == (3 if f < 49 else 4) and st["judges"] == (2 if f < 50 else 3), (f, st)
        assert st["units"] == st40["units"], (f, st)
        if f == 49:
            assert st["champion_ticks"] > 100, st             # (scored behind frame 49, under the new lights)
        if f == 50:
            _check_lists(acc.order_lists(st["read_set"]), st["units"], True)
    # frames 61-100, the lights set before every one: new lists at 66, 82 and 98, their sorts behind 65, 81 and 97
    tables = {0: (pos, inten, want), 1: (moved, inten, want_moved)}
    for f in range(61, 101):
        p, i, w = tables[f % 2]
        acc.set_lights(p, i)
        out, rays = _one_frame(acc, cfg, buf)
        assert rays == w[1] and np.array_equal(_bits(out), _bits(w[0])), f
        st = acc.order_judge()
        assert st["sorts"] == 4 + sum(f >= b for b in (65, 81, 97)) and st["judges"] == 3 + sum(f >= j for j in (66, 82, 98)), (f, st)


def test_the_champions_score_is_cleared_scored_and_left(rtk, monkeypatch):
    """What k_order_by_cost does with the champion's score.  A shape's first sort, in front of frame 2, clears it: no frame has run
    under a sorted list.  The sort behind frame 17 stores that frame's time.  With a new list every frame (RTK_COST_RESORT_EVERY=1)
    every frame from the third has the judge AND the sort behind it: the sort must leave what the judge stored -- under "always
    take" the challenger's own score (an interval given without a cap is not stretched: accel.hpp) -- and not score the frame again, which would add the judge's time."""
    import torch
    case = "scene5_64_auto"
    cfg = _cfg(rtk, case)
    acc = _accel(rtk, monkeypatch, BY_SCORE)
    buf = torch.empty((acc.output_floats(cfg),), dtype=torch.float32, device="cuda")
    for f in range(1, 18):
        _one_frame(acc, cfg, buf)
        st = acc.order_judge()
        if f < 17:
            assert st["champion_ticks"] == 0 and st["sorts"] == (0 if f < 2 else 1), (f, st)
        else:
            assert st["champion_ticks"] > 100 and st["sorts"] == 2 and st["judges"] == 0, (f, st)
    monkeypatch.setenv("RTK_COST_RESORT_EVERY", "1")
    acc = _accel(rtk, monkeypatch, ALWAYS_TAKE)
    for f in range(1, 7):
        _one_frame(acc, cfg, buf)
        st = acc.order_judge()
        if f >= 3:
            assert st["judges"] == f - 2 and st["taken"] == f - 2 and st["sorts"] == f, (f, st)
            assert st["champion_ticks"] == st["challenger_ticks"] > 100, (f, st)
