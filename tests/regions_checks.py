"""What the tests of rtk_render_regions share (test_gpu_regions.py): rectangle lists made from a frame's size, and the comparison of
what a call returns with crops of a reference frame, by bits.  A reference frame is the CPU oracle's (views_checks.Oracle, computed
once per shape) or, where the test says so, the frame the same accel renders."""
import numpy as np

from views_checks import bits

SENTINEL = np.float32(-7.0)


def crop(frame, r):
    x0, y0, x1, y1 = (int(v) for v in r)
    return frame[y0:y1, x0:x1]


def area(rects):
    return int(sum((int(r[2]) - int(r[0])) * (int(r[3]) - int(r[1])) for r in rects))


def around(w, h, r):
    """The four rectangles that, with r, tile the w x h frame: the rows above it, the rows below it, what is left and right of it."""
    x0, y0, x1, y1 = r
    return [(0, 0, w, y0), (0, y1, w, h), (0, y0, x0, y1), (x1, y0, w, y1)]


def grid_rects(w, h, seed, cell=16):
    """One rectangle per cell of a `cell`-pixel grid over the frame, each inset from its cell by 0..4 pixels on every side: pairwise
    disjoint, some touching.  Every 9th is one pixel wide, every 11th one pixel high, every 37th has no pixels."""
    rng = np.random.default_rng(seed)
    out = []
    for cy in range(0, h, cell):
        for cx in range(0, w, cell):
            i = len(out)
            a, b, c, d = (int(v) for v in rng.integers(0, 5, 4))
            x0, y0 = cx + a, cy + b
            x1, y1 = min(cx + cell, w) - c, min(cy + cell, h) - d
            x1, y1 = max(x1, x0 + 1), max(y1, y0 + 1)
            if i % 9 == 4:
                x1 = x0 + 1
            if i % 11 == 7:
                y1 = y0 + 1
            if i % 37 == 20:
                x1 = x0
            out.append((x0, y0, x1, y1))
    return out


def check_packed(views, rects, ref, what):
    """every view of a packed call is the crop of `ref`"""
    assert len(views) == len(rects), what
    for i, (v, r) in enumerate(zip(views, rects)):
        want = crop(ref, r)
        assert v.shape == want.shape, (what, i, r, v.shape)
        bad = int((bits(v) != bits(want)).any(axis=-1).sum())
        assert bad == 0, (what, i, r, bad)


def inside_mask(w, h, rects):
    m = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in rects:
        m[y0:y1, x0:x1] = True
    return m


def check_in_frame(frame, rects, ref, what, sentinel=SENTINEL):
    """inside the rectangles the frame is `ref`; every float outside them still has the sentinel's bits"""
    h, w = ref.shape[:2]
    assert frame.shape == (h, w, 3), what
    m = inside_mask(w, h, rects)
    bad = int((bits(frame)[m] != bits(ref)[m]).any(axis=-1).sum())
    assert bad == 0, (what, "inside", bad)
    touched = int((bits(frame)[~m] != bits(np.float32(sentinel))).any(axis=-1).sum())
    assert touched == 0, (what, "outside", touched)
