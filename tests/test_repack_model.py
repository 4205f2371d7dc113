"""The float32 model of csrc/repack.hip (tests/repack_model.py) held to properties that do not restate the heuristic: they are
the model's licence before tests/test_gpu_repack_probe.py holds the device to it.  The key map is a monotone bijection, the
octahedral map injective and continuous across its fold, the Morton interleave a bijection, every key below 2^30, a batch
sorted by its keys is judged coherent by the probe's own measure, and the raster width is the row length (or, for a row length
that is no multiple of 8, 0 or a multiple of it).  Needs no GPU.  The figures are printed (pytest -s)."""
import math

import numpy as np
import pytest

import repack_cases as rc
import repack_model as rm

f32 = np.float32
u32 = np.uint32


def test_f2key_is_a_strictly_monotone_bijection():
    x = np.asarray([-np.inf, -3.0e38, -1.0e30, -1.0, -1.0e-38, -1.0e-40, -1.0e-45, -0.0, 0.0, 1.0e-45, 1.0e-40, 1.0e-38, 1.0, 1.0e30,
                    3.0e38, np.inf], f32)
    k = rm.f2key(x)
    assert (np.diff(k.astype(np.int64)) > 0).all(), k                        # -0 < +0 included
    assert np.array_equal(rm.key2f(k).view(u32), x.view(u32))
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(u32)
    fl = bits.view(f32)
    assert np.array_equal(rm.key2f(rm.f2key(fl)).view(u32), bits)            # NaN payloads too
    fl = np.sort(fl[~np.isnan(fl)])
    kk = rm.f2key(fl).astype(np.int64)
    assert (np.diff(kk) >= 0).all() and ((np.diff(kk) > 0) == (np.diff(fl.view(u32).astype(np.int64)) != 0)).all()


@pytest.mark.parametrize("pole", [0, 1, 2, 4, 5, 6])
def test_octa_map_is_bounded_injective_and_continuous_across_the_fold(pole):
    rng = np.random.default_rng(10 + pole)
    d = rc.sphere(rng, 40_000).astype(f32)
    u, v = rm.octa_map(d, pole)
    assert (np.abs(u) <= 1.0).all() and (np.abs(v) <= 1.0).all()
    def cell_of(u, v):
        return (np.floor((u.astype(np.float64) + 1.0) * 16384).clip(0, 32767).astype(np.int64) << 15) \
            | np.floor((v.astype(np.float64) + 1.0) * 16384).clip(0, 32767).astype(np.int64)

    # a neighbour 1e-3 away in a random tangent direction: another 15-bit cell, always
    t = np.cross(d.astype(np.float64), rng.normal(size=d.shape))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    d2 = d + 1.0e-3 * t
    d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(f32)
    dist = np.linalg.norm(d2.astype(np.float64) - d, axis=1)
    assert dist.min() > 0.99e-3
    cell, cell2 = cell_of(u, v), cell_of(*rm.octa_map(d2, pole))
    assert (cell != cell2).all()
    # ... and whatever of the sample shares a cell is closer than that
    both = np.concatenate([cell, cell2]); dd2 = np.concatenate([d, d2]).astype(np.float64)
    order = np.argsort(both, kind="stable")
    same = np.nonzero(np.diff(both[order]) == 0)[0]
    worst = max([float(np.linalg.norm(dd2[order[i + 1]] - dd2[order[i]])) for i in same], default=0.0)
    print(f"pole {pole}: {len(same)} pairs of {len(both)} directions share a 15-bit cell, the farthest {worst:.2e} apart")
    assert worst < 1.0e-3
    # the fold: the same (a, b) a hair on either side of c = 0.  Unfolded |a| / (A + eps), folded 1 - |b| / (A + eps) with
    # A = |a| + |b|: they differ by eps / (A + eps), plus a few float32 roundings of numbers below 1
    axis = pole & 3
    ab = rng.uniform(-1.0, 1.0, size=(2000, 2))
    A = np.abs(ab).sum(axis=1)
    eps = 1.0e-6
    dd = np.zeros((2000, 3))
    dd[:, (1, 2, 0)[axis]] = ab[:, 0]; dd[:, (2, 0, 1)[axis]] = ab[:, 1]
    dd[:, axis] = eps
    up = rm.octa_map(dd.astype(f32), pole)
    dd[:, axis] = -eps
    dn = rm.octa_map(dd.astype(f32), pole)
    gap = np.maximum(np.abs(up[0] - dn[0]), np.abs(up[1] - dn[1]))
    assert (gap <= eps / A + 8 * 2.0 ** -24).all(), float((gap - eps / A).max())
    assert ((up[0] >= 0) == (dn[0] >= 0)).all() and ((up[1] >= 0) == (dn[1] >= 0)).all()      # the same quadrant on both sides
    # the pole itself is the middle, its antipode a corner; a zero direction has no image
    p = np.zeros((3, 3), f32); p[0, axis] = -1.0 if pole & 4 else 1.0; p[1, axis] = -p[0, axis]
    u, v = rm.octa_map(p, pole)
    assert (u[0], v[0]) == (0.0, 0.0) and abs(u[1]) == 1.0 and abs(v[1]) == 1.0 and np.isnan(u[2]) and np.isnan(v[2])


def test_octa_pole_of_the_first_ray():
    assert rm.octa_pole(np.zeros((0, 6), f32)) == 2
    for pole, first in rc.POLE_FIRSTS.items():
        assert rm.octa_pole(rc.one_origin_sphere(100, first=first)) == pole
    assert rm.octa_pole(np.asarray([[0, 0, 0, 0.5, 0.5, 0.5]], f32)) == 2    # ties go to z, then y
    assert rm.octa_pole(np.asarray([[0, 0, 0, 0.5, 0.5, 0.1]], f32)) == 1


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_spread_bits_interleave_is_a_monotone_bijection(n):
    bits = 30 // n
    full = np.arange(1 << min(bits, 16), dtype=u32)
    s = rm.spread_bits(full, n, bits)
    assert np.array_equal(s, rm.spread_bits_loop(full, n, bits))              # the magic masks of n = 2, 3 against the loop, every x
    assert (np.diff(s.astype(np.int64)) > 0).all()                           # monotone in the coordinate (the others fixed: OR of disjoint bits)
    rng = np.random.default_rng(n)
    c = rng.integers(0, 1 << bits, size=(50_000, n), dtype=np.uint64).astype(u32)
    c[0] = 0; c[1] = (1 << bits) - 1
    key = np.zeros(len(c), u32)
    for j in range(n):
        sj = rm.spread_bits(c[:, j], n, bits)
        assert (key & (sj << u32(n - 1 - j))).max() == 0                     # disjoint bit sets
        key |= sj << u32(n - 1 - j)
    assert key.max() == (1 << (bits * n)) - 1 and key.max() < 1 << 30
    back = np.zeros_like(c)                                                  # decode: bit b of coordinate j sits at b * n + (n - 1 - j)
    for j in range(n):
        for b in range(bits):
            back[:, j] |= ((key >> u32(b * n + n - 1 - j)) & u32(1)) << u32(b)
    assert np.array_equal(back, c)


def _all_batches(n=4097):
    out = {}
    for name, (rays, truth) in rc.families(n).items():
        out[name] = (rays, 1, truth)
    out["outside_sample"] = (rc.outside_sample(n, 3)[0], 3, None)
    out["raster_128_fov90_shuffled"] = (rc.shuffled(rc.raster(128, 128, 90.0)), 16, (1, 2))
    return out


@pytest.mark.parametrize("n", [1024, 4097, 2 ** 14 + 77, 64 * (4 * 2048 + 5)])
def test_family_verdicts_are_the_stated_ones_and_clear_of_the_threshold(n):
    """The sizes at which the device test holds the probe's verdict to the truth of each family."""
    for name, (rays, stride, truth) in _all_batches(n).items():
        words, _ = rm.bounds(rays, stride, True)
        wide, spread, oext, _ = rm.shares(words)
        got = rm.verdict(words)
        print(f"{name}: wide {float(wide):.3f} spread {float(spread):.3f} -> sort {got[0]} dims {got[1]}")
        assert not (0.2 <= wide <= 0.3) and not (0.2 <= spread <= 0.3), name
        if truth is not None:
            assert got == truth, (name, got, truth)


def test_every_key_is_below_2_to_the_30():
    """One varying dimension has 30 bits, and the float clamp bound 2^30 - 1 rounds to 2^30: without the integer clamp the ray at the
    maximum gets key 0x40000000, outside the sorted bits, and comes first.  Two and more dimensions never reach their bound's
    rounding (15 bits and fewer), so their keys are the same with and without it."""
    for name, (rays, stride, _) in _all_batches().items():
        words, _ = rm.bounds(rays, stride, False)
        for dirs3 in (0, 1):
            k = rm.keys(rays, words, dirs3)
            assert int(k.max()) < 1 << 30, (name, dirs3, hex(int(k.max())))
            old = rm.keys(rays, words, dirs3, clamp_after=False)
            n_active = len(rm.key_layout(words, dirs3)[1])
            if n_active >= 2:
                assert np.array_equal(k, old), name
    line = rc.line(4097)
    words, _ = rm.bounds(line, 1, False)
    old = rm.keys(line, words, clamp_after=False)
    new = rm.keys(line, words)
    assert int(old.max()) == 1 << 30 and int(np.argmax(old)) == 4096         # the finding: the last ray of the line
    assert list(rm.order(old)[:2]) == [0, 4096]                              # ... came first, next to ray 0: bit 30 is not sorted on
    assert rm.order(new)[-1] == 4096 and np.array_equal(new[:-1], old[:-1])
    assert (np.diff(new.astype(np.int64)) >= 0).all()                        # keys along the line are monotone


def test_verdict_dims_are_the_keys_dims_also_with_three_direction_components():
    """RTK_REPACK_DIRS3 with one origin: the keys take three direction components, ten bits each.  A verdict that counts the two
    octahedral coordinates lets the host skip 14 low bits -- of a key whose dimensions have 10."""
    for name, (rays, stride, _) in _all_batches().items():
        words, _ = rm.bounds(rays, stride, True)
        for dirs3 in (0, 1):
            assert rm.verdict(words, dirs3)[1] == len(rm.key_layout(words, dirs3)[1]), (name, dirs3)
    words, _ = rm.bounds(rc.one_origin_sphere(4097), 1, True)
    assert rm.verdict(words, 0)[1] == 2 and len(rm.key_layout(words, 1)[1]) == 3      # what disagreed
    assert rm.sort_from_bit(2) == 14 and rm.sort_from_bit(3) == 6


def _wide_share(rays):
    w, _ = rm.bounds(rays, 1, True)
    return float(rm.shares(w)[0]), rm.verdict(w)[0]


@pytest.mark.parametrize("size,fov", [(128, 37.5), (128, 90.0), (512, 37.5), (512, 90.0)])
def test_a_batch_sorted_by_its_keys_is_coherent_by_the_probes_own_measure(size, fov):
    """Closed loop, no implementation in the expectation: shuffled camera rays are judged incoherent; the same rays in the order of
    their keys are judged coherent, with all key bits sorted and with the 14 lowest left out (the host's choice for two
    dimensions); the pixel order is coherent where 64 pixels of a row are less than 0.25 apart.  At 128 x 128 a wave is half a
    row, 0.3 and more wide at either fov: there the pixel order is itself what the probe calls incoherent."""
    pix = rc.raster(size, size, fov)
    shuf = rc.shuffled(pix, size)
    n = len(pix)
    words, _ = rm.bounds(shuf, rm.probe_stride(n), True)
    sort, dims = rm.verdict(words)
    assert (sort, dims) == (1, 2)
    k = rm.keys(shuf, words)
    share_shuf, _ = _wide_share(shuf)
    share_pix, sort_pix = _wide_share(pix)
    out = [share_shuf, share_pix]
    for bb in (0, rm.sort_from_bit(dims)):
        share, s = _wide_share(shuf[rm.order(k, bb)])
        out.append(share)
        assert s == 0 and share < 0.2, (bb, share)
    print(f"{size}x{size} fov {fov}: wide share shuffled {out[0]:.3f}, pixel order {out[1]:.3f}, sorted {out[2]:.3f}, sorted from bit 14 {out[3]:.3f};"
          f" {n - len(np.unique(k))} of {n} keys collide")
    assert share_shuf > 0.3
    assert not 0.2 <= share_pix <= 0.3
    if 2.0 * math.tan(math.radians(fov) / 2.0) * 64.0 / size < 0.25:          # (normalising only shortens the difference)
        assert sort_pix == 0 and share_pix < 0.2
    else:
        assert size == 128 and share_pix > 0.3


@pytest.mark.parametrize("w,h,fov", [(64, 16, 90.0), (64, 40, 37.5), (72, 17, 90.0), (128, 16, 37.5), (640, 16, 90.0), (1920, 17, 37.5)])
def test_raster_width_of_a_row_length_that_is_a_multiple_of_8(w, h, fov):
    r = rc.raster(w, h, fov)
    assert rm.raster_width(r) == w
    assert rm.raster_width(rc.repeated(r, len(r) + 3 * w + 77)) == w          # a frame and a ragged tail
    assert rm.raster_width(r[:16 * w]) == w and rm.raster_width(r[:16 * w - 1]) == 0
    assert rm.raster_width(rc.shuffled(r)) == 0
    # by design only the first sixteen rows are looked at, and that a seventeenth begins where it should: what follows does not
    # matter (lane placement hangs on the answer, no result)
    tall = rc.raster_then_noise(w, 40, fov, 16)
    assert rm.raster_width(tall) == w
    assert rm.raster_width(rc.raster_then_noise(w, 40, fov, 15)) == 0         # ... but every one of the sixteen does


ODD_ANSWERS = {}


@pytest.mark.parametrize("w,h", [(60, 40), (66, 80), (100, 40), (333, 400)])
@pytest.mark.parametrize("fov", [37.5, 90.0])
def test_raster_width_of_a_row_length_that_is_no_multiple_of_8(w, h, fov):
    """The first jump is looked for at positions 64 + 8k only, so such a raster is seen as one of lcm(w, 8) or not at all.  Both are
    accepted: a multiple of the true row length is a raster too (its rows are several real rows), the 8x8 deal of k_intersect
    then takes pieces of real rows that lie under each other, and only lane placement hangs on it.  What is pinned: the answer
    is 0 or a multiple of the true row length, a multiple of 8, >= 64, with sixteen of its rows in the batch."""
    r = rc.raster(w, h, fov)
    got = rm.raster_width(r)
    print(f"row length {w} (x{h}, fov {fov}): raster width {got}" + (f" = {got // w} rows" if got else ""))
    assert got == 0 or (got % w == 0 and got % 8 == 0 and got >= 64 and 16 * got <= len(r))
    if got:
        assert got == w * 8 // math.gcd(w, 8)
