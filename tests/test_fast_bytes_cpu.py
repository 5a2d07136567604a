"""CPU: the byte form of the FAST pair test (tests/fast_bytes.py: saturated thresholds, two v_lerp_u8 per ring pixel, pair
logic on bit 7) equals the integer comparisons of tests/fast_sides.py -- for every (r, v) byte pair per comparison, and
per pixel on the boundary-stamp images; and those images hold every boundary regime at least 100 times at level 0."""
import numpy as np
import pytest

from tests import fast_bytes as fb
from tests import fast_sides as fs

THRS = (1, 15, 120, 254)


@pytest.mark.parametrize("thr", THRS)
def test_lerp_flags_exhaustive(thr):
    """all 256 x 256 (r, v): not-darker is r >= v - thr, brighter is r > v + thr, saturated ends included"""
    r, v = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32))
    nd, br = fb.flags(v, r, thr)
    assert np.array_equal(nd, ~(v - r > thr))
    assert np.array_equal(br, r - v > thr)
    yd, yb = fb.thresholds(v, thr)
    assert yd.min() >= 0 and yd.max() <= 255 and yb.min() >= 0 and yb.max() <= 255      # they are bytes


@pytest.mark.parametrize("thr", THRS)
def test_sides_exhaustive_pairs(thr):
    """every (v, r_a) with eight r_b across the range for one opposite pair, the other three pairs passing both sides
    (0 and 255) or refusing both (v and v): the pair logic on bit 7 equals fast_sides.sides"""
    v, ra, rb = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32),
                            np.array([0, 1, 64, 127, 128, 191, 254, 255], np.int32), indexing="ij")
    for p, (a, b) in enumerate(fs.PAIRS):
        for passing in (True, False):
            r = np.empty((16,) + v.shape, np.int32)
            r[:] = v
            for a2, b2 in fs.PAIRS:
                r[a2], r[b2] = (0, 255) if passing else (v, v)
            r[a], r[b] = ra, rb
            for got, ref in zip(fb.sides(v, r, thr), fs.sides(v, r, thr)):
                assert np.array_equal(got, ref), (thr, p, passing)
        if thr != THRS[0]:
            break                                         # the pairs are symmetric in the model: all four at one threshold


@pytest.mark.parametrize("thr", THRS)
def test_boundary_stamps(oracle, thr):
    img = fb.boundary_stamps(thr)
    assert img.shape == (480, 640) and img.dtype == np.uint8
    v, r = fs.ring(img)
    dark, brt = fs.sides(v, r, thr)
    got_dark, got_brt = fb.sides(v, r, thr)
    assert np.array_equal(got_dark, dark) and np.array_equal(got_brt, brt)
    # the regimes, level 0 (a condition on the input, fixed)
    lo = np.max([np.minimum(r[a], r[b]) for a, b in fs.PAIRS], axis=0)
    hi = np.min([np.maximum(r[a], r[b]) for a, b in fs.PAIRS], axis=0)
    corner = oracle.fast_score_map(img, thr)[3:-3, 3:-3] > 0
    counts = {
        "brighter corner, v < thr": int((corner & brt & (v < thr)).sum()),
        "darker corner, v > 255 - thr": int((corner & dark & (v > 255 - thr)).sum()),
        "refused by equality, v - lo == thr": int((v - lo == thr).sum()),
        "refused by equality, hi - v == thr": int((hi - v == thr).sum()),
        "passed by one, == thr + 1": int(((v - lo == thr + 1) | (hi - v == thr + 1)).sum()),
    }
    print(thr, counts)
    for name, cnt in counts.items():
        assert cnt >= 100, (thr, name, cnt)
