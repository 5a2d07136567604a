"""CPU: the FAST kernel's one-sided score (tests/fast_sides.py) equals the oracle's full cornerScore map on every pixel
of every pyramid level, for synthetic scenes and for the images that exercise each side path; and those images do
reach every path (darker-only, brighter-only, both sides, candidates that are not corners, dense tiles)."""
import numpy as np

from tests import fast_sides as fs


def _levels(oracle, img):
    pyr, L = oracle.build_pyramid(img, 1000)
    off = 0
    for l in range(12):
        w, h = L.w[l], L.h[l]
        yield l, pyr[off:off + w * h].reshape(h, w)
        off += w * h


def test_one_sided_score_equals_full_score(oracle, K_vga):
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_pair(7, K_vga)
    for img in [i1, i2] + list(fs.side_images()):
        for l, lvl in _levels(oracle, img):
            assert np.array_equal(fs.one_sided_score_map(lvl), oracle.fast_score_map(lvl, 15)), l


def test_side_images_reach_every_path(oracle):
    imgs = fs.side_images()
    n_dark = n_brt = n_both = n_cand_not_corner = 0
    dense_cand = dense_corner = 0
    for img in imgs:
        v, r = fs.ring(img)
        dark, brt = fs.sides(v, r)
        sc = oracle.fast_score_map(img, 15)[3:-3, 3:-3]
        n_dark += int((dark & ~brt).sum()); n_brt += int((brt & ~dark).sum()); n_both += int((dark & brt).sum())
        n_cand_not_corner += int(((dark | brt) & (sc == 0)).sum())
        # one kernel tile: 64 x 64 outputs, scores on 66 x 66 around them (level 0 tiles start at x, y = 31 + 64 k)
        for ty in range(31, 480 - 31 - 64, 64):
            for tx in range(31, 640 - 31 - 64, 64):
                y, x = ty - 1 - 3, tx - 1 - 3
                dense_cand = max(dense_cand, int((dark | brt)[y:y + 66, x:x + 66].sum()))
                dense_corner = max(dense_corner, int((sc[y:y + 66, x:x + 66] > 0).sum()))
    assert n_dark > 1000 and n_brt > 1000 and n_both > 1000 and n_cand_not_corner > 1000
    assert dense_cand > 1024 and dense_corner > 256
