"""retain_fast_kernel's two launches share the level lists by length: up to RPE_RETAIN_TIER = 2048 corners the small-LDS
launch, above it the long-list launch, whose workgroups walk over the images.  Dot grids put level 0 (and level 1) of an
image exactly AT the tier (2048 corners, the last list of the first launch) and one corner above it (2049, the shortest
list of the second); both replay retainBest (2 x quota is far below).  600 images, more than the 512 rows of the long-list
grid, so that a workgroup walks two images: the long lists sit in its first image, in its second, and in both.
Keypoints in cv2's order, descriptors and counts equal the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIER = 2048
N_IMG, GRID_Y = 600, 512           # rpe_launch_raster_retain: dim3(nlev_big, min(n_img, 512))


def _dots(extra):
    d = np.full((480, 640), 40, np.uint8)
    d[40:40 + 8 * 32:8, 40:40 + 8 * 64:8] = 220               # 32 x 64 dots: one FAST corner each
    if extra:
        d[400, 100] = 220
    return d


def _level_counts(oracle, img):
    L = oracle.orb_layout(640, 480, 1000)
    pyr, _ = oracle.build_pyramid(img, 1000)
    out, off = [], 0
    for l in range(12):
        w, h = L.w[l], L.h[l]
        out.append(int((oracle.nms_map(oracle.fast_score_map(pyr[off:off + w * h].reshape(h, w), 15)) > 0).sum()))
        off += w * h
    return out, L


def test_lists_at_and_above_the_tier(oracle, K_vga):
    from relative_pose_estimation_amd import _capi, synthetic
    plain = synthetic.make_batch(1, K_vga, cfg=3)[0][0]
    at, above = _dots(False), _dots(True)
    ca, L = _level_counts(oracle, at)
    cb, _ = _level_counts(oracle, above)
    assert ca[0] == ca[1] == TIER and cb[0] == cb[1] == TIER + 1, (ca, cb)
    assert TIER > 2 * L.quota[0] and 640 * 480 // 64 > TIER + 1       # retainBest runs on both; the raster list holds both
    kinds = {0: plain, 1: at, 2: above}
    which = np.zeros(N_IMG, np.int64)
    # workgroup y of the long-list launch walks images y and y + 512
    which[5] = 2; which[5 + GRID_Y] = 2                        # both images of a workgroup
    which[20] = 2; which[20 + GRID_Y] = 1                      # the first only; the other stops at the tier
    which[30 + GRID_Y] = 2                                     # the second only
    which[40] = 1; which[GRID_Y - 1] = 2; which[N_IMG - 1] = 2  # the last row of the grid, the last image
    imgs = np.stack([kinds[k] for k in which])
    e = _capi.Engine(640, 480, max_batch=N_IMG // 2, nfeatures=1000, max_matches=500)
    try:
        kps, desc, cnt = e.orb_detect_and_compute(imgs)
    finally:
        e.close()
    want = {k: oracle.orb_detect_and_compute(img, 1000) for k, img in kinds.items()}
    assert all(len(w[0]) > 500 for w in want.values())
    for n in range(N_IMG):
        ko, do = want[int(which[n])]
        assert cnt[n] == len(ko), (n, which[n], cnt[n], len(ko))
        kg = kps[n, :cnt[n]]
        assert np.array_equal(kg["lx"], ko["lx"]) and np.array_equal(kg["ly"], ko["ly"]) and np.array_equal(kg["octave"], ko["octave"]), (n, which[n])
        assert np.array_equal(desc[n, :cnt[n]], do), (n, which[n])
