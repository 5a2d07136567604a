"""Kernels launched with more than 64 KB of dynamic LDS have their limit raised once, in rpe_create, to the most any legal
handle asks: a captured graph, its replay and plain launches of raster_corners_kernel agree whatever other handles ran in
between, handles created in any order compute what fresh ones compute, and the pair-table instance of
match_l2_select_kernel equals the rule instance."""
import numpy as np
import pytest

from tests import reference_rows as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


def _same(a, b):
    """two (R, t, inliers, n_matches, status) five-tuples, bit for bit"""
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y)


def _strip(src, w, h, x0):
    """a w x h image: a column strip of an HD frame, repeated downwards"""
    return np.ascontiguousarray(np.tile(src[:, x0:x0 + w], (-(-h // src.shape[0]), 1))[:h])


def raster_lds_bytes(w, h):
    """rpe_launch_raster_retain's formula at level 0 (the largest level) by build_layout's / build_tables' rules: h + 1 row
    starts, h fill counters, ccap + w / 2 + 64 staged entries, ntile + 1 tile prefixes, 4 bytes each"""
    ccap = min(max(w * h // 64, 1024), 8192)
    ntile = -(-(h - 62) // 64) * -(-(w - 31 - 28) // 64)
    return 4 * (2 * h + 2 + ccap + w // 2 + 64 + ntile)


def test_raster_corners_graph_replay_under_foreign_handles(capi, K_vga):
    """128 x 4095: ccap = 8190, 64 x 2 = 128 FAST tiles, 8192 + 8318 + 128 = 16638 words = 66552 bytes of dynamic LDS, above
    the 65536 default (128 x 4000 stays below with 65016, VGA needs 24864).  A VGA handle is created first and runs before and after the
    tall ones.  The keypoints equal the oracle's; the capture of a device batch, its replay after a VGA handle and a
    128 x 4000 handle have launched the same kernel with their own sizes, and the plain launches of a fresh profiling
    handle give the same five-tuple bit for bit; the VGA handle computes what a fresh VGA handle computes.  Whether the
    first device batch was captured is not observable here: rpe_enqueue_batch_device falls back to plain launches
    silently (RPE_NO_GRAPH, a failed capture), and then "replayed" is a second plain run -- the comparisons still hold,
    the replay is not exercised; that fall-back is outside this test."""
    from oracle import oracle
    from relative_pose_estimation_amd import geometry, synthetic
    W, H = 128, 4095
    assert raster_lds_bytes(W, H) == 66552 and raster_lds_bytes(128, 4000) == 65016 and raster_lds_bytes(640, 480) == 24864
    v1, v2, _, _ = synthetic.make_batch(1, K_vga, cfg=9)
    vga = capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=500)
    vga_first = vga.estimate_batch(v1, v2, K_vga)

    src = rr.load("salah", rows=[3])["img1"][0]
    a, b = _strip(src, W, H, 600), _strip(src, W, H, 604)
    K = geometry.default_camera_matrix(W, H)
    e = capi.Engine(W, H, max_batch=1, nfeatures=4000, max_matches=500)
    kps, desc, cnt = e.orb_detect_and_compute(a[None])
    ko, do, fo = oracle.orb_detect_and_compute(a, 4000, return_flags=True)
    assert cnt[0] == len(ko) >= 100
    kg = kps[0, :cnt[0]]
    assert np.array_equal(kg["lx"], ko["lx"]) and np.array_equal(kg["ly"], ko["ly"]) and np.array_equal(kg["octave"], ko["octave"])
    assert np.array_equal(kg["angle"].view(np.uint32), ko["angle"].view(np.uint32)) and np.array_equal(desc[0, :cnt[0]], do)

    d1, d2 = e.upload(a[None]), e.upload(b[None])
    captured = e.estimate_batch_device(d1, d2, 1, K)
    _same(vga.estimate_batch(v1, v2, K_vga), vga_first)
    other = capi.Engine(W, 4000, max_batch=1, nfeatures=4000, max_matches=500)
    other.estimate_batch(a[None, :4000], b[None, :4000], geometry.default_camera_matrix(W, 4000))
    other.close()
    replayed = e.estimate_batch_device(d1, d2, 1, K)
    e.close()
    fresh = capi.Engine(W, H, max_batch=1, nfeatures=4000, max_matches=500)
    fresh.set_profiling(True)
    plain = fresh.estimate_batch(a[None], b[None], K)
    fresh.close()
    _same(captured, replayed)
    _same(captured, plain)

    _same(vga.estimate_batch(v1, v2, K_vga), vga_first)
    vga.close()
    fresh = capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=500)
    _same(fresh.estimate_batch(v1, v2, K_vga), vga_first)
    fresh.close()


def test_l2_select_pair_table_above_64_kb(capi):
    """match_l2_select_kernel<true>: 96 x 96 frames in the store of an uncapped-SIFT handle (kcap = 16384: 128 KB of sort
    keys whatever the frames hold); the pair list equals the batch over the same pairs (match_l2_select_kernel<false>) bit
    for bit"""
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(96, 96)
    frames = synthetic.make_stream(3, K, 96, 96, seed=11, step=0.02)[0]
    e = capi.Engine(96, 96, max_batch=2, nfeatures=0, max_matches=500, feature_method=capi.FEATURE_SIFT, norm_type=capi.NORM_L2)
    assert e.kcap == capi.SIFT_UNCAPPED_CAPACITY + 64 and 8 * e.kcap == 131072
    batch = e.estimate_batch(frames[:2], frames[1:], K)
    assert batch[3].sum() > 0, batch
    e.frames_reserve(3)
    e.frames_put(frames[:2], [0, 1])
    e.frames_put(frames[2:], [2])
    _same(e.estimate_pairs([0, 1], [1, 2], K), batch)
    e.close()
