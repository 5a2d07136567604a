"""GPU: the grouped detection schedule of large ORB batches (csrc/orb_groups.h, run_orb): FAST per group of pyramid levels,
the selection chain of a finished group on a second stream beside FAST of the next.  It is taken from
rpe_orb_group_min_images() images on; smaller extractions launch one kernel after the other.  Every workgroup does the work
it does in the linear schedule, so the two must agree byte for byte:
  detect     n = the threshold, the smallest grouped batch, of 200 x 140 (upper levels shrink to one tile, then to dead
             levels) and of 131 x 127 images (level-0 tiles cut by both far edges): the pattern images of
             tests/test_gpu_fast_lists.py plus seeded noise.  One grouped call against the same images through the same
             handle in chunks below the threshold; the first five of either against the CPU oracle, so that two wrong
             results cannot agree.  The oracle alone first: the noise image has keypoints on three levels or more, so
             every group has something to select.
  X, Y, X    two different image sets alternate on one handle: a missing edge between the streams would leave data of Y
             in the second X.
  poses      17 pairs of 320 x 240 (34 images: grouped) through rpe_enqueue_batch_device against the same pairs in calls of
             16 and 1 (linear, replayed graphs): identical pose records.
  profiling  the stage events stay on the handle's stream: every stage time is >= 0, and their sum, the span from the
             first to the last stage event, fits into the host's time around the call."""
import ctypes
import time

import numpy as np
import pytest

from tests import test_gpu_fast_lists as fl

pytestmark = pytest.mark.gpu

NF = 1000
KP_INT, KP_F32 = ("lx", "ly", "octave"), ("x", "y", "response", "angle")


def _threshold():
    from relative_pose_estimation_amd import _capi
    lib = _capi.load()
    assert lib.rpe_device_count() > 0, "no HIP device visible"
    n = lib.rpe_orb_group_min_images()
    assert 2 * 16 < n <= 34, n          # above every captured batch (16 pairs), and the 17-pair run below is grouped
    return n


def _images(w, h, n):
    """the pattern images of the size (200 x 140: tests/test_gpu_fast_lists.py's five; 131 x 127: its noise image), then noise"""
    if (w, h) == (fl.W, fl.H):
        d = fl.dots()
        head = [fl.noise(), d, 255 - d, fl.last_pass(), np.full((h, w), 77, np.uint8)]
    else:
        head = [fl.noise(w, h, seed=29)]
    return np.stack(head + [fl.noise(w, h, seed=1000 + i) for i in range(n - len(head))])


def _same(a, b):
    """two (kps, desc, counts) results are the same bytes; rows past an image's count are whatever the slot held before"""
    (ka, da, ca), (kb, db, cb) = a, b
    return np.array_equal(ca, cb) and all(ka[i, :c].tobytes() == kb[i, :c].tobytes() and da[i, :c].tobytes() == db[i, :c].tobytes()
                                          for i, c in enumerate(ca))


def _linear(e, imgs, chunk):
    """the images through the handle in calls of at most `chunk`: the linear schedule"""
    parts = [e.orb_detect_and_compute(imgs[i:i + chunk]) for i in range(0, len(imgs), chunk)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


@pytest.mark.parametrize("w,h", [(200, 140), (131, 127)])
def test_grouped_detection_equals_linear_and_oracle(oracle, w, h):
    from relative_pose_estimation_amd import _capi
    n = _threshold()
    imgs = _images(w, h, n)
    n_oracle = 5
    want = [oracle.orb_detect_and_compute(im, NF) for im in imgs[:n_oracle]]
    # the oracle alone: the noise image spreads its keypoints over the levels
    assert len(np.unique(want[0][0]["octave"])) >= 3 and len(want[0][0]) > 100, np.unique(want[0][0]["octave"])
    e = _capi.Engine(w, h, max_batch=(n + 1) // 2, nfeatures=NF)
    try:
        grouped = e.orb_detect_and_compute(imgs)
        linear = _linear(e, imgs, n // 2)                   # three calls, each below the threshold
    finally:
        e.close()
    kg, dg, cg = grouped
    assert np.array_equal(cg, linear[2]), (cg, linear[2])
    assert cg[0] > 100 and _same(grouped, linear)
    for i, (ko, do) in enumerate(want):
        assert cg[i] == len(ko), (i, cg[i], len(ko))
        k = kg[i, :cg[i]]
        for f in KP_INT:
            assert np.array_equal(k[f], ko[f]), (i, f)
        for f in KP_F32:
            assert np.array_equal(k[f].view(np.uint32), ko[f].view(np.uint32)), (i, f)
        assert np.array_equal(dg[i, :cg[i]], do), i


def test_sets_alternating_on_one_handle():
    from relative_pose_estimation_amd import _capi
    n = _threshold()
    X = _images(fl.W, fl.H, n)
    Y = np.stack([fl.noise(seed=5000 + i) for i in range(n)])
    Y[::3] = 255 - X[::3]
    e = _capi.Engine(fl.W, fl.H, max_batch=(n + 1) // 2, nfeatures=NF)
    try:
        x1 = e.orb_detect_and_compute(X)
        y = e.orb_detect_and_compute(Y)
        x2 = e.orb_detect_and_compute(X)
    finally:
        e.close()
    assert not np.array_equal(x1[2], y[2])                   # Y is another workload
    assert x1[2][0] > 100 and _same(x1, x2)


@pytest.fixture(scope="module")
def pairs17():
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(320, 240)
    i1, i2, _, _ = synthetic.make_batch(17, K, 320, 240)
    return K, i1, i2


def test_pose_records_equal_the_linear_calls(pairs17):
    from relative_pose_estimation_amd import _capi
    assert 2 * 17 >= _threshold()
    K, i1, i2 = pairs17
    e = _capi.Engine(320, 240, max_batch=17, nfeatures=NF)
    try:
        a, b = e.upload(i1), e.upload(i2)
        e.enqueue_batch_device(a, b, 17, K)
        grouped = e.fetch_results(17)
        parts = []
        for lo, cnt in ((0, 16), (16, 1)):
            off = lo * 320 * 240
            e.enqueue_batch_device(ctypes.c_void_p(a.value + off), ctypes.c_void_p(b.value + off), cnt, K)
            parts.append(e.fetch_results(cnt))
    finally:
        e.close()
    linear = [np.concatenate([p[k] for p in parts]) for k in range(5)]
    assert (grouped[4] == 0).sum() >= 12, grouped[4]        # the pairs do give poses
    for g, l in zip(grouped, linear):
        assert g.tobytes() == l.tobytes()


def test_stage_times_partition_the_grouped_step(pairs17):
    from relative_pose_estimation_amd import _capi
    K, i1, i2 = pairs17
    e = _capi.Engine(320, 240, max_batch=17, nfeatures=NF)
    try:
        a, b = e.upload(i1), e.upload(i2)
        e.set_profiling(True)
        e.enqueue_batch_device(a, b, 17, K)                 # first call: module load and table uploads stay out of the timing
        e.synchronize()
        t0 = time.perf_counter()
        e.enqueue_batch_device(a, b, 17, K)
        e.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms = e.stage_ms()
    finally:
        e.close()
    assert all(v >= 0. for v in ms.values()), ms
    assert ms["fast"] > 0. and ms["pyramid"] > 0., ms
    assert 0. < sum(ms.values()) <= wall_ms, (ms, wall_ms)
