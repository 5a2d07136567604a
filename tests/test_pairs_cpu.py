"""Frame store / pair lists, the parts that need no GPU: the chunk planner of PoseEstimator.estimate_pairs, the NULL-handle
refusals of the new C-ABI entry points, and the argument validation that runs before any device call."""
import ctypes as C

import numpy as np
import pytest

from relative_pose_estimation_amd import PoseEstimator, _capi, plan_pairs
from relative_pose_estimation_amd.geometry import default_camera_matrix


@pytest.mark.parametrize("F,P,mb", [(8, 21, 24), (8, 21, 4), (9, 24, 4), (1, 1, 1), (256, 1014, 64), (17, 0, 4), (5, 3, 1)])
def test_plan_covers_everything_once_within_limits(F, P, mb):
    puts, runs = plan_pairs(F, P, mb)
    frames = [f for a, b in puts for f in range(a, b)]
    assert frames == list(range(F)), "every frame put exactly once, in order"
    assert all(0 < b - a <= 2 * mb for a, b in puts)
    pairs = [p for a, b in runs for p in range(a, b)]
    assert pairs == list(range(P)), "every pair run exactly once, in order"
    assert all(0 < b - a <= mb for a, b in runs)


def test_plan_window_list_puts_each_frame_once():
    """window 4 over 256 frames: 1014 pairs, 256 extractions (the batch form needs 2028), the fewest calls the limits allow"""
    F, k, mb = 256, 4, 64
    P = sum(F - d for d in range(1, k + 1))
    assert P == 1014
    puts, runs = plan_pairs(F, P, mb)
    assert sum(b - a for a, b in puts) == F
    assert len(puts) == -(-F // (2 * mb)) and len(runs) == -(-P // mb)


def test_plan_rejects_nonsense():
    for bad in [(0, 1, 1), (4, -1, 1), (4, 1, 0)]:
        with pytest.raises(ValueError):
            plan_pairs(*bad)


def test_new_entry_points_refuse_a_null_handle():
    lib = _capi.load()
    one = np.zeros(1, np.int32)
    K = np.eye(3)
    img = np.zeros((96, 96), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rpe_frames_reserve(None, 4) == -1
    assert lib.rpe_frames_capacity(None) == 0
    assert lib.rpe_frames_put(None, p(img), 1, p(one)) == -1
    assert lib.rpe_frames_put_device(None, p(img), 1, p(one)) == -1
    assert lib.rpe_frames_info(None, 1, p(one), p(one), None) == -1
    assert lib.rpe_enqueue_pairs(None, p(one), p(one), 1, p(K)) == -1
    out = np.zeros(16)
    assert lib.rpe_estimate_pairs(None, p(one), p(one), 1, p(K), p(out), p(out), p(one), p(one), p(one)) == -1


def test_exports_name_the_new_calls():
    for n in ["rpe_frames_reserve", "rpe_frames_capacity", "rpe_frames_put", "rpe_frames_put_device", "rpe_frames_info",
              "rpe_enqueue_pairs", "rpe_estimate_pairs"]:
        assert n in _capi.EXPORTS
        getattr(_capi.load(), n)


@pytest.fixture()
def pe(monkeypatch):
    est = PoseEstimator(default_camera_matrix(640, 480), nfeatures=1000, max_batch=4)

    def no_device(*a, **k):
        raise AssertionError("validation must fail before an engine is created")
    monkeypatch.setattr(est, "_engine", no_device)
    return est


@pytest.mark.parametrize("pairs", [[[0, 4]], [[-1, 0]], [[0, 1], [2, 7]], [0, 1], [[0, 1, 2]], np.zeros((0, 2), np.int32),
                                   [[0.0, 1.0]], [[[0, 1]]]])
def test_estimate_pairs_validates_the_pair_list(pe, pairs):
    frames = np.zeros((4, 480, 640), np.uint8)
    with pytest.raises(ValueError):
        pe.estimate_pairs(frames, pairs)


@pytest.mark.parametrize("frames", [np.zeros((480, 640), np.uint8), np.zeros((4, 480, 640), np.float32),
                                    np.zeros((4, 480, 640, 4), np.uint8), np.zeros((0, 480, 640), np.uint8)])
def test_estimate_pairs_validates_the_frames(pe, frames):
    with pytest.raises(ValueError):
        pe.estimate_pairs(frames, [[0, 0]])


def test_frame_store_validates_before_any_device_call(pe):
    with pytest.raises(ValueError):
        pe.frame_store(0)
    fs = pe.frame_store(4)
    img = np.zeros((480, 640), np.uint8)
    for slots, imgs in [([4], img[None]), ([-1], img[None]), ([1, 1], np.stack([img, img])), ([0, 1], img[None]),
                        ([0], img[None].astype(np.float32)), ([0.5], img[None])]:
        with pytest.raises(ValueError):
            fs.put_many(slots, imgs)
    with pytest.raises(ValueError):
        fs.estimate([[0, 4]])
    with pytest.raises(ValueError):
        fs.info([4])
    cnt, fl = fs.info([0, 3])                 # nothing put yet: every slot is empty, and no engine was needed to say so
    assert list(cnt) == [-1, -1] and list(fl) == [0, 0]
    fs.close()
