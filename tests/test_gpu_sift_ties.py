"""The thresholds of the HIP SIFT path's radix selects where keys tie, and the prefilter's radix branch, which no small
frame reaches: GPU == oracle in count, every keypoint field's bits, descriptors and overflow flags.  Images and the oracle's
counts: tests/sift_tie_cases.py (asserted without a GPU in tests/test_sift_tie_cases_cpu.py)."""
import numpy as np
import pytest

import sift_tie_cases as tie

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


def _gpu_equals_oracle(capi, oracle, monkeypatch, img, nfeatures, sel_k):
    """RPE_SIFT_SEL_K is read when the engine is created"""
    H, W = img.shape
    if sel_k:
        monkeypatch.setenv("RPE_SIFT_SEL_K", str(sel_k))
    e = capi.Engine(W, H, max_batch=1, nfeatures=nfeatures, max_matches=200, feature_method=capi.FEATURE_SIFT, norm_type=capi.NORM_L2)
    if sel_k:
        monkeypatch.delenv("RPE_SIFT_SEL_K")
    try:
        kps, desc, cnt = e.sift_detect_and_compute(img[None])
        from relative_pose_estimation_amd import geometry
        e.estimate_batch(img[None], img[None], geometry.default_camera_matrix(W, H))      # flags are a whole run's: the image as both sides
        flags = int(e.fetch_overflow(1)[0])
        ko, do, fo = oracle.sift_detect_and_compute(img, nfeatures, cap=e.kcap, return_flags=True)
        tie.assert_equal_to_oracle(kps[0, :cnt[0]], desc[0, :cnt[0]], flags, ko, do, fo)
        return len(ko), fo
    finally:
        e.close()


@pytest.mark.parametrize("sel_k", [0, 10])
@pytest.mark.parametrize("nfeatures", [5, 48, 49])
def test_ties_at_every_threshold(capi, oracle, monkeypatch, nfeatures, sel_k):
    """48 strong and 32 weak keypoints.  sel_k = 0: the default selection (nfeatures * 5/4 + 256 >= all 80 survivors, nothing
    is cut).  RPE_SIFT_SEL_K = 10: select's threshold falls on the strong tie group, which it must keep whole; at nfeatures =
    48 those fill the cap, at 49 they do not (nuniq < nfeatures), so the second round orients every survivor and finalize's
    threshold falls on the weak group: all 80."""
    count, flags = _gpu_equals_oracle(capi, oracle, monkeypatch, tie.blob_grid(tie.TWO_AMPLITUDES), nfeatures, sel_k)
    assert (count, flags) == tie.EXPECTED[(tie.TWO_AMPLITUDES, nfeatures)]


@pytest.mark.parametrize("nfeatures", [16, 5])
def test_one_tie_group_at_and_over_capacity(capi, oracle, monkeypatch, nfeatures):
    """80 keypoints of one response: finalize's ordered compaction fills the capacity exactly (nfeatures = 16: 80 slots) and
    cuts the sorted list at it (nfeatures = 5: the first 69, RPE_OVF_SIFT_KEYPOINTS)"""
    count, flags = _gpu_equals_oracle(capi, oracle, monkeypatch, tie.blob_grid(tie.ONE_AMPLITUDE), nfeatures, 0)
    assert (count, flags) == tie.EXPECTED[(tie.ONE_AMPLITUDE, nfeatures)]


def test_prefilter_radix_branch(capi, oracle, monkeypatch):
    """nfeatures = 8 with RPE_SIFT_SEL_K = 100000: every survivor of the 640x480 frame is oriented, so the raw list is
    longer than the K = 2 * 8 + 1024 entries the prefilter lets through and its radix select runs"""
    f = tie.PREFILTER_FRAME
    img = tie.prefilter_frame()
    ku, _ = oracle.sift_detect_and_compute(img, 0)
    assert len(ku) > 2 * f["nfeatures"] + 1024
    _gpu_equals_oracle(capi, oracle, monkeypatch, img, f["nfeatures"], 100000)
