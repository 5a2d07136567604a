"""The CPU oracle's SIFT (oracle/sift_oracle.c) against the independent float64 model of cv2's SIFT
(tests/sift_reference.py), one stage at a time -- each stage fed the oracle's own upstream output.  The oracle and the
HIP kernels share their conventions bit for bit (tests/test_gpu_parity.py), so these rows pin both against cv2's
algorithm; tests/test_gpu_sift_reference.py runs the same rows on the kernels.  Tolerances: tests/sift_stage_checks.py."""
import numpy as np
import pytest

import sift_reference as ref
import sift_stage_checks as chk

SIZES = [(320, 240), (211, 157)]


def _frame(W, H, cfg=6):
    from relative_pose_estimation_amd import synthetic, geometry
    i1, _, _, _ = synthetic.make_batch(1, geometry.default_camera_matrix(W, H), W, H, cfg=cfg)
    return i1[0]


@pytest.fixture(scope="module")
def runs(oracle):
    """image -> (pyramid, uncapped keypoints, descriptors), computed once per module"""
    cache = {}

    def get(name, img):
        if name not in cache:
            H, W = img.shape
            flat, _ = oracle.sift_gauss_pyramid(img)
            k, d = oracle.sift_detect_and_compute(img, 0)
            cache[name] = (ref.split_pyramid(flat, W, H), k, d)
        return cache[name]
    return get


def _inputs():
    out = [(f"cfg6_{W}x{H}", (W, H)) for W, H in SIZES]
    out += [(f"drawn_{n}", n) for n in chk.drawn_images()]
    return out


def _image(spec):
    if isinstance(spec, tuple):
        return _frame(*spec)
    return chk.drawn_images()[spec]


CASES = _inputs()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_gaussian_levels(runs, name, spec):
    img = _image(spec)
    pyr, _, _ = runs(name, img)
    err = chk.check_pyramid(img, pyr)
    print(f"{name}: pyramid max |err| {err:.3g}")


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_refined_keypoints(runs, name, spec):
    img = _image(spec)
    pyr, k, _ = runs(name, img)
    st = chk.check_keypoints(pyr, k)
    print(f"{name}: {st}")
    if name == "drawn_flat":
        assert len(k) == 0 and st["n_model"] == 0
    if name == "drawn_large_blob":                      # found in the deep octaves only
        assert len(k) and np.all(ref.locate(k)[0] >= 3)


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_orientations(runs, name, spec):
    img = _image(spec)
    pyr, k, _ = runs(name, img)
    st = chk.check_orientations(pyr, k)
    print(f"{name}: {st}")


def test_orientation_wraps_at_zero(runs):
    """the drawn 'wrap' blobs put angles on both sides of 0 / 360 degrees, and the model's 360 -> 0 rule holds there"""
    img = chk.drawn_images()["wrap_blobs"]
    pyr, k, _ = runs("drawn_wrap_blobs", img)
    a = k["angle"]
    assert np.all((a >= 0) & (a < 360))
    near = np.minimum(a, 360 - a) < 12
    assert near.sum() >= 2, np.sort(a)
    chk.check_orientations(pyr, k[near])


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_descriptors(runs, name, spec):
    img = _image(spec)
    pyr, k, d = runs(name, img)
    st = chk.check_descriptors(pyr, k, d)
    print(f"{name}: {st}")


@pytest.mark.parametrize("nfeatures", [0, 150, 300])
def test_post_processing_and_order(oracle, runs, nfeatures):
    """removeDuplicatedSorted + retainBest + rescale: the same set as the model; without a cap the same order.  Under a
    cap the oracle's default order is sorted (the HIP path's documented convention), and its cv2_order switch gives the
    model's order -- cv2's, through the real std::nth_element -- for both C++ runtimes."""
    img = _frame(320, 240)
    _, k, _ = runs("cfg6_320x240", img)
    capped, _ = oracle.sift_detect_and_compute(img, nfeatures)
    m = chk.check_post(k, capped, nfeatures)
    if 0 < nfeatures < len(k):
        assert not chk.same_records(m, capped.astype(ref.KP_DTYPE))     # the two orders really differ here
    pre = ref.unscale_first_octave(k)
    for rt in ("libstdc++", "msvc"):
        c2, _ = oracle.sift_detect_and_compute(img, nfeatures, cv2_order=rt)
        assert chk.same_records(c2.astype(ref.KP_DTYPE), ref.post_process(pre, nfeatures, rt)), rt


def test_cap_2048_on_a_textured_frame(oracle):
    """a 960x540 textured frame holds more than 2048 keypoints: the cap bites, set and order as above"""
    img = _frame(960, 540, cfg=5)
    k, _ = oracle.sift_detect_and_compute(img, 0)
    assert len(k) > 2048
    capped, _ = oracle.sift_detect_and_compute(img, 2048)
    chk.check_post(k, capped, 2048)
    c2, _ = oracle.sift_detect_and_compute(img, 2048, cv2_order="libstdc++")
    assert chk.same_records(c2.astype(ref.KP_DTYPE), ref.post_process(ref.unscale_first_octave(k), 2048))
