"""Images whose SIFT keypoints tie in response, for the thresholds of the HIP path's three radix selects (select,
prefilter, finalize) and finalize's ordered compaction.  A grid of identical Gaussian blobs gives identical keypoints up to
a translation, hence identical responses; rows of the grid alternate between two amplitudes.

The counts below are the CPU oracle's (tests/test_sift_tie_cases_cpu.py asserts them); capacity = nfeatures + 64."""
import numpy as np

W, H = 320, 240
TWO_AMPLITUDES = (90, 60)       # 80 keypoints, two distinct responses: 48 strong, 32 weak
ONE_AMPLITUDE = (90, 90)        # 80 keypoints, one response
OVF_SIFT_CAP, OVF_SIFT_KEYPOINTS = 1 << 7, 1 << 8
# (amplitudes, nfeatures) -> (keypoints kept, overflow flags).  retainBest keeps every tie of the nfeatures-th response.
EXPECTED = {
    (TWO_AMPLITUDES, 5): (48, OVF_SIFT_CAP),
    (TWO_AMPLITUDES, 48): (48, OVF_SIFT_CAP),
    (TWO_AMPLITUDES, 49): (80, OVF_SIFT_CAP),
    (ONE_AMPLITUDE, 16): (80, OVF_SIFT_CAP),                          # exactly the capacity of 80
    (ONE_AMPLITUDE, 5): (69, OVF_SIFT_CAP | OVF_SIFT_KEYPOINTS),      # the first 69 of the 80
}
# the prefilter's radix branch needs more raw keypoints than 2 * nfeatures + 1024: a 640x480 cfg-6 frame holds 1749
PREFILTER_FRAME = dict(W=640, H=480, cfg=6, nfeatures=8, uncapped=1749)


def blob_grid(amplitudes):
    """320x240 u8, base 110: blobs exp(-(dx^2 / (2 2.0^2) + dy^2 / (2 3.0^2))) on a 32-px grid from (48, 48), 40 px
    clear of the far edges; grid row j has amplitude amplitudes[j & 1]"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W), 110.0)
    for j, cy in enumerate(range(48, H - 40 + 1, 32)):
        for cx in range(48, W - 40 + 1, 32):
            img += amplitudes[j & 1] * np.exp(-((x - cx) ** 2 / (2 * 2.0 ** 2) + (y - cy) ** 2 / (2 * 3.0 ** 2)))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def prefilter_frame():
    from relative_pose_estimation_amd import synthetic, geometry
    f = PREFILTER_FRAME
    i1, _, _, _ = synthetic.make_batch(1, geometry.default_camera_matrix(f["W"], f["H"]), f["W"], f["H"], cfg=f["cfg"])
    return i1[0]


def assert_equal_to_oracle(kg, dg, flags_g, ko, do, flags_o):
    """count, the bits of every keypoint field, descriptors and overflow flags"""
    assert len(kg) == len(ko), (len(kg), len(ko))
    for f in ("x", "y", "size", "angle", "response"):
        assert np.array_equal(kg[f].view(np.uint32), ko[f].view(np.uint32)), f
    assert np.array_equal(kg["octave"], ko["octave"])
    assert np.array_equal(dg, do)
    assert flags_g == flags_o, (flags_g, flags_o)
