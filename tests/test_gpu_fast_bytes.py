"""GPU: the byte form of the fused FAST kernel's pair test (four pixels per register, v_lerp_u8 against saturated
thresholds) on the images that sit on its boundaries (tests/fast_bytes.py; tests/test_fast_bytes_cpu.py checks that they
hold every regime): rpe_orb_debug_fetch(which=2) equals the oracle's FAST score -> 3x3 NMS -> border filter on every
pixel of all 12 levels, at thresholds from 1 to 254."""
import numpy as np
import pytest

from tests import fast_bytes as fb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("thr", (1, 15, 120, 254))
def test_fast_nms_boundary_stamps(oracle, thr):
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    img = fb.boundary_stamps(thr)
    e = _capi.Engine(640, 480, max_batch=1, nfeatures=1000, fast_threshold=thr)
    try:
        e.orb_detect_and_compute(img[None])
        L = oracle.orb_layout(640, 480, 1000)
        pyr_o, _ = oracle.build_pyramid(img, 1000)
        nms_g = e.orb_debug_fetch(0, 2)
        off = 0
        for l in range(12):
            w, h = L.w[l], L.h[l]
            nm = oracle.nms_map(oracle.fast_score_map(pyr_o[off:off + w * h].reshape(h, w), thr))
            assert np.array_equal(nm, nms_g[off:off + w * h].reshape(h, w)), (thr, l)
            off += w * h
    finally:
        e.close()
