"""The HIP ORB kernels against the independent NumPy model of cv2's ORB stages behind FAST (tests/orb_reference.py), one
stage at a time, each stage fed the kernels' own upstream output, through the C-ABI only: Engine.orb_detect_and_compute,
orb_debug_fetch (pyramid, NMS map, blurred pyramid) and fetch_overflow.  The same rows run on the CPU oracle in
tests/test_orb_reference_cpu.py; tolerances and their derivations: tests/orb_stage_checks.py.  Run with -s for the figures."""
import numpy as np
import pytest

import orb_stage_checks as chk

pytestmark = pytest.mark.gpu


def gpu_run(img, nfeatures):
    from relative_pose_estimation_amd import _capi, geometry
    H, W = img.shape
    e = _capi.Engine(W, H, max_batch=1, nfeatures=nfeatures, max_matches=500)
    try:
        kps, desc, cnt = e.orb_detect_and_compute(img[None])
        pyr, nms, blur = (e.orb_debug_fetch(0, which) for which in (0, 2, 3))
        e.estimate_batch(img[None], img[None], geometry.default_camera_matrix(W, H))    # the flags belong to a batch
        flags = int(e.fetch_overflow(1)[0])
    finally:
        e.close()
    n = int(cnt[0])
    return chk.make_run(img, nfeatures, pyr, nms, blur, kps[0, :n].copy(), desc[0, :n].copy(), flags)


@pytest.mark.parametrize("W,H,nf", chk.SCENES)
def test_scene_stages(W, H, nf):
    run = gpu_run(chk.scene(W, H), nf)
    st = chk.check_all(run, sample=chk.HD_SAMPLE if W * H > 10 ** 6 else None, expect_overflow=chk.scene_overflows(W, H))
    print(f"\nscene {W}x{H}/{nf}: {len(run['kps'])} keypoints {st}")
    assert len(run["kps"]) > 0


@pytest.mark.parametrize("name", list(chk.drawn_images()))
def test_drawn_stages(name):
    img, nf, overflow = chk.drawn_images()[name]
    run = gpu_run(img, nf)
    st = chk.check_all(run, expect_overflow=overflow)
    print(f"\n{name}: {len(run['kps'])} keypoints {st}")
    chk.check_drawn_purpose(name, run, st)
