"""orient_describe_kernel after the row-paired horizontal blur pass and the wave-uniform keypoint record: keypoints, angles
(exact f32) and descriptors of Engine.orb_detect_and_compute equal oracle.orb_detect_and_compute bit for bit.

The image is a seeded texture (random blocks of 16, 32 and 64 px plus a little noise against tied scores), chosen on the CPU
so that the oracle's keypoints cover what the kernel's addressing depends on; the choice is asserted on the oracle's output:
  * all four values of (x - 22) & 3, the byte phase of the patch rows against their aligned dword loads, on >= 3 levels;
  * patches that touch the first and the last usable rows / columns of a level (x or y = 31, x = w - 32 or y = h - 32),
    the extremes of the 32-bit patch offsets;
  * keypoints on the smallest level.
(a) the 256 x 192 image, nfeatures 300; (b) a batch of three: the image, a constant grey image (no keypoints: every
workgroup leaves at the count test, through the scalar loads) and the image again; (c) the same texture at 640 x 480 with
nfeatures 1000, the workload's grid and XCD mapping."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 4


def _textured(W, H):
    rng = np.random.default_rng(SEED)
    img = np.zeros((H, W), np.float64)
    for b in (16, 32, 64):
        img += np.kron(rng.integers(0, 256, (-(-H // b), -(-W // b))), np.ones((b, b)))[:H, :W]
    return (img * (0.95 / 3) + rng.integers(0, 13, (H, W))).astype(np.uint8)


@pytest.fixture(scope="module")
def small(oracle):
    img = _textured(256, 192)
    kps, desc, flags = oracle.orb_detect_and_compute(img, 300, return_flags=True)
    assert flags == 0
    return img, kps, desc


def _same(kg, dg, ko, do):
    assert len(kg) == len(ko), (len(kg), len(ko))
    for f in ("lx", "ly", "octave"):
        assert np.array_equal(kg[f], ko[f]), f
    for f in ("x", "y", "response", "angle"):
        assert np.array_equal(kg[f].view(np.uint32), ko[f].view(np.uint32)), f"{f} not bit-identical"
    bad = np.flatnonzero((dg != do).any(axis=1))
    assert bad.size == 0, f"{bad.size} descriptors differ, first: keypoint {bad[:1]} {ko[bad[:1]]}"


def _run(imgs, W, H, nfeatures):
    from relative_pose_estimation_amd import _capi
    e = _capi.Engine(W, H, max_batch=2, nfeatures=nfeatures, max_matches=500)
    try:
        return e.orb_detect_and_compute(imgs)
    finally:
        e.close()


def _covers(oracle, kps, W, H, nfeatures):
    L = oracle.orb_layout(W, H, nfeatures)
    lv = kps["octave"]
    w = np.array(list(L.w))[lv]
    h = np.array(list(L.h))[lv]
    phases = sum(1 for l in range(12) if len(set(((kps["lx"][lv == l] - 22) & 3).tolist())) == 4)
    first = bool(np.any((kps["lx"] == 31) | (kps["ly"] == 31)))
    last = bool(np.any((kps["lx"] == w - 32) | (kps["ly"] == h - 32)))
    return phases, first, last, int(np.sum(lv == 11))


def test_small_image(oracle, small):
    img, ko, do = small
    phases, first, last, top = _covers(oracle, ko, 256, 192, 300)
    assert phases >= 3 and first and last and top > 0, (phases, first, last, top)
    kps, desc, cnt = _run(img[None], 256, 192, 300)
    _same(kps[0, :cnt[0]], desc[0, :cnt[0]], ko, do)


def test_batch_with_an_empty_image(oracle, small):
    img, ko, do = small
    grey = np.full_like(img, 128)
    assert len(oracle.orb_detect_and_compute(grey, 300)[0]) == 0
    kps, desc, cnt = _run(np.stack([img, grey, img]), 256, 192, 300)
    assert cnt[1] == 0
    assert cnt[0] == cnt[2] and np.array_equal(kps[0], kps[2]) and np.array_equal(desc[0], desc[2])
    _same(kps[0, :cnt[0]], desc[0, :cnt[0]], ko, do)
    _same(kps[2, :cnt[2]], desc[2, :cnt[2]], ko, do)


def test_vga_image(oracle):
    img = _textured(640, 480)
    ko, do, flags = oracle.orb_detect_and_compute(img, 1000, return_flags=True)
    assert flags == 0 and len(ko) == 1000
    phases, first, last, top = _covers(oracle, ko, 640, 480, 1000)
    assert phases >= 3 and first and last and top > 0, (phases, first, last, top)
    kps, desc, cnt = _run(img[None], 640, 480, 1000)
    _same(kps[0, :cnt[0]], desc[0, :cnt[0]], ko, do)
