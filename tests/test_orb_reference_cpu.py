"""The CPU oracle's ORB (oracle/orb_oracle.c) against the independent NumPy model of cv2's ORB stages behind FAST
(tests/orb_reference.py), one stage at a time, each stage fed the oracle's own upstream output.  The oracle and the HIP
kernels agree bit for bit (tests/test_gpu_parity.py), so these rows pin both; tests/test_gpu_orb_reference.py runs the
same rows on the kernels.  Tolerances and their derivations: tests/orb_stage_checks.py.  Run with -s for the figures."""
import numpy as np
import pytest

import orb_reference as ref
import orb_stage_checks as chk


def oracle_run(oracle, img, nfeatures):
    pyr, L = oracle.build_pyramid(img, nfeatures)
    layout = (list(L.scale), list(L.w), list(L.h), list(L.quota))
    nms = np.zeros_like(pyr); blur = np.zeros_like(pyr)
    for l in range(ref.NLEVELS):
        off, w, h = L.offset[l], L.w[l], L.h[l]
        lv = pyr[off:off + w * h].reshape(h, w)
        nms[off:off + w * h] = oracle.nms_map(oracle.fast_score_map(lv, ref.FAST_THRESHOLD)).ravel()
        blur[off:off + w * h] = oracle.blur_level(lv).ravel()
    kps, desc, flags = oracle.orb_detect_and_compute(img, nfeatures, return_flags=True)
    return chk.make_run(img, nfeatures, pyr, nms, blur, kps, desc, flags, layout)


@pytest.fixture(scope="module")
def runs(oracle):
    cache = {}

    def get(name, img, nfeatures):
        if name not in cache:
            cache[name] = oracle_run(oracle, img, nfeatures)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------ the model's own rows
def test_model_patch_disc():
    d = ref.patch_disc()
    assert d.shape == (31, 31) and d.sum() == 749
    assert np.array_equal(d, d.T) and np.array_equal(d, d[::-1, ::-1])
    assert ((d.sum(axis=1) - 1) // 2)[15:].tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    u = np.arange(-15, 16)
    r2 = u[:, None] ** 2 + u[None, :] ** 2
    assert d[r2 <= 14.5 ** 2].all() and not d[r2 > 15.5 ** 2].any()          # a disc of radius 15 to within half a pixel


def test_model_basics():
    scale, w, h, quota = ref.layout(640, 480, 1000)
    assert (w[0], h[0]) == (640, 480) and quota.sum() == 1000 and np.all(np.diff(quota[:-1]) <= 0)
    assert abs(float(scale[11]) - 1.1 ** 11) < 1e-5 and (w[1], h[1]) == (582, 436)
    assert abs(ref.gauss_taps().sum() - 1) < 1e-15
    flat = np.full((50, 70), 93, np.uint8)
    assert np.allclose(ref.blur(flat), 93, atol=1e-12) and np.allclose(ref.resize_linear(flat, 64, 45)[0], 93, atol=1e-12)
    ramp = np.tile(np.arange(70, dtype=np.uint8) * 3, (50, 1))                 # a ramp: Ix = 8 * 3, Iy = 0
    r, m, a, b, c = ref.harris_at(ramp, [30], [25])
    assert (a[0], b[0], c[0]) == (49 * 24 * 24, 0, 0) and r[0] < 0
    m01, m10 = ref.moments(ramp, [30], [25])
    assert m01[0] == 0 and m10[0] == 3 * int((ref.patch_disc() * np.arange(-15, 16)[None, :] ** 2).sum())
    assert ref.angle_deg(m01, m10)[0] == 0 and ref.angle_deg(np.array([-1]), np.array([0]))[0] == 270
    img = np.arange(64 * 64, dtype=np.int64).reshape(64, 64) % 251
    bits, margin = ref.descriptor_bits(img.astype(np.uint8), [32], [32], [0.0])
    p = ref.load_pattern()
    assert np.array_equal(bits[0], (img[32 + p[:, 1], 32 + p[:, 0]] < img[32 + p[:, 3], 32 + p[:, 2]]).astype(np.uint8))
    assert np.all(margin == 0.5) and np.array_equal(ref.unpack_bits(ref.pack_bits(bits)), bits)
    assert ref.keep_by_score(np.array([5, 7, 7, 3, 9]), 2).tolist() == [False, True, True, False, True]   # ties kept


# ------------------------------------------------------------------------------------------ the oracle against the model
@pytest.mark.parametrize("W,H,nf", chk.SCENES)
def test_scene_stages(runs, W, H, nf):
    run = runs(f"scene_{W}x{H}_{nf}", chk.scene(W, H), nf)
    st = chk.check_all(run, sample=chk.HD_SAMPLE if W * H > 10 ** 6 else None, expect_overflow=chk.scene_overflows(W, H))
    print(f"\nscene {W}x{H}/{nf}: {len(run['kps'])} keypoints {st}")
    assert len(run["kps"]) > 0


DRAWN = list(chk.drawn_images())


@pytest.mark.parametrize("name", DRAWN)
def test_drawn_stages(runs, name):
    img, nf, overflow = chk.drawn_images()[name]
    run = runs(name, img, nf)
    st = chk.check_all(run, expect_overflow=overflow)
    print(f"\n{name}: {len(run['kps'])} keypoints {st}")
    chk.check_drawn_purpose(name, run, st)


# ------------------------------------------------------------------------------------------ sensitivity
def _raises(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def test_checks_catch_subtle_damage(oracle, runs):
    """one oracle result, damaged the way a subtly wrong kernel would be: every damage is caught by its check"""
    W, H, nf = 640, 480, 1000
    img = chk.scene(W, H)
    good = runs(f"scene_{W}x{H}_{nf}", img, nf)
    chk.check_all(good)

    def damaged(**kw):
        r = dict(good)
        r.update(kw)
        return r
    k = good["kps"]
    # an angle shifted by 0.05 degrees
    k2 = k.copy(); k2["angle"] = (k2["angle"] + np.float32(0.05)) % np.float32(360)
    assert _raises(chk.check_keypoint_fields, damaged(kps=k2))
    k2 = k.copy(); k2["angle"][len(k) // 2] += np.float32(0.05)
    assert _raises(chk.check_keypoint_fields, damaged(kps=k2))
    # the response scaled by 1 + 1e-5 on the keypoints where it does not cancel
    resp = np.concatenate([ref.harris_at(good["pyr"][l], k["lx"][k["octave"] == l], k["ly"][k["octave"] == l])[:2]
                           for l in range(ref.NLEVELS) if np.any(k["octave"] == l)], axis=1)
    plain = np.abs(resp[0]) > 0.5 * resp[1]
    assert plain.sum() > 50
    k2 = k.copy(); k2["response"][plain] *= np.float32(1 + 1e-5)
    assert _raises(chk.check_keypoint_fields, damaged(kps=k2))
    k2 = k.copy(); j = np.nonzero(plain)[0][0]; k2["response"][j] *= np.float32(1 + 1e-5)
    assert _raises(chk.check_keypoint_fields, damaged(kps=k2))
    # one pyramid level shifted by a pixel
    pyr = list(good["pyr"]); pyr[3] = np.roll(pyr[3], 1, axis=1)
    assert _raises(chk.check_pyramid, damaged(pyr=pyr))
    # the blur with cvRound(256 g) taps [18, 34, 49, 55, ...] / 257
    try:
        oracle.set_variant(0, 0)
        bl = [oracle.blur_level(lv) for lv in good["pyr"]]
    finally:
        oracle.set_variant(0, 3)
    assert not np.array_equal(bl[0], good["blur"][0]) and _raises(chk.check_blur, damaged(blur=bl))
    # 2 % of the keypoints with one descriptor bit flipped
    rng = np.random.default_rng(5)
    d2 = good["desc"].copy()
    for i in rng.choice(len(k), len(k) // 50, replace=False):
        d2[i, rng.integers(32)] ^= np.uint8(1 << rng.integers(8))
    assert _raises(chk.check_descriptors, damaged(desc=d2))
    d2 = good["desc"].copy(); d2[7, 3] ^= np.uint8(16)
    bits, margin = ref.descriptor_bits(good["blur"][int(k["octave"][7])], k["lx"][7:8], k["ly"][7:8], k["angle"][7:8])
    assert margin[0, 3 * 8 + 4] >= chk.DESC_MARGIN and _raises(chk.check_descriptors, damaged(desc=d2))
    # one kept keypoint swapped for the best rejected candidate of its level
    l = 0
    _, _, sel = chk.model_selection(good, l)
    assert len(sel["x"]) > good["quota"][l]
    rej = np.nonzero(~sel["keep"])[0]
    best = rej[np.argmax(sel["resp"][rej])]
    k2 = k.copy()
    j = np.nonzero(k["octave"] == l)[0][np.argmax(k["response"][k["octave"] == l])]
    k2["lx"][j], k2["ly"][j] = sel["x"][best], sel["y"][best]
    assert _raises(chk.check_selection, damaged(kps=k2))
    # the quota of two levels exchanged
    q = good["quota"].copy(); q[[2, 5]] = q[[5, 2]]
    assert _raises(chk.check_selection, good, quota=q)
    s_, w_, h_, q_ = good["layout"]
    q_ = list(q_); q_[2], q_[5] = q_[5], q_[2]
    assert _raises(chk.check_layout, damaged(layout=(s_, w_, h_, q_)))
    chk.check_all(good)                                            # and the undamaged result still passes
