"""Per-frame camera models (rpe_*_cameras, Camera, PoseEstimator(dist_coeffs=...)) on the GPU.  Bit comparisons are
np.array_equal on doubles viewed as uint64; the lens itself is checked against tests/camera_model.py, the float64
specification of the camera path (cv2 is not available to the tests)."""
import numpy as np
import pytest

import camera_model as cm

pytestmark = pytest.mark.gpu

# the 21 pairs of tests/test_gpu_pairs.py: (i, i + d) for d = 1, 2, 3, two reversed pairs and a self pair
WINDOW = [(i, i + d) for d in (1, 2, 3) for i in range(8 - d)] + [(3, 0), (7, 4), (2, 2)]


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def frames(K_vga):
    from relative_pose_estimation_amd import synthetic
    return synthetic.make_stream(8, K_vga)[0]


@pytest.fixture(scope="module")
def eng(capi):
    e = capi.Engine(640, 480, max_batch=24, nfeatures=1000, max_matches=500)
    yield e
    e.close()


@pytest.fixture(scope="module")
def strong16(K_vga):
    """the 16 strong-lens pairs of the accuracy table"""
    from relative_pose_estimation_amd import synthetic
    return synthetic.make_batch(16, K_vga, cfg=8, dist=cm.STRONG, workers=8)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b, what=""):
    """two tuples of arrays, bit for bit"""
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        x = np.asarray(x); y = np.asarray(y)
        if x.dtype == np.float64:
            x, y = _u64(x), _u64(y)
        assert x.shape == y.shape and np.array_equal(x, y), (what, "field", k)


def _with_images(e, i1, i2, fn):
    d1 = e.upload(i1); d2 = e.upload(i2)
    try:
        return fn(d1, d2)
    finally:
        e.synchronize()
        e.device_free(d1); e.device_free(d2)


def _all_of(e, B):
    """what test 1 compares after a batch or pair list: structure and refined poses"""
    return e.fetch_structure(B) + e.refine_poses(B)


def _store8(e, frames):
    e.frames_reserve(0)
    e.frames_reserve(8)
    e.frames_put(frames, np.arange(8))


# ------------------------------------------------------------------ 1. pinhole cameras change nothing
def test_pinhole_cameras_return_todays_bits(capi, eng, frames, K_vga):
    cam = capi.Camera(K_vga)
    w = np.asarray(WINDOW)
    i1, i2 = frames[w[:8, 0]], frames[w[:8, 1]]

    def both(d1, d2):
        a = eng.estimate_batch_device(d1, d2, 8, K_vga); sa = _all_of(eng, 8)
        b = eng.estimate_batch_cameras_device(d1, d2, 8, cam, cam); sb = _all_of(eng, 8)
        c = eng.estimate_batch_device(d1, d2, 8, K_vga); sc = _all_of(eng, 8)       # and back: the camera path leaves nothing behind
        return a, sa, b, sb, c, sc
    a, sa, b, sb, c, sc = _with_images(eng, i1, i2, both)
    assert (a[4] == 0).all() and (a[3] >= 400).all(), (a[4], a[3])                    # not an empty comparison
    _same(a, b, "camera batch"); _same(sa, sb, "camera batch: structure / refined")
    _same(a, c, "single-K batch after a camera batch"); _same(sa, sc, "single-K after: structure / refined")
    _same(a, eng.estimate_batch_cameras(i1, i2, cam, cam), "host camera batch")

    _store8(eng, frames)
    p = eng.estimate_pairs(w[:, 0], w[:, 1], K_vga); sp = _all_of(eng, 21)
    eng.frames_set_cameras(np.arange(8), cam)
    q = eng.estimate_pairs_cameras(w[:, 0], w[:, 1]); sq = _all_of(eng, 21)
    assert (p[4] == 0).all()
    _same(p, q, "camera pair list"); _same(sp, sq, "camera pair list: structure / refined")
    _same(p, eng.estimate_pairs(w[:, 0], w[:, 1], K_vga), "single-K pair list ignores slot cameras")
    eng.frames_reserve(0)


def test_estimator_with_zero_dist_coeffs_returns_todays_bits(frames, K_vga):
    from relative_pose_estimation_amd import PoseEstimator
    plain = PoseEstimator(K_vga, nfeatures=1000, max_batch=8)
    lens = PoseEstimator(K_vga, nfeatures=1000, max_batch=8, dist_coeffs=np.zeros(5))
    try:
        _same(plain.estimate(frames[0], frames[1]), lens.estimate(frames[0], frames[1]), "estimate")
        a, b = plain.estimate_with_structure(frames[0], frames[2]), lens.estimate_with_structure(frames[0], frames[2])
        assert a.keys() == b.keys()
        _same([np.asarray(a[k]) for k in a], [np.asarray(b[k]) for k in a], "estimate_with_structure")
        a, b = plain.estimate_refined(frames[1], frames[2]), lens.estimate_refined(frames[1], frames[2])
        _same([np.asarray(a[k]) for k in a if k != 'vp_debug'], [np.asarray(b[k]) for k in a if k != 'vp_debug'], "estimate_refined")
        _same(plain.estimate_batch(frames[:4], frames[4:]), lens.estimate_batch(frames[:4], frames[4:]), "estimate_batch")
        _same(plain.last_refined(), lens.last_refined(), "last_refined")
        _same(plain.estimate_sequence(frames), lens.estimate_sequence(frames), "estimate_sequence")
        _same(plain.estimate_pairs(frames, WINDOW), lens.estimate_pairs(frames, WINDOW), "estimate_pairs")
    finally:
        plain.close(); lens.close()


# ------------------------------------------------------------------ 2. a mixed batch is its parts
def test_mixed_batch_and_pair_list_are_their_parts(capi, eng, frames, K_vga):
    KA = K_vga
    KB = K_vga.copy(); KB[0, 0] *= 1.125; KB[1, 1] *= 1.0625; KB[0, 2] += 7.5; KB[1, 2] -= 3.25
    camA, camB = capi.Camera(KA), capi.Camera(KB)
    w = np.asarray(WINDOW)
    i1, i2 = frames[w[:8, 0]], frames[w[:8, 1]]
    cams = [camA if p % 2 == 0 else camB for p in range(8)]

    def run(d1, d2):
        return (eng.estimate_batch_device(d1, d2, 8, KA), eng.estimate_batch_device(d1, d2, 8, KB),
                eng.estimate_batch_cameras_device(d1, d2, 8, cams, cams))
    a, b, m = _with_images(eng, i1, i2, run)
    assert (a[4] == 0).all() and (b[4] == 0).all()
    assert not np.array_equal(_u64(a[0]), _u64(b[0])), "the two cameras must give different poses, or the test shows nothing"
    for p in range(8):
        part = a if p % 2 == 0 else b
        _same([x[p] for x in part], [x[p] for x in m], f"mixed batch, pair {p}")

    # store: frames 0..3 on camera A, 4..7 on camera B; pairs inside either group
    _store8(eng, frames)
    eng.frames_set_cameras(np.arange(8), [camA] * 4 + [camB] * 4)
    pl = np.asarray([(0, 1), (4, 5), (1, 3), (7, 5), (2, 0), (6, 6), (3, 2), (5, 7)])
    a = eng.estimate_pairs(pl[:, 0], pl[:, 1], KA); b = eng.estimate_pairs(pl[:, 0], pl[:, 1], KB)
    m = eng.estimate_pairs_cameras(pl[:, 0], pl[:, 1])
    for p in range(len(pl)):
        part = a if pl[p, 0] < 4 else b
        _same([x[p] for x in part], [x[p] for x in m], f"mixed pair list, pair {p}")
    eng.frames_reserve(0)


# ------------------------------------------------------------------ 3. two cameras in one pair, exactly
def test_two_cameras_in_one_pair_exact_scaling(capi, eng, frames, oracle):
    """camera 2 = camera 1 scaled by two with pts2 doubled: the normalised points are bitwise the single camera's, and
    threshold 1.5 over the mean focal 768 is 1.0 / 512 exactly"""
    f, cx, cy = 512.0, 320.0, 240.0
    K1 = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.]])
    K2 = np.array([[2 * f, 0, 2 * cx], [0, 2 * f, 2 * cy], [0, 0, 1.]])
    assert 1.5 / 768 == 1.0 / 512
    w = np.asarray(WINDOW)
    B = 6
    res = eng.estimate_batch(frames[w[:B, 0]], frames[w[:B, 1]], K1)
    p1s, p2s = eng.fetch_matched_points(B)
    nm = res[3]
    assert (nm >= 400).all()
    pts1 = [p1s[p, :nm[p]] for p in range(B)]; pts2 = [p2s[p, :nm[p]] for p in range(B)]
    pts2x = [(2 * q).astype(np.float32) for q in pts2]
    e15 = capi.Engine(640, 480, max_batch=B, nfeatures=1000, max_matches=500, ransac_threshold=1.5)
    try:
        E0, m0, f0, i0 = eng.find_essential(pts1, pts2, K1)
        E1, m1, f1, i1 = e15.find_essential_cameras(pts1, pts2x, capi.Camera(K1), capi.Camera(K2))
        _same((E0, m0, f0, i0), (E1, m1, f1, i1), "find_essential")
        assert (f0 == 1).all()
        for p in range(B):
            _, om, _ = oracle.find_essential(pts1[p], pts2[p], K1)
            assert np.array_equal(m1[p, :nm[p]], om), p
        _same(eng.recover_pose(E0, pts1, pts2, K1), e15.recover_pose_cameras(E1, pts1, pts2x, capi.Camera(K1), capi.Camera(K2)), "recover_pose")
        # the refinement's pixel scale is the mean focal too: 768 against 512 scales the residuals, not the minimiser's
        # path bit for bit, so only the single-camera form is compared exactly
        R0, t0, _ = eng.recover_pose(E0, pts1, pts2, K1)
        masks = [m0[p, :nm[p]] for p in range(B)]
        _same(eng.refine_pose_points(R0, t0, pts1, pts2, masks, K1),
              eng.refine_pose_points_cameras(R0, t0, pts1, pts2, masks, capi.Camera(K1), capi.Camera(K1)), "refine_pose_points")
    finally:
        e15.close()


# ------------------------------------------------------------------ 4. undistortion against the model
@pytest.mark.parametrize("name,dist", [("mild", cm.MILD), ("strong", cm.STRONG), ("rational", cm.RATIONAL)])
def test_undistort_points_against_the_model(capi, eng, K_vga, name, dist):
    """values are O(1), about 150 rounded operations, a contraction mapping: the bound is near 1e-13; 1e-12 is 10x over it"""
    rng = np.random.default_rng(11)
    pts = np.vstack([rng.random((4096, 2)) * [639, 479], [[0, 0], [639, 0], [0, 479], [639, 479]]]).astype(np.float32)
    got = eng.undistort_points(pts, capi.Camera(K_vga, dist))
    ref = cm.normalise(pts, cm.Cam(K_vga, dist))
    err = float(np.abs(got - ref).max())
    print(name, "max |gpu - model|", err, "bit-identical:", bool(np.array_equal(_u64(got), _u64(ref))))
    assert err <= 1e-12
    # the lens does something: the corner moves by tens of pixels
    raw = cm.normalise(pts, cm.Cam(K_vga))
    assert np.abs(got - raw).max() * K_vga[0, 0] > 10


# ------------------------------------------------------------------ 5. masks and structure under a lens
def test_masks_and_structure_under_a_lens(capi, K_vga, strong16):
    i1, i2 = strong16[0][:8], strong16[1][:8]
    cam = capi.Camera(K_vga, cm.STRONG); mc = cm.Cam(K_vga, cm.STRONG)
    e = capi.Engine(640, 480, max_batch=8, nfeatures=1000, max_matches=500)
    try:
        def run(d1, d2):
            res = e.estimate_batch_cameras_device(d1, d2, 8, cam, cam)
            return res, e.fetch_structure(8), e.fetch_matched_points(8)
        (R, t, inl, nm, st), (rm, pm, pts), (p1s, p2s) = _with_images(e, i1, i2, run)
        assert (st == 0).all() and (nm >= 357).all(), (st, nm)
        pts1 = [p1s[p, :nm[p]] for p in range(8)]; pts2 = [p2s[p, :nm[p]] for p in range(8)]
        E, smask, found, _ = e.find_essential_cameras(pts1, pts2, cam, cam)
        assert (found == 1).all()
        excluded = 0
        for p in range(8):
            n = int(nm[p])
            x1 = cm.normalise(pts1[p], mc); x2 = cm.normalise(pts2[p], mc)
            mask, near = cm.sampson_mask(E[p], x1, x2, 1.0, cm.pair_focal(mc, mc))
            excluded += int(near.sum())
            assert np.array_equal(rm[p, :n], smask[p, :n].astype(bool)), (p, "batch mask vs stage mask")
            assert not ((rm[p, :n] != mask) & ~near).any(), (p, np.nonzero(rm[p, :n] != mask))
            assert not rm[p, n:].any() and not pm[p, n:].any() and not pts[p, n:].any(), p
            assert int(pm[p].sum()) == int(inl[p]), (p, pm[p].sum(), inl[p])
            cmask, P, cnear = cm.triangulate(R[p], t[p], x1, x2)
            assert not ((pm[p, :n] != cmask) & ~cnear).any(), (p, np.nonzero(pm[p, :n] != cmask))
            sel = pm[p, :n] & cmask
            err = np.linalg.norm(pts[p, :n][sel] - P[sel], axis=1)
            assert np.all(err <= 1e-7 * np.maximum(1.0, np.linalg.norm(P[sel], axis=1))), (p, err.max())
            print(p, "matches", n, "ransac inliers", int(rm[p].sum()), "pose inliers", int(inl[p]), "near the threshold", int(near.sum()))
        print("excluded", excluded, "of", int(nm.sum()))
        assert excluded <= 0.01 * nm.sum()
    finally:
        e.close()


# ------------------------------------------------------------------ 6. it helps
def test_cameras_beat_ignoring_the_lens(capi, K_vga, strong16):
    """CPU reference (tests/test_camera_cpu.py, accuracy table): median rotation error 2.038 deg ignoring the strong lens,
    0.548 deg with the matched points undistorted first"""
    from relative_pose_estimation_amd.geometry import rotation_error
    i1, i2, Rgt, _ = strong16
    cam = capi.Camera(K_vga, cm.STRONG)
    e = capi.Engine(640, 480, max_batch=16, nfeatures=1000, max_matches=500)
    try:
        def run(d1, d2):
            return e.estimate_batch_device(d1, d2, 16, K_vga), e.estimate_batch_cameras_device(d1, d2, 16, cam, cam)
        raw, fix = _with_images(e, i1, i2, run)
    finally:
        e.close()
    assert (raw[4] == 0).all() and (fix[4] == 0).all(), (raw[4], fix[4])
    r_raw = np.array([rotation_error(raw[0][p], Rgt[p]) for p in range(16)])
    r_fix = np.array([rotation_error(fix[0][p], Rgt[p]) for p in range(16)])
    print("rotation error ignoring the lens:", np.round(r_raw, 3).tolist())
    print("rotation error with cameras:     ", np.round(r_fix, 3).tolist())
    print("medians", float(np.median(r_raw)), float(np.median(r_fix)), "CPU reference", cm.CPU_STRONG_MEDIAN_ROT)
    assert np.median(r_fix) < np.median(r_raw)
    assert np.median(r_fix) <= 1.25 * cm.CPU_STRONG_MEDIAN_ROT[1]


# ------------------------------------------------------------------ 7. refusals, persistence
def test_refusals_leave_the_handle_usable(capi, eng, frames, K_vga):
    cam = capi.Camera(K_vga, cm.MILD)
    w = np.asarray(WINDOW)
    _store8(eng, frames)
    eng.frames_set_cameras(np.arange(7), cam)                       # slot 7 has none
    good = eng.estimate_pairs_cameras(w[:3, 0], w[:3, 1])
    assert (good[4] == 0).all()
    with pytest.raises(capi.RpeError):
        eng.estimate_pairs_cameras([0, 6], [1, 7])
    _same(good, eng.estimate_pairs_cameras(w[:3, 0], w[:3, 1]), "after a slot without a camera")
    bad_f = cam.record(); bad_f["fx"] = 0.
    bad_n = cam.record(); bad_n["dist"][0, 2] = np.nan
    for bad in (bad_f, bad_n):
        with pytest.raises(capi.RpeError):
            eng.frames_set_cameras([0], bad)
        with pytest.raises(capi.RpeError):
            eng.undistort_points(np.zeros((4, 2), np.float32), bad)
        with pytest.raises(capi.RpeError):
            eng.estimate_batch_cameras(frames[:1], frames[1:2], bad, cam)
        with pytest.raises(capi.RpeError):
            eng.find_essential_cameras([np.zeros((8, 2), np.float32)], [np.zeros((8, 2), np.float32)], cam, bad)
        _same(good, eng.estimate_pairs_cameras(w[:3, 0], w[:3, 1]), "after a refused camera")
    # cameras survive growth of the store ...
    eng.frames_reserve(12)
    _same(good, eng.estimate_pairs_cameras(w[:3, 0], w[:3, 1]), "after frames_reserve growth")
    with pytest.raises(capi.RpeError):
        eng.estimate_pairs_cameras([0], [7])                        # still none
    # ... and are replaced by a later assignment: the strong lens gives another pose, the mild one the first again
    eng.frames_set_cameras(np.arange(8), capi.Camera(K_vga, cm.STRONG))
    other = eng.estimate_pairs_cameras(w[:3, 0], w[:3, 1])
    assert not np.array_equal(_u64(other[0]), _u64(good[0]))
    eng.frames_put(frames[:4], np.arange(4))                        # a put keeps the slots' cameras
    eng.frames_set_cameras(np.arange(8), cam)
    _same(good, eng.estimate_pairs_cameras(w[:3, 0], w[:3, 1]), "after replacing the cameras")
    eng.frames_reserve(0)


def test_frame_store_uses_slot_cameras(frames, K_vga):
    """FrameStore.put(camera=...) / estimate: slot cameras when every named slot has one, the estimator's K when none has"""
    from relative_pose_estimation_amd import Camera, PoseEstimator
    est = PoseEstimator(K_vga, nfeatures=1000, max_batch=8)
    lens = PoseEstimator(K_vga, nfeatures=1000, max_batch=8, dist_coeffs=cm.MILD)
    try:
        fs = est.frame_store(8)
        fs.put_many(np.arange(4), frames[:4], cameras=Camera(K_vga, cm.MILD))
        fs.put_many(np.arange(4, 8), frames[4:])
        with_cam = fs.estimate([[0, 1], [1, 3]])
        without = fs.estimate([[4, 5], [5, 7]])
        with pytest.raises(ValueError):
            fs.estimate([[0, 4]])
        fs.close()
        _same(with_cam, lens.estimate_pairs(frames[:4], [[0, 1], [1, 3]]), "slot cameras vs dist_coeffs estimator")
        _same(without, est.estimate_pairs(frames[4:], [[0, 1], [1, 3]]), "slots without cameras vs plain estimator")
    finally:
        est.close(); lens.close()
