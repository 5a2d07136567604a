"""Homography RANSAC and the rotation fit on the GPU (rpe_find_homography / rpe_pair_homographies, through the C-ABI)
against the float64 model of the header's rule (tests/homography_model.py).  mask, n_H, info and H are compared with
array_equal.  R_rot comes from the library's Jacobi SVD and the model's from LAPACK, so n_rot is compared with the model's
count evaluated at the RETURNED R_rot (exactly), and R_rot itself with the model's fit over the kernel's own mask under
ROT_BOUND_DEG.  Covered: the wave and workgroup edges of M, one, two and four rounds of samples, the three LDS layouts
(below 64 KB, above it, points read from HBM), invalid models, points behind the homography, batch / stream / pair list /
camera runs, failed pairs, the rendered rotation-only and general pairs, the refusals, and that the call changes nothing of
the run it reads."""
import numpy as np
import pytest

from tests import camera_model as cm
from tests import guided_model as gm
from tests import homography_cases as hc
from tests import homography_model as hm
from tests import scale_model as sc

pytestmark = pytest.mark.gpu

# Largest angle between the kernel's R_rot and the model's SVD fit over the kernel's own mask, over every OK pair of the
# stage-form cases below (summation order and Jacobi against LAPACK, not algorithm error): MEASURED_ROT_DEG; the bound is
# 1000 times that.
MEASURED_ROT_DEG = 2.611e-13
ROT_BOUND_DEG = 1000 * MEASURED_ROT_DEG
ORTHO_TOL = 1e-13          # R^T R and det: a few dozen roundings of 2.2e-16 through the Jacobi sweeps and the products


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


@pytest.fixture(scope="module")
def cases(K_vga):
    return hc.stage_cases(K_vga)


_subsets = {}


def subsets(oracle, M, iters):
    """rows [0, iters) of the subset stream of M (the stream does not depend on how many rows are drawn)"""
    if M < 6:
        return np.zeros((iters, 5), np.int32)
    if M not in _subsets or len(_subsets[M]) < iters:
        _subsets[M] = oracle.ransac_subsets(M, max(iters, 1000))
    return _subsets[M][:iters]


def assert_pair(p, got, r, a, b, thr2, mm, n_E=None):
    """one pair of a GPU result against the model's dict r; returns the angle (deg) between the two rotation fits or None"""
    H, R, mask, counts, info = got
    M = len(a)
    assert info[p].tolist() == [r["code"], r["it"], r["n_valid"], 0], (p, info[p].tolist(), r["code"], r["it"], r["n_valid"])
    assert np.array_equal(mask[p, :M], r["mask"]) and not mask[p, M:].any(), p
    assert np.array_equal(H[p], r["H"]), (p, H[p], r["H"])
    assert counts[p, 0] == r["n_H"], (p, counts[p].tolist(), r["n_H"])
    if n_E is not None:
        assert counts[p, 2] == n_E, (p, counts[p].tolist(), n_E)
    if r["code"] != hm.HOMOGRAPHY_OK:
        assert not R[p].any() and counts[p, 0] == 0 and counts[p, 1] == 0, p
        return None
    if not R[p].any():                                          # a non-finite fit is returned as zeros
        assert counts[p, 1] == 0, p
        return None
    assert counts[p, 1] == hm.rotation_count(R[p], a, b, thr2)[0], (p, counts[p].tolist())
    assert np.abs(R[p].T @ R[p] - np.eye(3)).max() <= ORTHO_TOL and abs(np.linalg.det(R[p]) - 1) <= ORTHO_TOL, p
    if r["n_H"] < 4:
        return None
    return hm.rotation_angle_deg(R[p], hm.rotation_fit(a, b, mask[p, :M]))


def run_stage(e, cases, K, oracle, iters, gate_px=hc.GATE_PX):
    """the stage form over the cases in chunks of max_batch, every pair against the model; returns the rotation angles"""
    thr2 = gm.thr2_of(gate_px, gm.focal_K(K))
    angles = []
    for c0 in range(0, len(cases), e.max_batch):
        chunk = cases[c0:c0 + e.max_batch]
        got = e.find_homography([c[1] for c in chunk], [c[2] for c in chunk], K, iters, gate_px)
        assert (got[3][:, 2] == -1).all()
        for p, (name, p1, p2) in enumerate(chunk):
            a, b = gm.normalise_K(p1, K), gm.normalise_K(p2, K)
            r = hm.find_homography(a, b, subsets(oracle, len(a), iters), thr2)
            ang = assert_pair(p, got, r, a, b, thr2, e.max_matches)
            if ang is not None:
                print(f"R_rot vs LAPACK fit: {name} iters {iters}: {ang:.3e} deg (n_H {r['n_H']})")
                angles.append(ang)
    return angles


# ------------------------------------------------------------------ stage form
@pytest.fixture(scope="module")
def stage_engine(capi):
    e = capi.Engine(640, 480, max_batch=8, nfeatures=1000, max_matches=500)
    yield e
    e.close()


def test_cases_exercise_the_rule(oracle, K_vga, cases):
    """the inputs do what the tests below rely on: the gate cuts through the true correspondences, invalid models occur,
    points lie behind the winner, winners past the first round of 256 samples"""
    thr2 = gm.thr2_of(hc.GATE_PX, gm.focal_K(K_vga))
    by_name = {c[0]: c for c in cases}
    p1, p2, true, _ = hc.scene_points("plane", 256, K_vga, 2, noise=hc.STAGE_NOISE_PX)
    assert np.array_equal(p1, by_name["plane-256"][1])
    r, _, _ = hc.model_on_pixels(p1, p2, K_vga, subsets(oracle, 256, 256))
    assert r["mask"][true].any() and not r["mask"][true].all()
    _, p1, p2 = by_name["duplicated-64"]
    r, _, _ = hc.model_on_pixels(p1, p2, K_vga, subsets(oracle, 64, 256))
    assert 0 < r["n_valid"] < 256
    _, p1, p2 = by_name["behind-200"]
    r, a, b = hc.model_on_pixels(p1, p2, K_vga, subsets(oracle, 200, 256))
    H = r["H"]
    w = (H[2, 0] * a[:, 0] + H[2, 1] * a[:, 1]) + H[2, 2]
    assert (w <= 0).sum() > 10 and r["n_H"] > 100 and not r["mask"][w <= 0].any()
    late = [hm.find_homography(gm.normalise_K(c[1], K_vga), gm.normalise_K(c[2], K_vga), subsets(oracle, len(c[1]), 1000), thr2)["it"]
            for c in cases if len(c[1]) >= 6]
    assert max(late) >= 256


@pytest.mark.parametrize("iters", [1, 256, 257, 1000])
def test_stage_form_equals_the_model(stage_engine, oracle, K_vga, cases, iters):
    """iters = 1; 256 = one full round of samples; 257 = the second round starts; 1000 = ransac_max_iters"""
    assert stage_engine.cfg.ransac_max_iters == 1000
    angles = run_stage(stage_engine, cases, K_vga, oracle, iters)
    assert iters == 1 or len(angles) >= 6
    assert max(angles, default=0.0) <= ROT_BOUND_DEG, max(angles)


def test_another_gate(stage_engine, oracle, K_vga, cases):
    angles = run_stage(stage_engine, cases, K_vga, oracle, 64, gate_px=2.5)
    assert max(angles) <= ROT_BOUND_DEG, max(angles)


def test_lds_above_64_kb(capi, oracle, K_vga):
    """max_matches = 1024: 36 KB of models + 32 KB of points, the kernel's raised dynamic-LDS limit"""
    e = capi.Engine(640, 480, max_batch=2, nfeatures=1000, max_matches=1024)
    big = [("rotation-1024",) + hc.scene_points("rotation", 1024, K_vga, 2, noise=hc.STAGE_NOISE_PX)[:2],
           ("plane-1000",) + hc.scene_points("plane", 1000, K_vga, 2, noise=hc.STAGE_NOISE_PX)[:2]]
    angles = run_stage(e, big, K_vga, oracle, 300)
    assert len(angles) == 2 and max(angles) <= ROT_BOUND_DEG, angles
    e.close()


def test_lds_at_the_2048_match_cut(capi, oracle, K_vga):
    """max_matches = 2048, the largest count that stages the points in LDS: 36 KB of models + 64 KB of points = 102400 bytes,
    the ceiling rpe_create raises homography_kernel<false> to (the launch asks for it whatever a pair holds)"""
    e = capi.Engine(640, 480, max_batch=2, nfeatures=2000, max_matches=2048)
    assert 256 * 18 * 8 + 32 * e.max_matches == 102400
    big = [("rotation-2048",) + hc.scene_points("rotation", 2048, K_vga, 2, noise=hc.STAGE_NOISE_PX)[:2],
           ("plane-1000",) + hc.scene_points("plane", 1000, K_vga, 2, noise=hc.STAGE_NOISE_PX)[:2]]
    angles = run_stage(e, big, K_vga, oracle, 300)
    assert len(angles) == 2 and max(angles) <= ROT_BOUND_DEG, angles
    e.close()


def test_points_read_from_hbm_above_2048_matches(capi, oracle, K_vga):
    """max_matches > 2048: the points no longer fit LDS beside the models"""
    e = capi.Engine(640, 480, max_batch=2, nfeatures=2100, max_matches=2112)
    big = [("rotation-2049",) + hc.scene_points("rotation", 2049, K_vga, 2, noise=hc.STAGE_NOISE_PX)[:2],
           ("general-70",) + hc.scene_points("general", 70, K_vga, 2, noise=hc.STAGE_NOISE_PX)[:2]]
    angles = run_stage(e, big, K_vga, oracle, 257)
    assert max(angles) <= ROT_BOUND_DEG, angles
    e.close()


# ------------------------------------------------------------------ batch form
def snapshot(e, P):
    return list(e.fetch_results(P)) + list(e.fetch_structure(P)) + list(e.refine_poses(P)) + list(e.fetch_matched_points(P))


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def check_run(e, P, oracle, K=None, cams=None, pairs=None, iters=256, gate_px=None):
    """pair_homographies over the last run == the model fed with the run's matched points, normalised as the geometry
    stages normalise them; n_E == the sum of findEssentialMat's mask; a failed pair is skipped; the run is untouched and
    a second call returns the same bits"""
    before = snapshot(e, P)
    got = e.pair_homographies(P, iters, gate_px)
    again = e.pair_homographies(P, iters, gate_px)
    assert_same(got, again)
    assert_same(before, snapshot(e, P))
    res = before[:5]
    nm, st, rmask = res[3], res[4], before[5]
    p1, p2 = before[-2], before[-1]
    g = 1.0 if gate_px is None else gate_px
    for p in range(P):
        M = int(nm[p]) if st[p] == 0 else 0
        if cams is None:
            a, b = gm.normalise_K(p1[p, :M], K), gm.normalise_K(p2[p, :M], K)
            thr2 = gm.thr2_of(g, gm.focal_K(K))
        else:
            c1, c2 = cams[pairs[p][0]], cams[pairs[p][1]]
            a, b = cm.normalise(p1[p, :M], c1), cm.normalise(p2[p, :M], c2)
            thr2 = gm.thr2_of(g, cm.pair_focal(c1, c2))
        r = hm.find_homography(a, b, subsets(oracle, M, iters), thr2, skipped=st[p] != 0)
        if st[p] != 0:
            assert got[4][p, 0] == hm.HOMOGRAPHY_SKIPPED and not got[2][p].any()
        assert_pair(p, got, r, a, b, thr2, e.max_matches, n_E=int(rmask[p].sum()))
    return got, res


def test_batch_with_a_failed_pair(capi, oracle, physics):
    frames, K = physics
    imgs1 = np.stack([frames[0], np.zeros_like(frames[0]), frames[1]]); imgs2 = np.stack([frames[1], np.zeros_like(frames[0]), frames[3]])
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    st = e.estimate_batch(imgs1, imgs2, K)[4]
    assert st[0] == 0 and st[1] != 0 and st[2] == 0
    got, _ = check_run(e, 3, oracle, K=K)
    assert got[4][:, 0].tolist() == [hm.HOMOGRAPHY_OK, hm.HOMOGRAPHY_SKIPPED, hm.HOMOGRAPHY_OK]
    check_run(e, 2, oracle, K=K, iters=1000, gate_px=2.0)          # fewer pairs than the run, every sample of the table
    e.close()


def test_stream_and_pair_list(capi, oracle, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.estimate_stream(frames[:4], K)
    got, res = check_run(e, 3, oracle, K=K)
    print("stream: counts (n_H, n_rot, n_E)", got[3].tolist(), "matches", res[3].tolist())
    # pair list: a reversed pair and a self pair (every match maps onto itself: H = identity, every match an inlier)
    pairs = [(0, 1), (0, 2), (1, 2), (2, 1), (3, 3), (2, 3)]
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    s1, s2 = np.array(pairs, np.int32).T
    e.estimate_pairs(s1, s2, K)
    got, res = check_run(e, 6, oracle, K=K)
    print("pair list: counts", got[3].tolist(), "matches", res[3].tolist(), "status", res[4].tolist())
    if res[4][4] == 0:
        assert got[3][4, 0] == res[3][4] and got[3][4, 1] == res[3][4]
    e.close()


def test_cameras(capi, oracle, physics):
    frames, K = physics
    pairs = [(0, 1), (1, 2), (2, 0)]
    s1, s2 = np.array(pairs, np.int32).T
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500)
    e.frames_reserve(3)
    e.frames_put(frames[:3], [0, 1, 2])
    # single K, then pinhole cameras: the same bits
    e.estimate_pairs(s1, s2, K)
    hk = e.pair_homographies(3)
    e.frames_set_cameras([0, 1, 2], capi.Camera(K))
    e.estimate_pairs_cameras(s1, s2)
    assert_same(hk, e.pair_homographies(3))
    # a lens on slot 1 and another focal length on slot 2
    K2 = K.copy(); K2[0, 0] *= 1.02; K2[1, 1] *= 1.02
    dist = [-0.08, 0.02, 0.001, -0.0005]
    e.frames_set_cameras([0, 1, 2], [capi.Camera(K), capi.Camera(K, dist), capi.Camera(K2)])
    e.estimate_pairs_cameras(s1, s2)
    cams = [cm.Cam(K), cm.Cam(K, dist), cm.Cam(K2)]
    got, _ = check_run(e, 3, oracle, cams=cams, pairs=pairs)
    print("cameras: counts", got[3].tolist())
    # a camera batch
    e.estimate_batch_cameras(frames[:2], frames[1:3], [capi.Camera(K), capi.Camera(K, dist)], [capi.Camera(K, dist), capi.Camera(K2)])
    check_run(e, 2, oracle, cams=cams, pairs=[(0, 1), (1, 2)])
    e.close()


def test_camera_batch_at_the_2048_match_cut(capi, oracle, physics):
    """homography_kernel<true> at its ceiling of 102400 bytes: the camera batch of test_cameras on a handle with
    max_matches = 2048"""
    frames, K = physics
    K2 = K.copy(); K2[0, 0] *= 1.02; K2[1, 1] *= 1.02
    dist = [-0.08, 0.02, 0.001, -0.0005]
    cams = [cm.Cam(K), cm.Cam(K, dist), cm.Cam(K2)]
    e = capi.Engine(640, 480, max_batch=2, nfeatures=2000, max_matches=2048)
    res = e.estimate_batch_cameras(frames[:2], frames[1:3], [capi.Camera(K), capi.Camera(K, dist)], [capi.Camera(K, dist), capi.Camera(K2)])
    assert not res[4].any(), res[4]
    got, _ = check_run(e, 2, oracle, cams=cams, pairs=[(0, 1), (1, 2)])
    assert (got[4][:, 0] == hm.HOMOGRAPHY_OK).all()
    e.close()


# ------------------------------------------------------------------ end to end
def test_rendered_pairs_classify_as_on_the_cpu(capi, oracle, K_vga):
    """the rotation-only and general rendered pairs of tests/test_homography_cpu.py on the GPU: the counts equal the
    model's on the GPU's own matched points, and classify_pair names them as it does on the CPU"""
    from relative_pose_estimation_amd import PoseEstimator, geometry
    i1, i2, Rgt = hc.rendered_images(K_vga)
    e = capi.Engine(640, 480, max_batch=6, nfeatures=1000, max_matches=500)
    R, t, inl, nm, st = e.estimate_batch(i1, i2, K_vga)
    assert (st == 0).all()
    got, _ = check_run(e, 6, oracle, K=K_vga)
    e.close()
    H, Rrot, mask, counts, info = got
    for p, (seed, baseline) in enumerate(hc.RENDERED):
        kind = geometry.classify_pair(int(nm[p]), int(counts[p, 2]), int(counts[p, 0]), int(counts[p, 1]), hc.ROTATION_RATIO, hc.PLANAR_RATIO)
        print(f"seed {seed} baseline {baseline}: matches {nm[p]} recoverPose inliers {inl[p]} five-point R error "
              f"{geometry.rotation_error(R[p], Rgt[p]):.3f} deg; n_H {counts[p, 0]} n_rot {counts[p, 1]} n_E {counts[p, 2]} "
              f"R_rot error {hm.rotation_angle_deg(Rrot[p], Rgt[p]):.3f} deg -> {kind}")
        if baseline == 0.0:
            assert kind == "rotation" and counts[p, 0] >= 0.5 * nm[p] and inl[p] <= 0.1 * nm[p], p
            assert hm.rotation_angle_deg(Rrot[p], Rgt[p]) < 0.05, p
        else:
            assert kind == "general" and counts[p, 0] <= 0.5 * counts[p, 2], p
    # the drop-in: the same pairs one at a time
    pe = PoseEstimator(K_vga, nfeatures=1000, max_matches=500)
    for p in (0, 3):
        Rp, tp, n_in, geom = pe.estimate_with_geometry(i1[p], i2[p], rotation_ratio=hc.ROTATION_RATIO, planar_ratio=hc.PLANAR_RATIO)
        assert np.array_equal(Rp, R[p]) and np.array_equal(tp, t[p]) and n_in == inl[p]
        assert geom["kind"] == ("rotation" if hc.RENDERED[p][1] == 0.0 else "general")
        assert (geom["n_H"], geom["n_rot"], geom["n_E"]) == tuple(counts[p].tolist()) and geom["n_matches"] == nm[p]
        assert np.array_equal(geom["H"], H[p]) and np.array_equal(geom["R_rot"], Rrot[p]) and np.array_equal(geom["mask"], mask[p, :nm[p]])
        Hp = geometry.pixel_homography(geom["H"], K_vga, K_vga)
        assert Hp.shape == (3, 3) and np.isfinite(Hp).all()
    d = pe.last_homographies()
    assert d["H"].shape == (1, 3, 3) and d["n_H"][0] == counts[3, 0] and d["code"][0] == hm.HOMOGRAPHY_OK
    # estimate itself is what it was
    Rp, tp = pe.estimate(i1[3], i2[3])
    assert np.array_equal(Rp, R[3]) and np.array_equal(tp, t[3])
    pe.close()


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500)
    e.frames_reserve(2)
    e.estimate_stream(frames[:3], K)
    good = e.pair_homographies(2)
    assert (good[4][:, 0] == hm.HOMOGRAPHY_OK).all() and good[3][:, 0].min() > 0
    lib, h = e.lib, e.h
    raw = lambda B, iters, thr: lib.rpe_pair_homographies(h, B, iters, thr, None, None, None, None, None)
    assert raw(2, 256, 1.0) == 0                                   # every output may be NULL
    for args in ((3, 256, 1.0),                                    # more pairs than the run
                 (0, 256, 1.0), (4, 256, 1.0),                     # outside 1 .. max_batch
                 (2, 0, 1.0), (2, 1001, 1.0), (2, -5, 1.0),        # iters outside 1 .. ransac_max_iters
                 (2, 256, 0.0), (2, 256, -1.0), (2, 256, float("nan")), (2, 256, float("inf"))):
        assert raw(*args) == -1, args
        assert_same(good, e.pair_homographies(2))
    assert raw(2, 1000, 1.0) == 0 and raw(2, 1, 1e-6) == 0
    # after a put the workspace holds other points
    e.frames_put(frames[3:4], [0])
    assert raw(2, 256, 1.0) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.pair_homographies(2))
    # after a stage call -- the stage form itself included
    p1, p2, _, _ = hc.scene_points("plane", 64, K, 1)
    stage = e.find_homography([p1], [p2], K)
    assert stage[4][0, 0] == hm.HOMOGRAPHY_OK
    assert raw(2, 256, 1.0) == -1
    with pytest.raises(capi.RpeError, match="rpe_pair_homographies"):
        e.pair_homographies(2)
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.pair_homographies(2))
    # once the store was resized under a pair list
    e.frames_put(frames[:2], [0, 1])
    e.estimate_pairs([0], [1], K)
    assert raw(1, 256, 1.0) == 0
    e.frames_reserve(3)
    assert raw(1, 256, 1.0) == -1
    # the stage form's own checks
    m = np.array([64], np.int32)
    pp1 = np.zeros((1, 500, 2), np.float32); pp2 = np.zeros((1, 500, 2), np.float32)
    pp1[0, :64] = p1; pp2[0, :64] = p2
    Kc = np.ascontiguousarray(K, np.float64)
    vp = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    sraw = lambda iters, thr, mm=m: lib.rpe_find_homography(h, vp(pp1), vp(pp2), vp(mm), 1, vp(Kc), iters, thr, None, None, None, None, None)
    for args in ((0, 1.0), (1001, 1.0), (256, 0.0), (256, float("nan")), (256, float("inf"))):
        assert sraw(*args) == -1, args
    assert sraw(256, 1.0, np.array([501], np.int32)) == -1
    assert sraw(256, 1.0) == 0
    assert_same(stage, e.find_homography([p1], [p2], K))
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.pair_homographies(2))
    e.close()
