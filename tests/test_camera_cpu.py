"""Camera models, the parts that need no GPU: the float64 lens model itself, the lens of synthetic.py pinned through the
CPU oracle (the accuracy table the GPU test refers to), the NULL-handle refusals of the new C-ABI entry points, and the
Python-side validation that runs before any device call."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import camera_model as cm
from relative_pose_estimation_amd import Camera, PoseEstimator, _capi, synthetic
from relative_pose_estimation_amd.geometry import default_camera_matrix, rotation_error, translation_direction_error

K_VGA = default_camera_matrix(640, 480)
NEW_CALLS = ["rpe_frames_set_cameras", "rpe_enqueue_pairs_cameras", "rpe_estimate_pairs_cameras",
             "rpe_enqueue_batch_cameras_device", "rpe_estimate_batch_cameras_device", "rpe_estimate_batch_cameras",
             "rpe_undistort_points", "rpe_find_essential_cameras", "rpe_recover_pose_cameras", "rpe_refine_pose_points_cameras"]


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("dist", [cm.MILD, cm.STRONG])
def test_model_round_trip_over_the_vga_image(dist):
    """distort(undistort(x, 50)) returns to x within 1e-12 (normalised units) at every pixel of the VGA image"""
    cam = cm.Cam(K_VGA, dist)
    u, v = np.meshgrid(np.arange(640, dtype=np.float64), np.arange(480, dtype=np.float64))
    xd = (u - cam.cx) / cam.fx; yd = (v - cam.cy) / cam.fy
    x, y = cm.undistort(xd, yd, cam.dist, 50)
    xb, yb = cm.distort(x, y, cam.dist)
    err = max(np.abs(xb - xd).max(), np.abs(yb - yd).max())
    print("round trip, worst over the image:", err)
    assert err <= 1e-12


@pytest.mark.parametrize("dist,resid,places,shift", [(cm.MILD, 1e-4, 4, 19.6), (cm.STRONG, 0.035, 3, 55.3)])
def test_five_iterations_leave_the_documented_residual_at_the_corner(dist, resid, places, shift):
    """pixel (0, 0): distance between five iterations and the converged inverse, and the corner's shift, equal to the
    documented figures (1e-4 px and 0.035 px; 19.6 px and 55.3 px) at the decimal places they are quoted with"""
    cam = cm.Cam(K_VGA, dist)
    xd, yd = (0. - cam.cx) / cam.fx, (0. - cam.cy) / cam.fy
    x5, y5 = cm.undistort(xd, yd, cam.dist, cm.UNDISTORT_ITERS)
    x50, y50 = cm.undistort(xd, yd, cam.dist, 50)
    r = float(np.hypot((x5 - x50) * cam.fx, (y5 - y50) * cam.fy))
    s = float(np.hypot(x50 * cam.fx + cam.cx, y50 * cam.fy + cam.cy))
    print("corner residual", r, "px, corner shift", s, "px")
    assert round(r, places) == resid
    assert round(s, 1) == shift
    assert cm.UNDISTORT_ITERS == _capi.UNDISTORT_ITERS == 5


def test_normalise_without_a_lens_is_the_pinhole_expression():
    rng = np.random.default_rng(3)
    pts = (rng.random((1000, 2)) * [640, 480]).astype(np.float32)
    n = cm.normalise(pts, cm.Cam(K_VGA))
    p = pts.astype(np.float64)
    ref = np.stack([(p[:, 0] - K_VGA[0, 2]) / K_VGA[0, 0], (p[:, 1] - K_VGA[1, 2]) / K_VGA[1, 1]], 1)
    assert np.array_equal(n.view(np.uint64), ref.view(np.uint64))
    assert cm.pair_focal(cm.Cam(K_VGA), cm.Cam(K_VGA)) == (K_VGA[0, 0] + K_VGA[1, 1]) / 2


# ------------------------------------------------------------------ synthetic.py
def test_synthetic_without_a_lens_keeps_the_parent_commits_images():
    """dist=None: the images of make_batch / make_stream are the bits they were before the lens existed (sha256 recorded
    from the parent commit)"""
    m = hashlib.sha256()
    i1, i2, _, _ = synthetic.make_batch(2, K_VGA, cfg=8)
    m.update(i1.tobytes()); m.update(i2.tobytes())
    f, _, _ = synthetic.make_stream(3, K_VGA)
    m.update(f.tobytes())
    assert m.hexdigest() == PARENT_IMAGES_SHA256


PARENT_IMAGES_SHA256 = "addeef2fade24233ffa6f0cffeddceb11157787049b452e88a4c91c80be553dc"


def table_row(dist):
    """One row of the accuracy table: 16 pairs of make_batch(cfg=8) through the lens, ORB-1000 / 500 matches and pose
    from the CPU oracle, on the matched points as they are against the same points undistorted by the float64 model
    (five iterations) and re-projected to pinhole pixels (f32)."""
    from oracle import oracle
    i1, i2, Rgt, tgt = synthetic.make_batch(16, K_VGA, cfg=8, dist=dist)
    out, pts = oracle.estimate_pose_batch(i1, i2, K_VGA, 1000, 500, nthreads=4, return_points=True)
    nm = out["n_matches"]
    cam = cm.Cam(K_VGA, dist)
    und = np.zeros_like(pts)
    for b in range(16):
        for s in range(2):
            und[b, s] = cm.to_pixels(cm.normalise(pts[b, s], cam), cam).astype(np.float32)
    raw = oracle.pose_from_points_batch(pts, nm, K_VGA, nthreads=4)
    fix = oracle.pose_from_points_batch(und, nm, K_VGA, nthreads=4)
    rot = lambda o: np.array([rotation_error(o["R"][b].reshape(3, 3), Rgt[b]) for b in range(16)])
    tdir = lambda o: np.array([translation_direction_error(o["t"][b].reshape(3, 1), tgt[b]) for b in range(16)])
    return {"status": np.concatenate([out["status"], raw["status"], fix["status"]]), "min_matches": int(nm.min()),
            "rot": (rot(raw), rot(fix)), "t": (tdir(raw), tdir(fix))}


# (lens, median rotation error ignoring / undistorted, median t-direction error ignoring / undistorted, closer pairs)
TABLE = [(None, 0.479, 0.479, 6.43, 6.43, 0), (cm.MILD, 0.694, 0.386, 5.36, 3.46, 9), (cm.STRONG, *cm.CPU_STRONG_MEDIAN_ROT, 7.71, 3.98, 14)]


@pytest.mark.parametrize("dist,r_raw,r_fix,t_raw,t_fix,closer", TABLE)
def test_accuracy_table_through_the_cpu_oracle(dist, r_raw, r_fix, t_raw, t_fix, closer):
    """pins synthetic's lens (rendering and exact inverse) and is the reference of the GPU accuracy test"""
    row = table_row(dist)
    med = [float(np.median(a)) for a in (*row["rot"], *row["t"])]
    n_closer = int(np.sum(row["rot"][1] < row["rot"][0]))
    print("median rot ignoring / undistorted, t ignoring / undistorted:", med, "closer pairs:", n_closer,
          "fewest matches:", row["min_matches"])
    assert (row["status"] == 0).all() and row["min_matches"] >= 357
    assert [round(med[0], 3), round(med[1], 3)] == [r_raw, r_fix]
    assert [round(med[2], 2), round(med[3], 2)] == [t_raw, t_fix]
    assert n_closer == closer


# ------------------------------------------------------------------ C-ABI without a device
def test_new_entry_points_refuse_a_null_handle():
    lib = _capi.load()
    one = np.zeros(1, np.int32)
    cam = Camera(K_VGA).record()
    img = np.zeros((96, 96), np.uint8)
    pts = np.zeros((4, 2), np.float32)
    out = np.zeros(64)
    msk = np.zeros(16, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rpe_frames_set_cameras(None, 1, p(one), p(cam)) == -1
    assert lib.rpe_enqueue_pairs_cameras(None, p(one), p(one), 1) == -1
    assert lib.rpe_estimate_pairs_cameras(None, p(one), p(one), 1, p(out), p(out), p(one), p(one), p(one)) == -1
    assert lib.rpe_enqueue_batch_cameras_device(None, p(img), p(img), 1, p(cam), p(cam)) == -1
    assert lib.rpe_estimate_batch_cameras_device(None, p(img), p(img), 1, p(cam), p(cam), p(out), p(out), p(one), p(one), p(one)) == -1
    assert lib.rpe_estimate_batch_cameras(None, p(img), p(img), 1, p(cam), p(cam), p(out), p(out), p(one), p(one), p(one)) == -1
    assert lib.rpe_undistort_points(None, p(pts), 4, p(cam), p(out)) == -1
    assert lib.rpe_find_essential_cameras(None, p(pts), p(pts), p(one), 1, p(cam), p(cam), p(out), p(msk), p(one), p(one)) == -1
    assert lib.rpe_recover_pose_cameras(None, p(out), p(pts), p(pts), p(one), 1, p(cam), p(cam), p(out), p(out), p(one)) == -1
    assert lib.rpe_refine_pose_points_cameras(None, p(out), p(out), p(pts), p(pts), p(msk), p(one), 1, p(cam), p(cam), 5,
                                              p(out), p(out), p(one), p(one), p(out)) == -1


def test_exports_name_the_new_calls():
    for n in NEW_CALLS:
        assert n in _capi.EXPORTS
        getattr(_capi.load(), n)
    assert _capi.CAMERA_DTYPE.itemsize == 96


# ------------------------------------------------------------------ Python validation before any device call
def test_camera_validates_its_arguments():
    c = Camera(K_VGA, cm.STRONG)
    assert (c.fx, c.fy, c.cx, c.cy) == (K_VGA[0, 0], K_VGA[1, 1], K_VGA[0, 2], K_VGA[1, 2])
    assert list(c.dist) == list(cm.STRONG) + [0., 0., 0.]
    assert list(Camera(K_VGA).dist) == [0.] * 8 and list(Camera(K_VGA, cm.RATIONAL).dist) == list(cm.RATIONAL)
    r = c.record()
    assert r.dtype == _capi.CAMERA_DTYPE and r.nbytes == 96 and float(r["fx"][0]) == c.fx and list(r["dist"][0]) == list(c.dist)
    bad_K = K_VGA.copy(); bad_K[0, 0] = 0.
    nan_K = K_VGA.copy(); nan_K[1, 2] = np.nan
    for K, dist in [(np.eye(2), None), (bad_K, None), (nan_K, None), (K_VGA, [0.1, 0.2, 0.3]), (K_VGA, [np.nan, 0, 0, 0]),
                    (K_VGA, np.zeros(9)), (K_VGA, [np.inf, 0, 0, 0, 0])]:
        with pytest.raises(ValueError):
            Camera(K, dist)
    with pytest.raises(ValueError):
        _capi.camera_records([c, c], 3)
    with pytest.raises(ValueError):
        _capi.camera_records([c, K_VGA], 2)
    assert _capi.camera_records(c, 3).shape == (3,)


def test_vp_refinement_and_a_lens_are_refused_at_construction():
    with pytest.raises(ValueError):
        PoseEstimator(K_VGA, use_vp_refinement=True, dist_coeffs=np.zeros(5))
    with pytest.raises(TypeError):
        PoseEstimator(K_VGA, "ORB", "Hamming", 500, 4000, False, 120, 3000, 8e5, 8000.0, 12, 1e-2, 1e-3, 0, 1, None, "libstdc++",
                      np.zeros(5))                      # keyword-only
    with pytest.raises(ValueError):
        PoseEstimator(K_VGA, dist_coeffs=[0.1, 0.2])
    PoseEstimator(K_VGA, use_vp_refinement=True)         # unchanged
    PoseEstimator(K_VGA, dist_coeffs=cm.STRONG)


@pytest.fixture()
def pe(monkeypatch):
    est = PoseEstimator(K_VGA, nfeatures=1000, max_batch=4)

    def no_device(*a, **k):
        raise AssertionError("validation must fail before an engine is created")
    monkeypatch.setattr(est, "_engine", no_device)
    return est


def test_estimate_batch_validates_cameras_before_any_device_call(pe):
    imgs = np.zeros((2, 480, 640), np.uint8)
    cam = Camera(K_VGA)
    for c1, c2 in [([cam], None), (None, [cam, cam, cam]), ([cam, K_VGA], None)]:
        with pytest.raises(ValueError):
            pe.estimate_batch(imgs, imgs, cameras1=c1, cameras2=c2)


def test_frame_store_validates_cameras_before_any_device_call(pe):
    fs = pe.frame_store(4)
    img = np.zeros((480, 640), np.uint8)
    cam = Camera(K_VGA)
    with pytest.raises(ValueError):
        fs.put_many([0, 1], np.stack([img, img]), cameras=[cam])
    with pytest.raises(ValueError):
        fs.put(0, img, camera=K_VGA)
    # a list that names slots with and without a camera is refused before the engine is asked anything
    fs._has_cam[[0, 1]] = True
    with pytest.raises(ValueError):
        fs.estimate([[0, 1], [1, 2]])
    fs.close()
