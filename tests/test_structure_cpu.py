"""Per-match structure (rpe_fetch_structure / PoseEstimator.estimate_with_structure / last_structure): the float64
numpy model of recoverPose's triangulation and mask (tests/structure_model.py) checked on CPU against exact geometry
and the CPU oracle, and the public surface that exposes it."""
import numpy as np

from tests import structure_model as sm


def _project(X, R, t, K):
    Xc = X @ R.T + t
    p1 = (X[:, :2] / X[:, 2:3]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    p2 = (Xc[:, :2] / Xc[:, 2:3]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    return p1, p2, Xc[:, 2]


def test_model_on_exact_geometry(K_vga):
    """noise-free projections of known points (rounded to f32 pixels, as the library stores them): the model returns
    the points on the |t| = 1 scale, including one behind camera 1, and its mask is recoverPose's (in front of both
    cameras, closer than 50)"""
    rng = np.random.default_rng(4)
    th = np.radians(3.0)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    t = np.array([0.8, 0.1, 0.2]); t /= np.linalg.norm(t)
    X = np.column_stack([rng.uniform(-3, 3, 60), rng.uniform(-2, 2, 60), rng.uniform(4, 40, 60)])
    X[:5, 2] = rng.uniform(60, 90, 5)                                # beyond distanceThresh
    X[5] = [0.3, -0.2, -6.0]                                         # behind both cameras
    p1, p2, z2 = _project(X, R, t, K_vga)
    mask, P, near = sm.triangulate(R, t, p1.astype(np.float32), p2.astype(np.float32), K_vga)
    assert not near.any()
    want = (X[:, 2] > 0) & (X[:, 2] < sm.DIST) & (z2 > 0) & (z2 < sm.DIST)
    assert np.array_equal(mask, want) and want.sum() == 54
    assert np.allclose(P, X, rtol=2e-3, atol=0)


def test_model_count_equals_oracle_recover_pose(oracle, K_vga):
    """on the oracle's matched points and pose, the model's mask count is recoverPose's return value"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(4, K_vga, cfg=8)
    out, pts = oracle.estimate_pose_batch(i1, i2, K_vga, 1000, 500, return_points=True)
    for p in range(4):
        assert out[p]["status"] == 0
        n = int(out[p]["n_matches"]); p1, p2 = pts[p, 0, :n], pts[p, 1, :n]
        E, rmask, _ = oracle.find_essential(p1, p2, K_vga)
        cnt, R, t = oracle.recover_pose(E, p1, p2, K_vga)
        assert cnt == out[p]["inliers"] and np.array_equal(R.ravel(), out[p]["R"])
        mask, P, near = sm.triangulate(R, t, p1, p2, K_vga)
        assert mask.sum() == cnt and not near.any(), (p, mask.sum(), cnt)
        assert np.isfinite(P).all()


def test_model_depths_cluster_at_plane_depths(oracle, K_vga):
    """make_pair's planes at 4, 7, 12 with baseline 0.4 triangulate at 10, 17.5, 30 on the |t| = 1 scale"""
    from relative_pose_estimation_amd import synthetic, geometry
    Zs = []
    for seed in sm.PHYSICS_SEEDS:
        i1, i2, Rgt, _ = synthetic.make_pair(seed, K_vga, baseline=sm.PHYSICS_BASELINE)
        out, pts = oracle.estimate_pose_batch(i1[None], i2[None], K_vga, 1000, 500, return_points=True)
        n = int(out[0]["n_matches"])
        R, t = out[0]["R"].reshape(3, 3), out[0]["t"].reshape(3, 1)
        assert geometry.rotation_error(R, Rgt) < 0.3
        mask, P, _ = sm.triangulate(R, t, pts[0, 0, :n], pts[0, 1, :n], K_vga)
        assert mask.sum() == out[0]["inliers"]
        frac, _ = sm.depth_clusters(P[mask, 2], synthetic.DEPTHS)
        assert frac >= sm.DEPTH_BAND, (seed, frac)
        Zs.append(P[mask, 2])
    frac, per_plane = sm.depth_clusters(np.concatenate(Zs), synthetic.DEPTHS)
    assert frac >= sm.DEPTH_BAND and min(per_plane) >= 50, (frac, per_plane)


def test_structure_surface_exists():
    """the C-ABI entry point is exported and declared, and the Python surface binds it"""
    from relative_pose_estimation_amd import _capi, PoseEstimator
    assert "rpe_fetch_structure" in _capi.EXPORTS
    assert hasattr(_capi.load(), "rpe_fetch_structure")
    assert callable(getattr(_capi.Engine, "fetch_structure", None))
    assert callable(getattr(PoseEstimator, "estimate_with_structure", None))
    assert callable(getattr(PoseEstimator, "last_structure", None))
