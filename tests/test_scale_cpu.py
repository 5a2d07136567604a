"""Scale links (rpe_scale_links / PoseEstimator.last_scale_links / estimate_trajectory): the float64 model of the join
and the order statistics (tests/scale_model.py) checked on CPU against exact geometry, its rules one by one,
geometry.chain_trajectory against known trajectories, and the physics band fixed from the CPU oracle."""
import hashlib

import numpy as np

from tests import scale_model as sc
from tests import structure_model as sm


def test_scale_surface_exists():
    """the two C-ABI entry points are exported and declared, and the Python surface binds them"""
    import inspect
    from relative_pose_estimation_amd import _capi, PoseEstimator, geometry, synthetic
    lib = _capi.load()
    for name in ("rpe_fetch_match_indices", "rpe_scale_links"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    assert (_capi.LINK_OK, _capi.LINK_PAIR_FAILED, _capi.LINK_TOO_FEW) == (0, 1, 2) == (sc.LINK_OK, sc.LINK_PAIR_FAILED, sc.LINK_TOO_FEW)
    for cls, names in ((_capi.Engine, ("fetch_match_indices", "scale_links")), (PoseEstimator, ("last_scale_links", "estimate_trajectory"))):
        for n in names:
            assert callable(getattr(cls, n, None)), n
    assert inspect.signature(_capi.Engine.scale_links).parameters["min_shared"].default == 8
    assert inspect.signature(PoseEstimator.last_scale_links).parameters["min_shared"].default == 8
    assert inspect.signature(PoseEstimator.estimate_trajectory).parameters["min_shared"].default == 8
    assert callable(getattr(geometry, "chain_trajectory", None)) and callable(getattr(synthetic, "stream_poses", None))


# ------------------------------------------------------------------ exact geometry
def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    th = np.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _project(X, R, T, K):
    Xc = X @ R.T + T
    return ((Xc[:, :2] / Xc[:, 2:3]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)


def _exact_run(Rs, cs, X, pairs, K):
    """Run over `pairs` of cameras X_c = Rs[i] (X_w - cs[i]) seeing the cloud X: every point is keypoint k of every
    frame and match k of every pair; f32 pixels triangulated by structure_model under the true unit-t pose"""
    n, P = len(X), len(pairs)
    idx = np.tile(np.arange(n, dtype=np.int32), (P, 1))
    rm = np.ones((P, n), bool); pm = np.zeros((P, n), bool); pts = np.zeros((P, n, 3))
    R = np.zeros((P, 3, 3)); t = np.zeros((P, 3)); base = np.zeros(P)
    for p, (i, j) in enumerate(pairs):
        Ti, Tj = -Rs[i] @ cs[i], -Rs[j] @ cs[j]
        R[p] = Rs[j] @ Rs[i].T
        tr = Tj - R[p] @ Ti
        base[p] = np.linalg.norm(tr)
        assert np.isclose(base[p], np.linalg.norm(cs[j] - cs[i]), rtol=1e-12)
        t[p] = tr / base[p]
        pm[p], pts[p], near = sm.triangulate(R[p], t[p], _project(X, Rs[i], Ti, K), _project(X, Rs[j], Tj, K), K)
        assert not near.any()
    return sc.Run(idx, idx, rm, pm, pts, R, t, np.zeros(P, np.int32), np.full(P, n, np.int32)), base


def test_model_on_exact_geometry(K_vga):
    """three cameras with known centres and one cloud: the median (and both quartiles) of every link is the true
    baseline ratio, for all four ways two pairs can share a frame.  rtol 2e-3: the f32 rounding of the pixels, the
    allowance test_structure_cpu.py::test_model_on_exact_geometry grants the same triangulation"""
    rng = np.random.default_rng(11)
    X = np.column_stack([rng.uniform(-2.5, 2.5, 80), rng.uniform(-1.8, 1.8, 80), rng.uniform(5, 14, 80)])
    Rs = [np.eye(3), _rot([0.2, 1, 0.1], 3.0), _rot([1, -0.3, 0.5], -2.5)]
    cs = [np.zeros(3), np.array([0.5, 0.05, 0.1]), np.array([0.2, -0.35, 0.45])]
    pairs = [(0, 1), (1, 2), (0, 2)]
    run, base = _exact_run(Rs, cs, X, pairs, K_vga)
    assert run.pose_mask.all()
    links = [(0, 2, 0),      # (0,1) and (0,2) at frame 0: image 1 of both
             (0, 1, 1),      # (0,1) and (1,2) at frame 1: image 2 of a, image 1 of b
             (1, 0, 2),      # (1,2) and (0,1) at frame 1: image 1 of a, image 2 of b
             (2, 1, 3)]      # (0,2) and (1,2) at frame 2: image 2 of both
    stats, n, code = sc.scale_links(run, links)
    assert (code == sc.LINK_OK).all() and (n == 80).all()
    truth = np.array([base[b] / base[a] for a, b, _ in links])
    assert len(set(np.round(truth, 3))) == 4
    assert np.allclose(stats, truth[:, None], rtol=2e-3, atol=0), (stats, truth)
    # a wrong side joins the wrong frame: the distances no longer belong to one camera centre
    wrong, _, _ = sc.scale_links(run, [(0, 1, 0)])
    assert not np.isclose(wrong[0, 1], truth[1], rtol=2e-3)


# ------------------------------------------------------------------ the rules, one by one
def _axis_run(values_a, keys_a, keys_b, usable_a=None, usable_b=None, status=(0, 0), side=0):
    """two pairs whose points lie on the optical axis: pair 0's match i at depth values_a[i], pair 1's at depth 1, R = I
    and t = 0, so whatever the side the ratio of a shared key is exactly the depth of pair 0's match"""
    na, nb = len(keys_a), len(keys_b)
    mm = max(na, nb, 1) + 3
    q = np.full((2, mm), -1, np.int32); rm = np.zeros((2, mm), bool); pts = np.zeros((2, mm, 3))
    q[0, :na] = keys_a; q[1, :nb] = keys_b
    rm[0, :na] = True if usable_a is None else usable_a
    rm[1, :nb] = True if usable_b is None else usable_b
    pts[0, :na, 2] = values_a; pts[1, :nb, 2] = 1.0
    R = np.tile(np.eye(3), (2, 1, 1)); t = np.zeros((2, 3))
    return sc.Run(q, q.copy(), rm, rm.copy(), pts, R, t, np.array(status, np.int32), np.array([na, nb], np.int32))


def test_order_statistic_ranks():
    """n = 1 .. 9 ratios in shuffled match order: the outputs are r[(n-1)/4], r[(n-1)/2], r[(3(n-1))/4] of the sorted
    ratios, exactly (elements of the set, never an average)"""
    rng = np.random.default_rng(3)
    want = {1: (0, 0, 0), 2: (0, 0, 0), 3: (0, 1, 1), 4: (0, 1, 2), 5: (1, 2, 3), 6: (1, 2, 3), 7: (1, 3, 4), 8: (1, 3, 5), 9: (2, 4, 6)}
    for n in range(1, 10):
        vals = np.sort(rng.uniform(0.5, 2.0, n))
        keys = rng.permutation(40)[:n]
        order = rng.permutation(n)
        run = _axis_run(vals[order], keys[order], rng.permutation(keys))
        for side in range(4):
            stats, ns, code = sc.scale_links(run, [(0, 1, side)], min_shared=1)
            assert ns[0] == n and code[0] == sc.LINK_OK
            assert tuple(stats[0]) == tuple(vals[list(want[n])]), (n, side)


def test_duplicate_keys_lowest_usable_index_wins():
    """several matches of one pair on one keypoint (RPE_MATCH_RATIO): the usable match with the lowest index represents
    the key, in pair a and in pair b alike; an unusable match with a lower index does not"""
    # pair a: key 7 at matches 0 (unusable), 1, 3; key 9 at match 2.   pair b: key 9 at 0, 2; key 7 at 1; key 4 at 3
    run = _axis_run([11., 12., 13., 14.], [7, 7, 9, 7], [9, 7, 9, 4], usable_a=[False, True, True, True])
    assert sc.usable_keys(run, 0, False) == {7: 1, 9: 2} and sc.usable_keys(run, 1, True) == {9: 0, 7: 1, 4: 3}
    assert sc.link_ratios(run, 0, 1, 0).tolist() == [12., 13.]                     # keys 7, 9
    stats, ns, code = sc.scale_links(run, [(0, 1, 0)], min_shared=1)
    assert ns[0] == 2 and tuple(stats[0]) == (12., 12., 12.)
    # the same with the roles exchanged: b's duplicates decide which of b's points divides
    run2 = _axis_run([1., 1., 1., 1.], [9, 7, 9, 4], [7, 7, 9, 7], usable_b=[False, True, True, True])
    run2.points[1, :4, 2] = [2., 4., 8., 16.]
    assert sc.link_ratios(run2, 0, 1, 0).tolist() == [1 / 4., 1 / 8.]              # keys 7 (b's match 1), 9 (b's match 2)
    stats, ns, code = sc.scale_links(run2, [(0, 1, 0)], min_shared=1)
    assert ns[0] == 2 and tuple(stats[0]) == (1 / 8., 1 / 8., 1 / 8.)


def test_too_few_and_pair_failed():
    vals = np.arange(1., 6.)
    run = _axis_run(vals, np.arange(5), np.arange(2, 9))                 # keys 2, 3, 4 shared
    stats, ns, code = sc.scale_links(run, [(0, 1, 0)] * 2, min_shared=3)
    assert ns[0] == 3 and code[0] == sc.LINK_OK and tuple(stats[0]) == (3., 4., 4.)
    stats, ns, code = sc.scale_links(run, [(0, 1, 0)], min_shared=4)     # min_shared = n_shared + 1
    assert ns[0] == 3 and code[0] == sc.LINK_TOO_FEW and not stats.any()
    none = _axis_run(vals, np.arange(5), np.arange(5, 9))
    stats, ns, code = sc.scale_links(none, [(0, 1, 0)], min_shared=1)
    assert ns[0] == 0 and code[0] == sc.LINK_TOO_FEW and not stats.any()
    for status in ((2, 0), (0, 3), (1, 1)):
        bad = _axis_run(vals, np.arange(5), np.arange(5), status=status)
        stats, ns, code = sc.scale_links(bad, [(0, 1, 0), (1, 0, 3)], min_shared=1)
        assert (code == sc.LINK_PAIR_FAILED).all() and not ns.any() and not stats.any()


# ------------------------------------------------------------------ chain_trajectory
def _walk(F, seed):
    rng = np.random.default_rng(seed)
    Rs = [_rot(rng.normal(size=3), rng.uniform(-8, 8)) for _ in range(F)]
    cs = np.cumsum(rng.normal(size=(F, 3)) * rng.uniform(0.2, 1.5, (F, 1)), 0)
    R_rel = np.stack([Rs[i + 1] @ Rs[i].T for i in range(F - 1)])
    t_rel = np.stack([-Rs[i + 1] @ cs[i + 1] + R_rel[i] @ Rs[i] @ cs[i] for i in range(F - 1)])
    base = np.linalg.norm(t_rel, axis=1)
    assert np.allclose(base, np.linalg.norm(np.diff(cs, axis=0), axis=1))
    return Rs, cs, R_rel, t_rel / base[:, None], base


def test_chain_trajectory_reproduces_known_centres():
    """exact relative poses and exact ratios give the known trajectory, in frame 0's coordinates and in units of the
    first baseline: the one global scale a monocular chain cannot know"""
    from relative_pose_estimation_amd import geometry
    F = 7
    Rs, cs, R_rel, t_rel, base = _walk(F, 5)
    ratio = base[1:] / base[:-1]
    R_abs, T_abs, centers, baseline, segment = geometry.chain_trajectory(R_rel, t_rel.reshape(-1, 3, 1), np.zeros(F - 1, np.int32), ratio, np.zeros(F - 2, np.int32))
    assert R_abs.shape == (F, 3, 3) and T_abs.shape == centers.shape == (F, 3) and baseline.shape == segment.shape == (F - 1,)
    assert not segment.any()
    assert np.allclose(baseline, base / base[0], rtol=1e-12)
    want = (cs - cs[0]) @ Rs[0].T / base[0]
    assert np.allclose(centers, want, rtol=0, atol=1e-12 * np.abs(want).max())
    for i in range(F):
        assert np.allclose(R_abs[i], Rs[i] @ Rs[0].T, atol=1e-12)
        assert np.allclose(centers[i], -R_abs[i].T @ T_abs[i], atol=1e-12)


def test_chain_trajectory_segments():
    """a failed pair and a failed link split the chain as specified; across the boundary the ratio is 1, a failed pair
    contributes the identity and a zero step"""
    from relative_pose_estimation_amd import geometry
    F = 7
    Rs, cs, R_rel, t_rel, base = _walk(F, 6)
    ratio = base[1:] / base[:-1]
    st = np.zeros(F - 1, np.int32); st[2] = 3
    R_abs, T_abs, centers, baseline, segment = geometry.chain_trajectory(R_rel, t_rel, st, ratio, np.zeros(F - 2, np.int32))
    assert segment.tolist() == [0, 0, 1, 2, 2, 2]
    assert np.allclose(baseline, [1, ratio[0], ratio[0], ratio[0], ratio[0] * ratio[3], ratio[0] * ratio[3] * ratio[4]], rtol=1e-12)
    assert np.array_equal(R_abs[3], R_abs[2]) and np.array_equal(T_abs[3], T_abs[2]) and np.allclose(centers[3], centers[2], atol=1e-15)
    # inside the last segment distances share its scale: consecutive centre distances are in the ratio of the baselines
    d = np.linalg.norm(np.diff(centers, axis=0), axis=1)
    assert np.allclose(d[4:] / d[3], base[4:] / base[3], rtol=1e-9)
    code = np.zeros(F - 2, np.int32); code[1] = sc.LINK_TOO_FEW; code[3] = sc.LINK_PAIR_FAILED
    junk = ratio.copy(); junk[1] = 0.0; junk[3] = 0.0                       # the stats of a failed link are zero
    _, _, centers, baseline, segment = geometry.chain_trajectory(R_rel, t_rel, np.zeros(F - 1, np.int32), junk, code)
    assert segment.tolist() == [0, 0, 1, 1, 2, 2]
    assert np.allclose(baseline, [1, ratio[0], ratio[0], ratio[0] * ratio[2], ratio[0] * ratio[2], ratio[0] * ratio[2] * ratio[4]], rtol=1e-12)
    assert np.isfinite(centers).all()


# ------------------------------------------------------------------ synthetic.stream_poses
def test_make_stream_is_stream_poses_rendered():
    """make_stream's relative poses are those of stream_poses' absolute ones, and its frames and poses are still the
    bits they were before stream_poses was split out of it (digest taken from the parent revision)"""
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(160, 120)
    kw = dict(seed=5_000_017, max_angle_deg=3.0, step=0.2)
    frames, R_rel, t_rel = synthetic.make_stream(5, K, 160, 120, **kw)
    Rs, ts = synthetic.stream_poses(5, **kw)
    assert Rs.shape == (5, 3, 3) and ts.shape == (5, 3) and np.array_equal(Rs[0], np.eye(3)) and not ts[0].any()
    c = -np.einsum("fji,fj->fi", Rs, ts)
    assert np.allclose(np.linalg.norm(np.diff(c, axis=0), axis=1), 0.2, rtol=1e-12)
    for i in range(4):
        assert np.array_equal(R_rel[i], Rs[i + 1] @ Rs[i].T)
        tr = ts[i + 1] - Rs[i + 1] @ Rs[i].T @ ts[i]
        assert np.allclose(t_rel[i].ravel(), tr / np.linalg.norm(tr), rtol=1e-14, atol=0)
    part = synthetic.make_stream(5, K, 160, 120, frame_range=(1, 4), **kw)
    assert np.array_equal(part[0], frames[1:4]) and np.array_equal(part[1], R_rel[1:3])
    digest = hashlib.sha256(frames.tobytes() + R_rel.tobytes() + t_rel.tobytes()).hexdigest()
    assert digest == MAKE_STREAM_DIGEST


MAKE_STREAM_DIGEST = "a81b8a2f977366a8d366f0e0469c22f202fc5dfb9989d411392f5f5448a3c6b4"


# ------------------------------------------------------------------ physics
def test_physics_with_the_oracle(oracle):
    """the PHYSICS stream through the CPU oracle (ORB -> match -> findEssentialMat -> recoverPose), structure_model and
    the scale model: every link has at least PHYSICS_MIN_SHARED shared keypoints and its median lies inside SCALE_BAND
    of the true baseline ratio (1 for consecutive pairs, stream_poses' centres for the skip-one links).  Prints the
    figures SCALE_BAND was fixed from."""
    frames, K = sc.physics_frames()
    pairs, links = sc.physics_pairs_and_links()
    run = sc.oracle_run(oracle, frames, pairs, K)
    assert not run.status.any()
    stats, n, code = sc.scale_links(run, links, sc.PHYSICS_MIN_SHARED)
    truth = sc.physics_truth(pairs, links)
    dev = np.abs(stats[:, 1] / truth - 1)
    for l, link in enumerate(links):
        print(f"link {link}: n_shared {n[l]} truth {truth[l]:.4f} median {stats[l, 1]:.4f} deviation {dev[l]:.4f}")
    assert np.allclose(truth[:len(pairs) - len(links) // 2 - 1], 1.0, rtol=1e-12)        # the consecutive links
    assert (code == sc.LINK_OK).all() and (n >= sc.PHYSICS_MIN_SHARED).all(), (n, code)
    assert sc.SCALE_BAND <= 0.25
    assert (dev <= sc.SCALE_BAND).all(), dev
