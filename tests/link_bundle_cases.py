"""Inputs shared by test_link_bundle_cpu.py and test_gpu_link_bundle.py: link_pose_cases.hand_run extended so that pair a
carries noisy pixels on S and A, a perturbed pose and points triangulated from those pixels under that pose (as a real
run's are), and stage-form problems (rpe_bundle_three_view) of an exact point count built from the same kind of scene."""
import numpy as np

from tests import link_pose_cases as lc
from tests import link_pose_model as lp

NOISE_PX, OUTLIER_FRAC = lc.NOISE_PX, lc.OUTLIER_FRAC
COUNTS = lc.COUNTS[1:]                       # 6 and up
# perturbation of pair a's rotation and of its baseline direction: the median rotation error of the run's own five-point
# poses against ground truth (0.57 degrees on the benchmark's VGA pairs), so that pair a starts as far
# from the truth as a real run's pair does
POSE_NOISE_DEG = 0.57
STAGE_COUNTS = (6, 7, 255, 256, 257, 500)    # the lane-stride and wave-total edges


def _triangulate(R, t, xa, xb):
    """linear (DLT) triangulation of normalised observations xa (camera 1) and xb (camera 2 = R X + t), in camera 1's frame"""
    out = np.zeros((len(xa), 3))
    P2 = np.column_stack([R, t])
    for i in range(len(xa)):
        A = np.array([[1.0, 0, -xa[i, 0], 0], [0, 1.0, -xa[i, 1], 0], xb[i, 0] * P2[2] - P2[0], xb[i, 1] * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][-1]
        out[i] = v[:3] / v[3]
    return out


def _scene(rng, n):
    """the draws of link_pose_cases.hand_run, in its order: X in S's frame, (Ra, ta): S -> A, (Rc, tc): S -> C"""
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2.2, 2.2, n), rng.uniform(4, 14, n)])
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    Ra = lp.rodrigues(np.radians(3.0) * ax); ta = rng.normal(size=3); ta *= lc.BASE_A / np.linalg.norm(ta)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    Rc = lp.rodrigues(np.radians(4.0) * ax); tc = rng.normal(size=3); tc *= lc.BASE_C / np.linalg.norm(tc)
    return X, Ra, ta, Rc, tc


def _perturbed(rng, R, t, deg):
    """(R, t) turned by deg degrees about a random axis, t's direction by deg degrees, |t| kept"""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    Rn = lp.rodrigues(np.radians(deg) * ax) @ R
    ax = rng.normal(size=3); ax -= (ax @ t) * t / (t @ t); ax /= np.linalg.norm(ax)
    tn = lp.rodrigues(np.radians(deg) * ax) @ t
    return Rn, tn * (np.linalg.norm(t) / np.linalg.norm(tn))


def hand_run(n, side, K, seed=11, noise=NOISE_PX, outlier_frac=OUTLIER_FRAC, **kw):
    """link_pose_cases.hand_run with pair a made as noisy as pair b: f32 pixels with noise on S and A, pair a's pose perturbed
    by POSE_NOISE_DEG and its points triangulated from the noisy pixels under the perturbed pose (in its camera-1 frame,
    |t| = 1).  Returns (run, pts1, pts2, truth_a (R, t), truth_b (R, t) on pair a's TRUE scale, n_expected, outlier flags)."""
    run, p1, p2, truth_b, n_exp, out = lc.hand_run(n, side, K, seed=seed, noise=noise, outlier_frac=outlier_frac, **kw)
    K = np.asarray(K, np.float64)
    rng = np.random.default_rng(seed * 1000 + n)
    X, Ra, ta, _, _ = _scene(rng, n)
    rng.permutation(4 * n); rng.permutation(4 * n)                     # key, oth
    oa = rng.permutation(n)
    a2 = bool(side & 1)
    XA = X @ Ra.T + ta
    assert np.array_equal(run.points[0, :n], (XA if a2 else X)[oa] / lc.BASE_A), "link_pose_cases.hand_run draws differently"
    truth_a = (run.R[0].copy(), run.t[0].copy())
    r2 = np.random.default_rng(seed * 1000 + n + 500_000)
    pS = lc._project(X[oa], K, r2, noise); pA = lc._project(XA[oa], K, r2, noise)
    p1[0, :n], p2[0, :n] = (pA, pS) if a2 else (pS, pA)
    if noise:
        R0, t0 = _perturbed(r2, run.R[0], run.t[0], POSE_NOISE_DEG)
        x1, x2, _ = lp.observations(p1[:1], p2[:1], K)
        run.R[0], run.t[0] = R0, t0
        run.points[0, :n] = _triangulate(R0, t0, x1[0, :n], x2[0, :n])
        # a point behind either camera fails recoverPose's cheirality test: no pose_mask, as in a real run
        behind = (run.points[0, :n, 2] <= 0) | ((run.points[0, :n] @ R0[2] + t0[2]) <= 0)
        n_exp -= int((behind & run.ransac_mask[0, :n]).sum())
        run.pose_mask[0, :n] &= ~behind
        for d in range(run.points.shape[1] - n):                       # the duplicates of dup_a keep a wrong point
            if run.ransac_mask[0, n + d]:
                run.points[0, n + d] = run.points[0, d] * 3.0
    return run, p1, p2, truth_a, truth_b, n_exp, out


def stage_problem(n, n_c, seed=23, noise=NOISE_PX, f=500.0, spread=1.0):
    """a stage-form problem of exactly n points, the first n_c of a seeded permutation of them seen by C: dict obs (n, 6)
    normalised, hc, X0, RA, tA, RC, tC (the start state: truth with noise = 0, else perturbed poses and points triangulated
    from the noisy S and A observations), fa, fc, and truth.  spread < 1 pulls the points towards their centroid: a
    cluster in one corner of the image at nearly one depth, what the few strongest corners of a frame look like, and the
    weakest conditioning of the camera block"""
    rng = np.random.default_rng(seed * 1000 + n * 7 + n_c)
    X, Ra, ta, Rc, tc = _scene(rng, n)
    if spread != 1.0:
        X = X.mean(0) + spread * (X - X.mean(0)) + (1.0 - spread) * np.array([1.5, -1.0, 0.0])
    X = X / lc.BASE_A; ta = ta / lc.BASE_A; tc = tc / lc.BASE_A                                    # |tA| = 1
    proj = lambda Y: Y[:, :2] / Y[:, 2:3] + (rng.normal(scale=noise / f, size=(n, 2)) if noise else 0.0)
    obs = np.column_stack([proj(X), proj(X @ Ra.T + ta), proj(X @ Rc.T + tc)])
    hc = np.zeros(n, bool); hc[rng.permutation(n)[:n_c]] = True
    truth = dict(RA=Ra, tA=ta, RC=Rc, tC=tc, X=X)
    if not noise:
        return dict(obs=obs, hc=hc, X0=X.copy(), RA=Ra, tA=ta, RC=Rc, tC=tc, fa=f, fc=f, truth=truth)
    RA0, tA0 = _perturbed(rng, Ra, ta, POSE_NOISE_DEG)
    RC0, tC0 = _perturbed(rng, Rc, tc, POSE_NOISE_DEG)
    return dict(obs=obs, hc=hc, X0=_triangulate(RA0, tA0, obs[:, 0:2], obs[:, 2:4]), RA=RA0, tA=tA0, RC=RC0, tC=tC0 * 1.02, fa=f, fc=f,
                truth=truth)
