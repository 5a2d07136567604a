"""float64 numpy model of what cv2.recoverPose(E, p1, p2, K, distanceThresh) returns per match: triangulatePoints'
DLT with P0 = [I|0], P1 = [R|t] (null vector from np.linalg.svd), the cheirality mask and the dehomogenised point.
Independent of the library's Jacobi SVD; used by test_structure_cpu.py and test_gpu_structure.py."""
import numpy as np

DIST = 50.0      # the reference's 4-argument recoverPose call leaves distanceThresh at 50


def normalise(pts, K):
    """pixel points (f32) -> normalised camera coordinates, in recoverPose's order ((p - c) / f in f64)"""
    p = np.asarray(pts, np.float32).astype(np.float64)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], 1)


def triangulate(R, t, pts1, pts2, K):
    """(mask bool[n], points f64[n, 3], near bool[n]): recoverPose's cheirality mask, the point (X/W, Y/W, Z/W) in the
    camera-1 frame for every match, and whether the point lies within a relative 1e-9 of one of the mask's thresholds
    (where another SVD may legitimately decide the other way)."""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64)
    x1 = normalise(pts1, K); x2 = normalise(pts2, K)
    n = len(x1)
    P1 = np.hstack([R, t[:, None]])
    A = np.zeros((n, 4, 4))
    A[:, 0] = [-1., 0., 0., 0.]; A[:, 0, 2] = x1[:, 0]
    A[:, 1] = [0., -1., 0., 0.]; A[:, 1, 2] = x1[:, 1]
    A[:, 2] = x2[:, 0:1] * P1[2] - P1[0]
    A[:, 3] = x2[:, 1:2] * P1[2] - P1[1]
    Q = np.linalg.svd(A)[2][:, 3, :] if n else np.zeros((0, 4))    # right singular vector of the smallest singular value
    with np.errstate(divide="ignore", invalid="ignore"):
        front = Q[:, 2] * Q[:, 3] > 0
        X = Q[:, :3] / Q[:, 3:4]
        z2 = X @ R[2] + t[2]
        mask = front & (X[:, 2] < DIST) & (z2 > 0) & (z2 < DIST)
        scale = np.maximum(1.0, np.linalg.norm(X, axis=1))
        eps = 1e-9
        near = ((np.abs(X[:, 2]) <= eps * scale) | (np.abs(X[:, 2] - DIST) <= eps * DIST)
                | (np.abs(z2) <= eps * scale) | (np.abs(z2 - DIST) <= eps * DIST) | ~np.isfinite(X).all(1))
    return mask, X, near


# Physics check on synthetic.make_pair scenes (planes at DEPTHS in the camera-1 frame, baseline 0.4): on the |t| = 1 scale a
# pose inlier on plane k triangulates at DEPTHS[k] / 0.4 = 10, 17.5, 30.  How close depends on the pose's accuracy (a 1-degree
# rotation error moves the far plane by a third), so the scenes are seeds whose estimated rotation is within 0.3 degrees of
# the truth.  Fixed from the CPU oracle (test_structure_cpu.py): 90.4 / 91.6 / 93.6 % of their inlier depths lie within 15 %
# of a plane depth, every plane is populated.
PHYSICS_SEEDS = (7_000_004, 7_000_007, 7_000_008)
PHYSICS_BASELINE = 0.4
DEPTH_TOL = 0.15
DEPTH_BAND = 0.85


def depth_clusters(Z, depths, baseline=PHYSICS_BASELINE, tol=DEPTH_TOL):
    """(fraction of depths within tol of a plane depth / baseline, count per plane)"""
    D = np.asarray(depths, np.float64) / baseline
    rel = np.abs(np.asarray(Z, np.float64)[:, None] / D - 1)
    hit = rel.min(1) < tol
    k = rel.argmin(1)
    return float(hit.mean()), [int(((k == j) & hit).sum()) for j in range(len(D))]
