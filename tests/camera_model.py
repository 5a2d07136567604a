"""float64 numpy model of the camera path (include/rpe_amd.h, "camera models"): cv2's Brown-Conrady / rational lens, the
fixed-count undistortion the library runs, the normalisation of f32 pixels and the Sampson inlier test on normalised
points with the mean-focal threshold.  cv2 is not available to the tests, so this file is the specification: the library
reproduces its operation order (the build has no floating-point contraction).  Used by test_camera_cpu.py and
test_gpu_camera.py."""
import numpy as np

UNDISTORT_ITERS = 5            # RPE_UNDISTORT_ITERS

# the two lenses of the accuracy table (k1, k2, p1, p2, k3) and one that also sets the rational terms k4..k6
MILD = (-0.12, 0.03, 0.0008, -0.0005, 0.0)
STRONG = (-0.28, 0.09, 0.001, -0.0008, -0.01)
RATIONAL = (-0.20, 0.05, 0.0006, -0.0004, 0.002, 0.03, -0.01, 0.001)
# CPU reference for the 16 strong-lens pairs of the accuracy table: median rotation error in degrees ignoring the lens /
# with the matched points undistorted first (asserted by test_camera_cpu.py, used by test_gpu_camera.py)
CPU_STRONG_MEDIAN_ROT = (2.038, 0.548)


class Cam:
    """fx, fy, cx, cy of K (skew ignored) and dist padded to cv2's eight coefficients k1 k2 p1 p2 k3 k4 k5 k6"""

    def __init__(self, K, dist=None):
        K = np.asarray(K, np.float64)
        self.fx, self.fy, self.cx, self.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).reshape(-1)
        self.dist = np.zeros(8)
        self.dist[:d.size] = d

    @property
    def K(self):
        return np.array([[self.fx, 0., self.cx], [0., self.fy, self.cy], [0., 0., 1.]])

    @property
    def focal(self):
        return (self.fx + self.fy) / 2


def distort(x, y, dist):
    """ideal normalised (x, y) -> distorted normalised (xd, yd): cv2.projectPoints' lens"""
    k1, k2, p1, p2, k3, k4, k5, k6 = np.asarray(dist, np.float64)
    r2 = x * x + y * y
    cd = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return x * cd + dx, y * cd + dy


def undistort(xd, yd, dist, iters=UNDISTORT_ITERS):
    """cv2.undistortPoints' fixed-point iteration started at (xd, yd), `iters` rounds, in the library's operation order"""
    k1, k2, p1, p2, k3, k4, k5, k6 = np.asarray(dist, np.float64)
    xd = np.asarray(xd, np.float64); yd = np.asarray(yd, np.float64)
    x, y = xd, yd
    for _ in range(iters):
        r2 = x * x + y * y
        icd = (1 + r2 * (k4 + r2 * (k5 + r2 * k6))) / (1 + r2 * (k1 + r2 * (k2 + r2 * k3)))
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (xd - dx) * icd
        y = (yd - dy) * icd
    return x, y


def normalise(pts_f32, cam, iters=UNDISTORT_ITERS):
    """(n, 2) f32 pixels -> (n, 2) f64 normalised, undistorted coordinates; a camera without a lens skips the iteration"""
    p = np.asarray(pts_f32, np.float32).astype(np.float64).reshape(-1, 2)
    xd = (p[:, 0] - cam.cx) / cam.fx
    yd = (p[:, 1] - cam.cy) / cam.fy
    if not np.any(cam.dist != 0.):
        return np.stack([xd, yd], 1)
    x, y = undistort(xd, yd, cam.dist, iters)
    return np.stack([x, y], 1)


def to_pixels(xy, cam):
    """normalised coordinates -> ideal pinhole pixels of the camera (f64)"""
    return np.stack([xy[:, 0] * cam.fx + cam.cx, xy[:, 1] * cam.fy + cam.cy], 1)


def pair_focal(cam1, cam2):
    """the focal length a pair uses as a scale: the mean of the two cameras' (fx + fy) / 2"""
    return (((cam1.fx + cam1.fy) / 2) + ((cam2.fx + cam2.fy) / 2)) / 2


def sampson(E, x1, x2):
    """Sampson error (f64) of normalised points under E: findEssentialMat's computeError"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    a = np.hstack([x1, np.ones((len(x1), 1))]); b = np.hstack([x2, np.ones((len(x2), 1))])
    Ex1 = a @ E.T
    Etx2 = b @ E
    num = np.sum(b * Ex1, 1) ** 2
    den = Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den


def sampson_mask(E, x1, x2, threshold, focal, rel=1e-9):
    """(mask bool[n], near bool[n]): err <= (threshold / focal)^2 compared as findEssentialMat compares it (both sides
    rounded to f32), and whether the error lies within a relative `rel` of the threshold, where another operation order
    may legitimately decide the other way.  The f32 comparison puts the decision point of the f64 error half an f32 ulp
    above the f32 threshold (round to nearest), so `near` is measured against both values."""
    err = sampson(E, x1, x2)
    thr = threshold / focal
    thr2 = np.float32(thr * thr)
    mask = err.astype(np.float32) <= thr2
    mid = 0.5 * (float(thr2) + float(np.nextafter(thr2, np.float32(np.inf))))
    near = (np.abs(err - float(thr2)) <= rel * float(thr2)) | (np.abs(err - mid) <= rel * mid)
    return mask, near


def triangulate(R, t, x1, x2, DIST=50.0):
    """tests/structure_model.triangulate for points that are normalised already (f64, no K): (mask bool[n], points
    f64[n, 3], near bool[n]) with the same `near` rule"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    n = len(x1)
    P1 = np.hstack([R, t[:, None]])
    A = np.zeros((n, 4, 4))
    A[:, 0] = [-1., 0., 0., 0.]; A[:, 0, 2] = x1[:, 0]
    A[:, 1] = [0., -1., 0., 0.]; A[:, 1, 2] = x1[:, 1]
    A[:, 2] = x2[:, 0:1] * P1[2] - P1[0]
    A[:, 3] = x2[:, 1:2] * P1[2] - P1[1]
    Q = np.linalg.svd(A)[2][:, 3, :] if n else np.zeros((0, 4))
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
