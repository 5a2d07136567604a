"""Float64 NumPy model of the homography RANSAC and the rotation fit (include/rpe_amd.h, rpe_pair_homographies /
rpe_find_homography).  Written from the rule in the header, in its operation order: every product and sum below is an
elementwise NumPy operation (a * b + c * d is two products and a sum, never fused; no BLAS `@` in the model, the
transfer test or the election), vectorised over the RANSAC iterations.  The subset table is the caller's
(oracle.ransac_subsets(M, iters)); only its first four columns are read.  The rotation fit uses np.linalg.svd: it
agrees with the library's Jacobi SVD to rounding, not to the bit."""
import numpy as np

HOMOGRAPHY_OK, HOMOGRAPHY_SKIPPED, HOMOGRAPHY_NONE = 0, 1, 2


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def adj(A):
    """A[r][c] -> rows cross(c1, c2), cross(c2, c0), cross(c0, c1) of the columns of A"""
    c = [(A[0][k], A[1][k], A[2][k]) for k in range(3)]
    return [cross(c[1], c[2]), cross(c[2], c[0]), cross(c[0], c[1])]


def _basis(p):
    """p[k] = (x, y, 1) of the four sample points -> (lambda, A): A has the columns lambda_k * p_k"""
    lam = (dot(cross(p[1], p[2]), p[3]), dot(cross(p[2], p[0]), p[3]), dot(cross(p[0], p[1]), p[3]))
    A = [[lam[k] * p[k][r] for k in range(3)] for r in range(3)]
    return lam, A


def _w(F, x, y):
    return (F[2][0] * x + F[2][1] * y) + F[2][2]


def four_point(P, Q):
    """P, Q: (n, 4, 2) sample points of n iterations -> (H[3][3], G[3][3], valid), each entry an (n,) array"""
    P = np.asarray(P, np.float64); Q = np.asarray(Q, np.float64)
    one = np.ones(P.shape[0])
    p = [(P[:, k, 0], P[:, k, 1], one) for k in range(4)]
    q = [(Q[:, k, 0], Q[:, k, 1], one) for k in range(4)]
    with np.errstate(all="ignore"):
        lam, A = _basis(p)
        mu, B = _basis(q)
        J = adj(A)
        H = [[(B[r][0] * J[0][c] + B[r][1] * J[1][c]) + B[r][2] * J[2][c] for c in range(3)] for r in range(3)]
        s = None
        for r in range(3):
            for c in range(3):
                s = H[r][c] * H[r][c] if s is None else s + H[r][c] * H[r][c]
        n = np.sqrt(s)
        H = [[H[r][c] / n for c in range(3)] for r in range(3)]
        valid = np.ones(P.shape[0], bool)
        for k in range(3):
            valid &= (lam[k] != 0) & (mu[k] != 0)
        for r in range(3):
            for c in range(3):
                valid &= np.isfinite(H[r][c])
        neg = _w(H, p[0][0], p[0][1]) < 0
        H = [[np.where(neg, -H[r][c], H[r][c]) for c in range(3)] for r in range(3)]
        G = adj(H)
        neg = _w(G, q[0][0], q[0][1]) < 0
        G = [[np.where(neg, -G[r][c], G[r][c]) for c in range(3)] for r in range(3)]
    return H, G, valid


def transfer(F, px, py, qx, qy, thr2):
    """T(F, p -> q); the entries of F and the coordinates broadcast against each other"""
    with np.errstate(all="ignore"):
        u = (F[0][0] * px + F[0][1] * py) + F[0][2]
        v = (F[1][0] * px + F[1][1] * py) + F[1][2]
        w = (F[2][0] * px + F[2][1] * py) + F[2][2]
        dx = u - qx * w
        dy = v - qy * w
        return (w > 0) & ((dx * dx + dy * dy) <= thr2 * (w * w))


def inliers(H, G, a, b, thr2):
    """H, G with (n,) entries against M matches -> (n, M) bool"""
    Hc = [[H[r][c][:, None] for c in range(3)] for r in range(3)]
    Gc = [[G[r][c][:, None] for c in range(3)] for r in range(3)]
    ax, ay, bx, by = a[None, :, 0], a[None, :, 1], b[None, :, 0], b[None, :, 1]
    return transfer(Hc, ax, ay, bx, by, thr2) & transfer(Gc, bx, by, ax, ay, thr2)


def rotation_count(R, a, b, thr2):
    """n_rot and its mask for a given R_rot: T(R, a -> b) and T(R^T, b -> a), no gauge"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    F = [[R[r, c] for c in range(3)] for r in range(3)]
    Ft = [[R[c, r] for c in range(3)] for r in range(3)]
    m = transfer(F, a[:, 0], a[:, 1], b[:, 0], b[:, 1], thr2) & transfer(Ft, b[:, 0], b[:, 1], a[:, 0], a[:, 1], thr2)
    return int(m.sum()), m


def bearings(x):
    n = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + 1)
    return np.stack([x[:, 0] / n, x[:, 1] / n, 1 / n], 1)


def rotation_fit(a, b, mask):
    """R_rot = U diag(1, 1, det(U V^T)) V^T of C = sum b^ a^T over the masked matches (LAPACK's SVD)"""
    ah, bh = bearings(a[mask]), bearings(b[mask])
    C = np.einsum("ir,ic->rc", bh, ah)
    U, _, Vt = np.linalg.svd(C)
    return U @ np.diag([1., 1., np.linalg.det(U @ Vt)]) @ Vt


def find_homography(a, b, subsets, thr2, skipped=False):
    """a, b: (M, 2) f64 normalised points; subsets: (iters, >= 4) ints, the rows of the RANSAC subset stream of M.
    Returns a dict: code, H (3, 3), mask (M,) bool, n_H, n_rot, R_rot (3, 3), it (winning iteration), n_valid."""
    a = np.asarray(a, np.float64).reshape(-1, 2); b = np.asarray(b, np.float64).reshape(-1, 2)
    M = len(a)
    out = dict(code=HOMOGRAPHY_SKIPPED, H=np.zeros((3, 3)), mask=np.zeros(M, bool), n_H=0, n_rot=0, R_rot=np.zeros((3, 3)),
               it=0, n_valid=0)
    if skipped or M < 6:
        return out
    idx = np.asarray(subsets)[:, :4].astype(np.int64)
    H, G, valid = four_point(a[idx], b[idx])
    inl = inliers(H, G, a, b, thr2)
    cnt = np.where(valid, inl.sum(1), -1)
    out["n_valid"] = int(valid.sum())
    if not valid.any():
        out["code"] = HOMOGRAPHY_NONE
        out["n_valid"] = 0
        return out
    it = int(np.argmax(cnt))                                 # the first maximum: ties go to the lowest iteration
    out.update(code=HOMOGRAPHY_OK, it=it, n_H=int(cnt[it]), mask=inl[it].copy(),
               H=np.array([[H[r][c][it] for c in range(3)] for r in range(3)]))
    with np.errstate(all="ignore"):
        R = rotation_fit(a, b, out["mask"]) if out["n_H"] > 0 else np.full((3, 3), np.nan)
    if np.isfinite(R).all():
        out["R_rot"] = R
        out["n_rot"] = rotation_count(R, a, b, thr2)[0]
    return out


def rotation_angle_deg(Ra, Rb):
    """geodesic angle between two rotations, from the skew part for small angles (arccos loses them below 1e-6 deg)"""
    D = np.asarray(Ra) @ np.asarray(Rb).T
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    c = (np.trace(D) - 1) / 2
    return float(np.rad2deg(np.arctan2(s, c)))
