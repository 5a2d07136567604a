"""float64 model of rpe_link_poses, written from the rule in include/rpe_amd.h ("link poses"): per link a join of pair
a's usable matches and all of pair b's matches on the keypoint index of the shared frame (plain dicts), the
correspondences in the order of pair b's match index, P3P over the first three indices of the subset stream
(oracle.ransac_subsets(n, iters)), the score, the election and the Levenberg-Marquardt polish.  Independent of the kernel's
LDS table, scans and rounds.  The minimal solver runs on Python floats (IEEE doubles, one rounding per operation, in the
header's order) and the score on numpy arrays (elementwise, never fused), so with refine_iters = 0 the model's R and t
are the library's bits; the polish forms its residuals, its Cholesky solve and its rotation update in the library's
operation order too and sums with np.sum, so it differs from the library by the order of the sums alone -- what
reduction_margin() measures on the model itself.  The real-root finder restates the library's derivative chain (oracle/geom_oracle.c
poly_real_roots, which is not exported).  Used by test_link_pose_cpu.py and test_gpu_link_pose.py."""
import math

import numpy as np

from tests import camera_model as cm
from tests import scale_model as sc
from tests import structure_model as sm
from tests.bundle_math_model import SUMS, lm_loop, rodrigues, rot_angle_deg, rotate, solve, step_norm  # noqa: F401
from tests.bundle_math_model import dot3 as _dot, fdiv as _div, finite as _finite, fsqrt as _sqrt

LINKPOSE_OK, LINKPOSE_PAIR_FAILED, LINKPOSE_TOO_FEW, LINKPOSE_NONE = 0, 1, 2, 3


# ---------------------------------------------------------------- real roots (the library's derivative chain)
def _estrin(c, n, x):
    cc = [c[i] if i <= n else 0.0 for i in range(11)]
    x2 = x * x; x4 = x2 * x2; x8 = x4 * x4
    a0 = cc[0] + cc[1] * x; a1 = cc[2] + cc[3] * x; a2 = cc[4] + cc[5] * x
    a3 = cc[6] + cc[7] * x; a4 = cc[8] + cc[9] * x; a5 = cc[10]
    b0 = a0 + a1 * x2; b1 = a2 + a3 * x2; b2 = a4 + a5 * x2
    return (b0 + b1 * x4) + b2 * x8


def _ilogb(v):
    return math.frexp(v)[1] - 1


def _root_bound(p, k):
    ek = _ilogb(p[k])
    emax = None
    for i in range(k):
        if p[i] == 0.0:
            continue
        d = _ilogb(p[i]) - ek + 1; m = k - i
        q = (d + m - 1) // m if d >= 0 else -((-d) // m)
        if emax is None or q > emax:
            emax = q
    R = 1.0 if emax is None else math.ldexp(1.0, emax + 1)
    return R if R < 1e12 else 1e12


def _refine_root(p, dp, k, a, b, sa):
    xl, xh = (b, a) if sa else (a, b)
    rts = 0.5 * (a + b)
    dxold = abs(b - a); dx = dxold
    f = _estrin(p, k, rts); df = _estrin(dp, k - 1, rts)
    for _ in range(100):
        bis = ((((rts - xh) * df - f) * ((rts - xl) * df - f)) > 0.0) or (abs(2.0 * f) > abs(dxold * df))
        dxold = dx
        if bis:
            dx = 0.5 * (xh - xl); nr = xl + dx
        else:
            dx = _div(f, df); nr = rts - dx
        if nr == rts or abs(nr - rts) <= 2.3e-13 * abs(nr):
            rts = nr
            break
        rts = nr
        f = _estrin(p, k, rts); df = _estrin(dp, k - 1, rts)
        if f > 0.0:
            xh = rts
        else:
            xl = rts
    return rts


def real_roots(c):
    """ascending real roots of c[0] + c[1] x + ... (degree = the highest non-zero coefficient; [] for degree < 1)"""
    c = [float(v) for v in c]
    n = len(c) - 1
    while n >= 0 and c[n] == 0.0:
        n -= 1
    if n < 1:
        return []
    d = {n: c[:n + 1]}
    for k in range(n, 1, -1):
        d[k - 1] = [d[k][i + 1] * float(i + 1) for i in range(k)]
    prev = [_div(-d[1][0], d[1][1])]
    for k in range(2, n + 1):
        p, dp = d[k], d[k - 1]
        R = _root_bound(p, k)
        out = []
        for iv in range(len(prev) + 1):
            a = -R if iv == 0 else prev[iv - 1]
            b = R if iv == len(prev) else prev[iv]
            if a < -R:
                a = -R
            if b > R:
                b = R
            if not a < b:
                continue
            sa = _estrin(p, k, a) > 0.0; sb = _estrin(p, k, b) > 0.0
            if sa == sb:
                continue
            out.append(_refine_root(p, dp, k, a, b, sa))
        prev = out
    return prev


# ---------------------------------------------------------------- the minimal solver
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _frame(A1, A2, A3):
    d = _sub(A2, A1); w = _sub(A3, A1)
    nd = _sqrt(_dot(d, d))
    e1 = tuple(_div(v, nd) for v in d)
    c = _cross(e1, w)
    nc = _sqrt(_dot(c, c))
    e3 = tuple(_div(v, nc) for v in c)
    return e1, _cross(e3, e1), e3


def quartic(P, q):
    """the header's bearings, lengths, cosines and coefficients: dict j (three bearings), b2, q1, n, d, c (five)"""
    j = []
    for x, y in q:
        m = _sqrt((x * x + y * y) + 1.0)
        j.append((x / m, y / m, 1.0 / m))
    P1, P2, P3 = P
    d23 = _sub(P2, P3); d13 = _sub(P1, P3); d12 = _sub(P1, P2)
    a2 = _dot(d23, d23); b2 = _dot(d13, d13); c2 = _dot(d12, d12)
    ca = _dot(j[1], j[2]); cb = _dot(j[0], j[2]); cg = _dot(j[0], j[1])
    q1 = -(2.0 * cb); m = a2 - c2
    n0 = b2 + m; n1 = m * q1; n2 = m - b2
    d0 = (2.0 * b2) * cg; d1 = -((2.0 * b2) * ca)
    nn = (n0 * n0, 2.0 * (n0 * n1), 2.0 * (n0 * n2) + n1 * n1, 2.0 * (n1 * n2), n2 * n2)
    nd = (n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1)
    dd = (d0 * d0, 2.0 * (d0 * d1), d1 * d1)
    w0 = b2 - c2; w1 = -(c2 * q1); w2 = -c2
    wd = (w0 * dd[0], w0 * dd[1] + w1 * dd[0], (w0 * dd[2] + w1 * dd[1]) + w2 * dd[0], w1 * dd[2] + w2 * dd[1], w2 * dd[2])
    c = [(b2 * nn[i] - d0 * nd[i]) + wd[i] for i in range(4)] + [b2 * nn[4] + wd[4]]
    return dict(j=j, b2=b2, q1=q1, n=(n0, n1, n2), d=(d0, d1), c=c)


def pose_of_root(P, g, v):
    """(R 3x3, t 3) of root v, or None when v is no candidate"""
    n0, n1, n2 = g["n"]; d0, d1 = g["d"]
    Dv = d0 + d1 * v; Nv = (n0 + n1 * v) + n2 * (v * v); Qv = (1.0 + g["q1"] * v) + v * v
    u = _div(Nv, Dv)
    if not (v > 0.0 and Dv != 0.0 and u > 0.0 and Qv > 0.0):
        return None
    s1 = _sqrt(_div(g["b2"], Qv)); s = (s1, u * s1, v * s1)
    Y = [tuple(s[k] * g["j"][k][i] for i in range(3)) for k in range(3)]
    e = _frame(*P); f = _frame(*Y)
    R = [[(f[0][r] * e[0][c] + f[1][r] * e[1][c]) + f[2][r] * e[2][c] for c in range(3)] for r in range(3)]
    t = [Y[0][r] - ((R[r][0] * P[0][0] + R[r][1] * P[0][1]) + R[r][2] * P[0][2]) for r in range(3)]
    if not all(_finite(v) for row in R for v in row) or not all(_finite(v) for v in t):
        return None
    return np.array(R), np.array(t)


def p3p(P, q):
    """the candidates of one sample: [(root index, R, t)] in root order.  P: three 3D points, q: three normalised
    observations"""
    P = [tuple(float(v) for v in p) for p in P]; q = [tuple(float(v) for v in p) for p in q]
    g = quartic(P, q)
    out = []
    for r, v in enumerate(real_roots(g["c"])):
        cand = pose_of_root(P, g, v)
        if cand is not None:
            out.append((r, cand[0], cand[1]))
    return out


# ---------------------------------------------------------------- score
def inlier_mask(R, t, X, q, thr2):
    y0 = ((R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1]) + R[0, 2] * X[:, 2]) + t[0]
    y1 = ((R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1]) + R[1, 2] * X[:, 2]) + t[1]
    y2 = ((R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1]) + R[2, 2] * X[:, 2]) + t[2]
    dx = y0 - q[:, 0] * y2; dy = y1 - q[:, 1] * y2
    with np.errstate(invalid="ignore", over="ignore"):
        return (y2 > 0.0) & ((dx * dx + dy * dy) <= thr2 * (y2 * y2))


# ---------------------------------------------------------------- polish
def residuals(R, t, X, q, scale, jac=False):
    """r (m, 2) in pixels and, with jac, J (m, 2, 6): columns w0 w1 w2 (R <- exp([w]x) R), d0 d1 d2 (t <- t + d)"""
    a = np.stack([(R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1]) + R[k, 2] * X[:, 2] for k in range(3)], 1)   # the score's row order
    y = a + t
    u = y[:, :2] / y[:, 2:3]
    r = scale * (u - q)
    if not jac:
        return r
    m = len(X)
    s = scale / y[:, 2]
    dy = np.zeros((m, 3, 6))                   # d y / d w_k = e_k x a, d y / d d = I
    dy[:, 1, 0] = -a[:, 2]; dy[:, 2, 0] = a[:, 1]
    dy[:, 0, 1] = a[:, 2]; dy[:, 2, 1] = -a[:, 0]
    dy[:, 0, 2] = -a[:, 1]; dy[:, 1, 2] = a[:, 0]
    dy[:, 0, 3] = dy[:, 1, 4] = dy[:, 2, 5] = 1.0
    J = s[:, None, None] * (dy[:, :2, :] - u[:, :, None] * dy[:, 2:3, :])
    return r, J


def lm(R0, t0, X, q, scale, max_iters, order="forward"):
    """the iteration over the fixed set (X, q): dict R, t, cost0, cost, iters, accepted, decisions"""
    S = SUMS[order]
    R = np.array(R0, np.float64); t = np.array(t0, np.float64)
    lin = residuals(R, t, X, q, scale, True)           # (r, J) of the state; None once the state has moved
    cost0 = float(S((lin[0] * lin[0]).sum(1)))
    out = dict(R=R, t=t, cost0=cost0, cost=cost0, iters=0, accepted=0, decisions=[])
    if not np.isfinite(cost0):
        return out
    iu = np.triu_indices(6)
    d = new = None

    def step(lam):
        nonlocal lin, d
        if lin is None:
            lin = residuals(R, t, X, q, scale, True)
        r, J = lin
        H = np.zeros((6, 6))
        H[iu] = S((J[:, :, iu[0]] * J[:, :, iu[1]]).sum(1))
        H = np.triu(H) + np.triu(H, 1).T
        d = solve(H, S((J * r[:, :, None]).sum(1)), lam)
        return d is not None

    def trial(lam):
        nonlocal new
        new = (rotate(d[:3], R), t + d[3:])
        rn = residuals(new[0], new[1], X, q, scale)
        return float(S((rn * rn).sum(1)))

    def accept():
        nonlocal R, t, lin
        (R, t), lin = new, None

    cost, iters, acc, dec = lm_loop(cost0, max_iters, step, trial, lambda: step_norm(d), accept)
    out.update(R=R, t=t, cost=cost, iters=iters, accepted=acc, decisions=dec)
    return out


# ---------------------------------------------------------------- one link
def observations(pts1, pts2, K=None, cams=None):
    """(x1, x2 f64[P, mm, 2], focal f64[P]): the matched pixels (rpe_fetch_matched_points) normalised as the geometry stages
    normalise them -- with K, or per pair with its two camera_model.Cam (cams[p] = (cam1, cam2)) -- and the focal scale"""
    P = len(pts1)
    x1 = np.zeros((P,) + np.asarray(pts1[0]).shape, np.float64); x2 = np.zeros_like(x1); focal = np.zeros(P)
    for p in range(P):
        if cams is None:
            Kd = np.asarray(K, np.float64)
            x1[p] = sm.normalise(pts1[p], Kd); x2[p] = sm.normalise(pts2[p], Kd)
            focal[p] = (Kd[0, 0] + Kd[1, 1]) / 2
        else:
            x1[p] = cm.normalise(pts1[p], cams[p][0]); x2[p] = cm.normalise(pts2[p], cams[p][1])
            focal[p] = cm.pair_focal(*cams[p])
    return x1, x2, focal


def map_point(run, pair, i, image2):
    """match i's triangulated point in the camera frame of the pair's image 1 / image 2 ("scale links" expression)"""
    X, Y, Z = (float(v) for v in run.points[pair, i])
    if not image2:
        return X, Y, Z
    R, t = run.R[pair], run.t[pair]
    return tuple(((float(R[r, 0]) * X + float(R[r, 1]) * Y) + float(R[r, 2]) * Z) + float(t[r]) for r in range(3))


def correspondences(run, x1, x2, a, b, side):
    """(X f64[n, 3], q f64[n, 2], idx i32[n]) in ascending order of pair b's match index; None when pair a failed"""
    if run.status[a] != 0:
        return None
    a2, b2 = bool(side & 1), bool(side & 2)
    ka = sc.usable_keys(run, a, a2)
    kidx = run.tidx[b] if b2 else run.qidx[b]
    nb = min(int(run.n_matches[b]), kidx.shape[0])
    first = {}
    for i in range(nb):
        first.setdefault(int(kidx[i]), i)
    obs = x1[b] if b2 else x2[b]
    X, q, idx = [], [], []
    for i in range(nb):
        key = int(kidx[i])
        if first[key] == i and key in ka:
            X.append(map_point(run, a, ka[key], a2)); q.append(obs[i]); idx.append(i)
    return np.array(X, np.float64).reshape(-1, 3), np.array(q, np.float64).reshape(-1, 2), np.array(idx, np.int32)


def link_pose(run, x1, x2, focal, link, subsets, iters=256, threshold_px=1.0, min_shared=8, refine_iters=10, order="forward"):
    """one link (a, b, side) as the library returns it: dict code, n, R (3, 3), t (3,), mask bool[mm], counts (2), info
    (4), rms (2), decisions.  subsets(n, iters) -> i32[iters, 5] (oracle.ransac_subsets)."""
    a, b, side = (int(v) for v in link)
    mm = run.qidx.shape[1]
    res = dict(code=LINKPOSE_OK, n=0, R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(mm, bool), counts=(0, 0),
               info=(0, 0, 0, 0), rms=(0.0, 0.0), decisions=[])

    def ended(code, n):
        res.update(code=code, n=n, counts=(n, 0), info=(code, 0, 0, 0))
        return res

    cor = correspondences(run, x1, x2, a, b, side)
    if cor is None:
        return ended(LINKPOSE_PAIR_FAILED, 0)
    X, q, idx = cor
    n = len(idx)
    if n < max(min_shared, 6):
        return ended(LINKPOSE_TOO_FEW, n)
    scale = float(focal[b])
    thr = threshold_px / scale
    thr2 = thr * thr
    sub = np.asarray(subsets(n, iters))[:iters, :3]
    best = None                                            # (count, iteration, root, R, t, inliers)
    for it in range(iters):
        s = sub[it]
        for r, R, t in p3p(X[s], q[s]):
            inl = inlier_mask(R, t, X, q, thr2)
            c = int(inl.sum())
            if best is None or c > best[0]:
                best = (c, it, r, R, t, inl)
    if best is None:
        return ended(LINKPOSE_NONE, n)
    cnt, it, r, R, t, inl = best
    m = int(inl.sum())
    polish = 0
    o = lm(R, t, X[inl], q[inl], scale, refine_iters, order)
    before = float(np.sqrt(o["cost0"] / m)) if m > 0 else 0.0
    after = before
    res["decisions"] = o["decisions"]
    if o["accepted"] > 0:
        fin = bool(np.isfinite(o["R"]).all() and np.isfinite(o["t"]).all())
        inl_p = inlier_mask(o["R"], o["t"], X, q, thr2)
        if fin and int(inl_p.sum()) >= cnt:
            polish = o["iters"]; R, t, inl, cnt = o["R"], o["t"], inl_p, int(inl_p.sum())
            after = float(np.sqrt(o["cost"] / m))
        else:
            polish = -1
    if side & 2:                                           # S is b's image 2: the solved pose inverted
        t = np.array([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)])
        R = R.T.copy()
    mask = np.zeros(mm, bool)
    mask[idx[inl]] = True
    res.update(n=n, R=R, t=t, mask=mask, counts=(n, cnt), info=(LINKPOSE_OK, it, r, polish), rms=(before, after))
    return res


def link_poses(run, x1, x2, focal, links, subsets, **kw):
    return [link_pose(run, x1, x2, focal, l, subsets, **kw) for l in links]


def reduction_margin(run, x1, x2, focal, links, subsets, **kw):
    """the model against itself with the polish sums in reversed order: (forward results, tied link indices, largest
    |rms_after| difference in pixels, largest angle between the two R in degrees, largest |t| difference, largest
    |rms_before| difference).  A link is tied when the two runs disagree on a decision or on an integer output."""
    fwd, ties, d_rms, d_R, d_t, d_rms0 = [], [], 0.0, 0.0, 0.0, 0.0
    for i, l in enumerate(links):
        f = link_pose(run, x1, x2, focal, l, subsets, **kw)
        r = link_pose(run, x1, x2, focal, l, subsets, order="reversed", **kw)
        fwd.append(f)
        if f["decisions"] != r["decisions"] or f["info"] != r["info"] or f["counts"] != r["counts"]:
            ties.append(i)
            continue
        if f["code"] != LINKPOSE_OK:
            continue
        d_rms = max(d_rms, abs(f["rms"][1] - r["rms"][1])); d_rms0 = max(d_rms0, abs(f["rms"][0] - r["rms"][0]))
        d_R = max(d_R, rot_angle_deg(f["R"], r["R"])); d_t = max(d_t, float(np.abs(f["t"] - r["t"]).max()))
    return fwd, ties, d_rms, d_R, d_t, d_rms0


# ---------------------------------------------------------------- physics bands
# Twice the largest deviation of the model on the CPU oracle's run of the PHYSICS stream over physics_pairs_and_links()
# (the SCALE_BAND precedent of scale_model.py; 256 samples, 1 px gate, min_shared 30, 10 polish iterations), as
# test_link_pose_cpu.py::test_physics_with_the_oracle prints and re-derives it.  rot err = the angle between the link
# pose's R and stream_poses' truth; deviation = | |t| - true baseline ratio |, in units of pair a's baseline (absolute, so
# that it also serves a pair whose true baseline is 0); the scale link's median of the same link stands beside it.
#   link (a, b, side)  n    inliers  rot err deg  |t|     truth   deviation  scale-link median
#   (0, 1, 1)          260  118      0.3879       1.0419  1.0000  0.0419     1.0894
#   (1, 2, 1)          241  108      0.1497       1.0199  1.0000  0.0199     1.0759
#   (2, 3, 1)          223  146      0.1095       0.9976  1.0000  0.0024     0.9867
#   (3, 4, 1)          221  74       0.0894       0.9987  1.0000  0.0013     1.0419
#   (0, 5, 0)          254  122      0.9585       1.6651  1.6922  0.0271     1.7875   <- largest rotation error
#   (1, 6, 0)          257  117      0.2797       1.9826  1.9297  0.0529     1.7177
#   (2, 7, 0)          223  129      0.0524       1.2220  1.2523  0.0303     1.2344
#   (3, 8, 0)          227  64       0.5098       2.0331  1.9514  0.0816     2.0152   <- largest deviation (polish rejected)
# Rotation-only bridge (test_rotation_only_bridge: S, A = frames 0, 1 of the stream, C = S turned by (3, -2, 1.5) degrees
# about its own centre; pairs (S, A), (S, C), link (0, 1, 0)):
#   five-point pose of (S, C): status OK, 500 matches, 458 RANSAC inliers -> 3 pose inliers, rotation error 0.0521 deg, a
#   unit t that means nothing;  link pose: n 256, inliers 167, rotation error 0.1119 deg, |t| 0.0306 (truth 0)
# The GPU tests use the same frames and the same bands.
LINK_POSE_ROT_BAND_DEG = 2 * 0.9585
LINK_POSE_SCALE_BAND = 2 * 0.0816
