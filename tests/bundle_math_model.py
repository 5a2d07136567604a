"""The Python twin of relative_pose_estimation_amd/csrc/bundle_math.h: what the float64 models of pose refinement, link
poses, link bundles, track points and window bundles share -- the constants, the Levenberg-Marquardt acceptance rule, the
Cholesky solve, the damped inverse of a point block, the rotation update and the tangent basis -- stated once.  Plain
Python floats and numpy; it imports none of the models, they import it.  The scalar functions keep the library's operation
order (one rounding per operation); tests/test_bundle_math_cpu.py compares lm_loop, damped_inverse and solve with the
header's own statements run on the host, bit for bit."""
import math

import numpy as np

LAMBDA0, REL_TOL, STEP_TOL, SMALL_ANGLE = 1e-3, 1e-6, 1e-9, 1e-4      # the header's REFINE_* defines
DBL_MAX = float(np.finfo(np.float64).max)


# ---------------------------------------------------------------- sums and scalars
def _fsum(a, axis=0):
    return np.sum(a, axis=axis)


def _rsum(a, axis=0):
    """the same sum with the terms in reversed order (np.sum's pairwise tree then pairs different neighbours)"""
    return np.sum(np.flip(a, axis=axis), axis=axis)


def _lsum(a, axis=0):
    return np.sum(np.asarray(a, np.longdouble), axis=axis).astype(np.float64)


SUMS = {"forward": _fsum, "reversed": _rsum, "longdouble": _lsum}


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def finite(v):
    return abs(v) <= DBL_MAX


def fsqrt(v):
    """sqrt as C has it: NaN below zero, no exception"""
    return math.sqrt(v) if v >= 0.0 else math.nan


def fdiv(a, b):
    """a / b as C has it: infinities and NaN, no exception"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def step_norm(d):
    """lm_step_norm: d[0]^2 first, then ascending adds"""
    dn = d[0] * d[0]
    for k in range(1, len(d)):
        dn = dn + d[k] * d[k]
    return math.sqrt(dn)


# ---------------------------------------------------------------- the two solvers
def _elements(A, axes):
    """the entries of A over its last axes as nested lists: Python floats for one system, arrays over the leading axes for
    many -- the loops below are the same for both, and every entry keeps its own order of operations"""
    if A.ndim == axes:
        return A.tolist()
    if axes == 1:
        return [A[..., i] for i in range(A.shape[-1])]
    return [[A[..., i, j] for j in range(A.shape[-1])] for i in range(A.shape[-2])]


def cholesky(H):
    """bm_chol over systems of any leading shape, H (..., N, N) symmetric (its lower triangle is read): (L, ok) with
    H = L L', L (..., N, N) lower, and ok (...) False where a pivot is not > 0 or not finite (L is then not to be used).
    By columns; the pivot of column c is H(c, c) minus L(c, k)^2 for k = 0 .. c - 1, each subtracted serially in ascending
    k, then its square root; the entry (r, c) below it is H(r, c) minus L(r, k) L(c, k), subtracted the same way, divided
    by the pivot's root"""
    H = np.asarray(H, np.float64)
    N = H.shape[-1]
    a = _elements(H, 2)
    L = [[0.0] * N for _ in range(N)]
    ok = True
    with np.errstate(all="ignore"):
        for c in range(N):
            s = a[c][c]
            for k in range(c):
                s = s - L[c][k] * L[c][k]
            ok = ok & ((s > 0.0) & (abs(s) <= DBL_MAX))
            d = np.sqrt(s)
            L[c][c] = d
            for r in range(c + 1, N):
                v = a[r][c]
                for k in range(c):
                    v = v - L[r][k] * L[c][k]
                L[r][c] = v / d
    if H.ndim == 2:
        return np.array(L), ok
    out = np.zeros(H.shape)
    for r in range(N):
        for c in range(r + 1):
            out[..., r, c] = L[r][c]
    return out, ok


def cholesky_solve(L, r):
    """bm_chol_solve: z = (L L')^-1 r over any leading shape, L (..., N, N), r (..., N): forward, then back, each inner sum
    subtracted serially in ascending k"""
    L = np.asarray(L, np.float64); r = np.asarray(r, np.float64)
    N = L.shape[-1]
    a, b = _elements(L, 2), _elements(r, 1)
    y, z = [0.0] * N, [0.0] * N
    with np.errstate(all="ignore"):
        one = np.float64(1.0)                                   # divisions as C has them, also between two Python floats
        for i in range(N):
            v = b[i]
            for k in range(i):
                v = v - a[i][k] * y[k]
            y[i] = v * one / a[i][i]
        for i in range(N - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, N):
                v = v - a[k][i] * z[k]
            z[i] = v * one / a[i][i]
    return np.array(z) if r.ndim == 1 else np.stack(z, -1)


def solve(H, g, lam):
    """refine_solve: (H + lam diag H) d = -g by the library's Cholesky (rpe_refine_poses' solver for N parameters), or None
    when the matrix is not positive definite"""
    A = np.array(H, np.float64)
    i = np.arange(len(g))
    with np.errstate(all="ignore"):
        A[i, i] = A[i, i] + lam * A[i, i]
    L, ok = cholesky(A)
    if not ok:
        return None
    return cholesky_solve(L, -np.asarray(g, np.float64))


def damped_inverse(V, lam):
    """bm_damped_inverse over n point blocks V (n, 3, 3), symmetric: (Vi, ok) with Vi = (V + lam diag V)^-1 by the adjugate
    and ok (n,) False where V is singular (Vi is then not to be used).  V is damped in place"""
    with np.errstate(all="ignore"):
        for i in range(3):
            V[:, i, i] = V[:, i, i] + lam * V[:, i, i]
        v00, v01, v02, v11, v12, v22 = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
        c00 = v11 * v22 - v12 * v12; c01 = v02 * v12 - v01 * v22; c02 = v01 * v12 - v02 * v11
        c11 = v00 * v22 - v02 * v02; c12 = v01 * v02 - v00 * v12; c22 = v00 * v11 - v01 * v01
        det = (v00 * c00 + v01 * c01) + v02 * c02
        Vi = np.stack([np.stack([c00, c01, c02], 1), np.stack([c01, c11, c12], 1), np.stack([c02, c12, c22], 1)], 1) / det[:, None, None]
    return Vi, (det > 0.0) & (np.abs(det) <= DBL_MAX)


# ---------------------------------------------------------------- rotations and the tangent basis
def rodrigues(w):
    """exp([w]x) in numpy's matrix form: what the case modules build their scenes with"""
    w = np.asarray(w, np.float64).reshape(3)
    th2 = float(w @ w); th = np.sqrt(th2)
    if th < SMALL_ANGLE:
        A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0
    else:
        A = np.sin(th) / th; B = 2.0 * np.sin(0.5 * th) ** 2 / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + A * W + B * (np.outer(w, w) - th2 * np.eye(3))


def rotate(w, R):
    """exp([w]x) R as rpe_refine_poses forms it: I + A [w]x + B ([w][w]' - th2 I) entry by entry, then the row sums"""
    w = [float(v) for v in w]
    th2 = dot3(w, w); th = math.sqrt(th2)
    if th < SMALL_ANGLE:
        A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0
    else:
        sh = math.sin(0.5 * th); A = math.sin(th) / th; B = 2.0 * (sh * sh) / th2
    E = [[B * (w[i] * w[j]) + (1.0 - B * th2 if i == j else 0.0) for j in range(3)] for i in range(3)]
    E[0][1] -= A * w[2]; E[0][2] += A * w[1]
    E[1][0] += A * w[2]; E[1][2] -= A * w[0]
    E[2][0] -= A * w[1]; E[2][1] += A * w[0]
    R = np.asarray(R, np.float64)
    return np.array([[(E[i][0] * float(R[0, j]) + E[i][1] * float(R[1, j])) + E[i][2] * float(R[2, j]) for j in range(3)] for i in range(3)])


def rotate_np(w, R):
    """exp([w]x) R from numpy's matrix form and product.  It differs from rotate() in 92 % of random inputs, by 1.4e-15 at
    most; the refinement model keeps it, because under rotate() that model moves by more than its own reduction margin
    (profiles/README.md, round 24)"""
    return rodrigues(w) @ R


def tangent_basis(t):
    """refine_basis of rpe_refine_poses: b1 = normalise(t x e_k), k the axis of smallest |t_k| (lowest on ties), b2 = t x b1"""
    t = [float(v) for v in np.asarray(t).reshape(3)]
    k, m = 0, abs(t[0])
    if abs(t[1]) < m:
        k, m = 1, abs(t[1])
    if abs(t[2]) < m:
        k = 2
    e = [1.0 if i == k else 0.0 for i in range(3)]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    b1 = cross(t, e)
    n = math.sqrt(dot3(b1, b1))
    b1 = [v / n for v in b1]
    return np.array(b1), np.array(cross(t, b1))


def rot_angle_deg(Ra, Rb):
    """angle between two rotations, accurate for tiny angles (from the antisymmetric part, not from arccos of the trace)"""
    M = np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(np.sqrt(v @ v), 0.5 * (np.trace(M) - 1.0))))


def vec_angle_deg(a, b):
    a = np.asarray(a, np.float64).reshape(3); b = np.asarray(b, np.float64).reshape(3)
    c = np.cross(a, b)
    return float(np.degrees(np.arctan2(np.sqrt(c @ c), a @ b)))


# ---------------------------------------------------------------- the acceptance rule
def lm_loop(cost, max_iters, step, trial, step_norm, accept, rel_tol=REL_TOL, step_tol=STEP_TOL):
    """The header's lm_loop, the Levenberg-Marquardt acceptance rule and nothing else, over the same four hooks:
      step(lam)     forms the damped step at the caller's state (linearising it first where it has changed); None or False
                    when there is none
      trial(lam)    forms the trial state and returns its cost; non-finite vetoes the trial
      step_norm()   the length of the step; called for an accepted step only, before accept()
      accept()      the trial state becomes the state
    A missing step or a trial that does not strictly lower the cost multiplies lambda by 10; an accepted step divides it by
    10, moves the cost and stops the loop when it lowered the cost by no more than rel_tol of it or is no longer than
    step_tol.  Returns (cost, iterations begun, steps accepted, decisions: True = accepted, per iteration)."""
    lam, decisions = LAMBDA0, []
    for _ in range(max_iters):
        ok = bool(step(lam))
        if ok:
            c1 = trial(lam)
            ok = bool(finite(c1) and c1 < cost)
        decisions.append(ok)
        if not ok:
            lam = lam * 10.0
            continue
        dec, prev, dn = cost - c1, cost, step_norm()
        accept()
        cost = c1; lam = lam / 10.0
        if dec <= rel_tol * prev or dn <= step_tol:
            break
    return cost, len(decisions), sum(decisions), decisions
