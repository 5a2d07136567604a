"""float64 numpy model of rpe_refine_poses / rpe_refine_pose_points: Levenberg-Marquardt on the essential manifold over
a fixed set of matches, started from recoverPose's (R, t).  The same algorithm as the kernel (parameterisation,
tangent-basis rule, constants, accept / reject schedule, stop rules, fallback rule) with plain np.sum reductions and
np.linalg.solve; used by test_refine_cpu.py and test_gpu_refine.py.

  parameters   R <- exp([w]x) R (Rodrigues; series below SMALL_ANGLE), t <- normalise(t + a b1 + b b2) with (b1, b2) the
               tangent basis of the unit sphere at t: b1 = normalise(t x e_k), k the axis of smallest |t_k| (lowest
               index on ties), b2 = t x b1
  residual     signed Sampson distance of E = [t]x R on the K-normalised points, times (fx + fy) / 2 (pixels)
  step         (J'J + lambda diag(J'J)) d = -J'r; accepted only when the trial cost is strictly lower (lambda / 10),
               rejected otherwise (lambda * 10); a matrix that is not positive definite is a rejection
  stop         after max_iters iterations (accepted or rejected), or when an accepted step lowered the cost by no more
               than REL_TOL of it, or was no longer than STEP_TOL
  fallback     the refined pose is returned only if it is finite and keeps at least the input pose's cheirality inliers
               (tests/structure_model.triangulate over all matches)"""
import numpy as np

from tests import structure_model as sm
from tests.bundle_math_model import REL_TOL, STEP_TOL, SUMS, lm_loop, step_norm
from tests.bundle_math_model import rodrigues, rot_angle_deg, rotate_np, tangent_basis, vec_angle_deg

MIN_RESIDUALS = 6
REFINE_OK, REFINE_SKIPPED, REFINE_REJECTED = 0, 1, 2


def apply_step(R, t, d, basis=None):
    b1, b2 = basis if basis is not None else tangent_basis(t)
    Rn = rotate_np(d[:3], R)
    tn = t + d[3] * b1 + d[4] * b2
    return Rn, tn / np.sqrt(tn @ tn)


def residuals(R, t, x1, x2, scale, jac=False, basis=None):
    """r (n,) and, with jac, J (n, 5): columns w0 w1 w2 (left rotation increment), b1, b2 (tangent step of t)"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    n = len(x1)
    X1 = np.column_stack([x1, np.ones(n)]); X2 = np.column_stack([x2, np.ones(n)])
    a = X1 @ R.T                                     # R x1
    l = np.cross(t, a)                               # E x1
    c = np.cross(X2, t)
    m = c @ R                                        # E' x2 = R' (x2 x t)
    C = np.sum(X2 * l, 1)
    D = l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2
    inv = scale / np.sqrt(D)
    r = C * inv
    if not jac:
        return r
    b1, b2 = basis if basis is not None else tangent_basis(t)
    q = (C / D)[:, None]
    ta = a @ t
    dC = np.cross(a, c)                              # d C / d w
    dl0 = np.zeros((n, 3)); dl0[:, 0] = ta; dl0 -= a[:, 0:1] * t
    dl1 = np.zeros((n, 3)); dl1[:, 1] = ta; dl1 -= a[:, 1:2] * t
    dm0 = np.cross(R[:, 0], c); dm1 = np.cross(R[:, 1], c)
    g = l[:, 0:1] * dl0 + l[:, 1:2] * dl1 + m[:, 0:1] * dm0 + m[:, 1:2] * dm1
    J = np.zeros((n, 5))
    J[:, :3] = inv[:, None] * (dC - q * g)
    aX = np.cross(a, X2); r0X = np.cross(R[:, 0], X2); r1X = np.cross(R[:, 1], X2)
    for k, b in enumerate((b1, b2)):
        dCk = aX @ b
        dlk = np.cross(b, a)
        gk = l[:, 0] * dlk[:, 0] + l[:, 1] * dlk[:, 1] + m[:, 0] * (r0X @ b) + m[:, 1] * (r1X @ b)
        J[:, 3 + k] = inv * (dCk - q[:, 0] * gk)
    return r, J


def lm(R0, t0, x1, x2, scale, max_iters, order="forward", rel_tol=REL_TOL, step_tol=STEP_TOL):
    """the iteration on normalised points x1, x2 (n, 2), all of them residuals.  Returns a dict: R, t, cost0, cost,
    iters, accepted, history (cost after every iteration), decisions (True = accepted, per iteration)."""
    S = SUMS[order]
    R = np.asarray(R0, np.float64).reshape(3, 3).copy(); t = np.asarray(t0, np.float64).reshape(3).copy()
    iu = np.triu_indices(5)

    def linearise():
        basis = tangent_basis(t)
        return (basis,) + residuals(R, t, x1, x2, scale, True, basis)

    lin = linearise()                                  # (basis, r, J) of the state; None once the state has moved
    cost0 = float(S(lin[1] * lin[1]))
    out = dict(R=R, t=t, cost0=cost0, cost=cost0, iters=0, accepted=0, history=[cost0], decisions=[])
    if not np.isfinite(cost0):
        return out
    d = new = None
    taken = []                                         # the cost of every accepted trial

    def step(lam):
        nonlocal lin, d
        if lin is None:
            lin = linearise()
        _, r, J = lin
        H = np.zeros((5, 5))
        H[iu] = S(J[:, iu[0]] * J[:, iu[1]])
        H = np.triu(H) + np.triu(H, 1).T
        g = S(J * r[:, None])
        A = H + lam * np.diag(np.diag(H))
        try:
            np.linalg.cholesky(A)
            d = np.linalg.solve(A, -g)
            return bool(np.isfinite(d).all())
        except np.linalg.LinAlgError:
            return False

    def trial(lam):
        nonlocal new
        Rn, tn = apply_step(R, t, d, lin[0])
        rn = residuals(Rn, tn, x1, x2, scale)
        new = (Rn, tn, float(S(rn * rn)))
        return new[2]

    def accept():
        nonlocal R, t, lin
        R, t, lin = new[0], new[1], None
        taken.append(new[2])

    cost, iters, acc, dec = lm_loop(cost0, max_iters, step, trial, lambda: step_norm(d), accept, rel_tol, step_tol)
    for ok in dec:
        out["history"].append(taken.pop(0) if ok else out["history"][-1])
    out.update(R=R, t=t, cost=cost, iters=iters, accepted=acc, decisions=dec)
    return out


def refine(R0, t0, pts1, pts2, mask, K, max_iters=10, order="forward", status_ok=True):
    """one pair as the library returns it: dict R (3, 3), t (3,), inliers, info (code, iterations, residuals, accepted),
    rms (before, after), decisions.  pts in pixels (f32), mask selects the residuals."""
    K = np.asarray(K, np.float64)
    R0 = np.asarray(R0, np.float64).reshape(3, 3); t0 = np.asarray(t0, np.float64).reshape(3)
    mask = np.asarray(mask).astype(bool)
    n = int(mask.sum()) if status_ok else 0
    scale = (K[0, 0] + K[1, 1]) / 2
    x1 = sm.normalise(pts1, K)[mask[:len(pts1)]]; x2 = sm.normalise(pts2, K)[mask[:len(pts2)]]
    g_org = int(sm.triangulate(R0, t0, pts1, pts2, K)[0].sum()) if status_ok and len(pts1) else 0
    before = 0.0
    if n > 0:
        c0 = float(SUMS[order](residuals(R0, t0, x1, x2, scale) ** 2))
        before = float(np.sqrt(c0 / n))
    res = dict(R=R0, t=t0, inliers=g_org, info=(REFINE_SKIPPED, 0, n, 0), rms=(before, before), decisions=[])
    if not status_ok or n < MIN_RESIDUALS:
        return res
    o = lm(R0, t0, x1, x2, scale, max_iters, order)
    finite = bool(np.isfinite(o["cost0"]) and np.isfinite(o["R"]).all() and np.isfinite(o["t"]).all())
    g_ref = g_org
    if finite and o["accepted"] > 0:
        g_ref = int(sm.triangulate(o["R"], o["t"], pts1, pts2, K)[0].sum())
    res["decisions"] = o["decisions"]
    if not finite or g_ref < g_org:
        res["info"] = (REFINE_REJECTED, o["iters"], n, o["accepted"])
        return res
    res.update(R=o["R"], t=o["t"], inliers=g_ref, info=(REFINE_OK, o["iters"], n, o["accepted"]),
               rms=(before, float(np.sqrt(o["cost"] / n))))
    return res


def converge(R, t, x1, x2, scale=1.0):
    """the minimum the iteration is heading for: the same cost run for 200 iterations with the stop thresholds at
    machine precision"""
    return lm(R, t, x1, x2, scale, 200, rel_tol=np.finfo(np.float64).eps, step_tol=np.finfo(np.float64).eps)


# ---- scenes and the reduction-order margin shared by test_refine_cpu.py and test_gpu_refine.py
ACCURACY_PAIRS, ACCURACY_CFG = 48, 8         # synthetic.make_batch(ACCURACY_PAIRS, K_vga, cfg=ACCURACY_CFG)
NOISY_SEED = 2024


def noisy_scenes(K, B=16, n=300, sigma=0.5, outlier_frac=0.2, seed=NOISY_SEED):
    """B pairs of exact geometry with pixel noise: n matches of random points under a random pose, Gaussian noise of
    sigma pixels on both images, stored as f32; outlier_frac of the matches replaced by gross outliers (uniform over the
    image) and masked out; the start is the true pose turned by 0.5 ... 2 degrees about a random axis with t tilted by
    as much.  Returns a list of dicts R_true, t_true, R0, t0, pts1, pts2, mask."""
    rng = np.random.default_rng(seed)
    K = np.asarray(K, np.float64)
    f = np.array([K[0, 0], K[1, 1]]); c = np.array([K[0, 2], K[1, 2]])
    out = []
    for _ in range(B):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        R = rodrigues(np.radians(rng.uniform(1.0, 5.0)) * ax)
        t = rng.normal(size=3); t /= np.linalg.norm(t)
        X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2.2, 2.2, n), rng.uniform(4, 14, n)])
        Xc = X @ R.T + 0.4 * t
        p1 = X[:, :2] / X[:, 2:3] * f + c + rng.normal(scale=sigma, size=(n, 2))
        p2 = Xc[:, :2] / Xc[:, 2:3] * f + c + rng.normal(scale=sigma, size=(n, 2))
        mask = np.ones(n, bool)
        bad = rng.choice(n, int(round(outlier_frac * n)), replace=False)
        mask[bad] = False
        p2[bad] = rng.uniform([0, 0], [2 * c[0], 2 * c[1]], size=(len(bad), 2))
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = np.radians(rng.uniform(0.5, 2.0))
        R0 = rodrigues(ang * ax) @ R
        e = np.zeros(3); e[np.argmin(np.abs(t))] = 1.0                  # a tangent pair at t, in the numpy form the scenes
        b1 = np.cross(t, e); b1 = b1 / np.sqrt(b1 @ b1); b2 = np.cross(t, b1)   # were drawn with: they stay what they were
        ph = rng.uniform(0, 2 * np.pi)
        t0 = np.cos(ang) * t + np.sin(ang) * (np.cos(ph) * b1 + np.sin(ph) * b2)
        out.append(dict(R_true=R, t_true=t, R0=R0, t0=t0 / np.linalg.norm(t0), pts1=p1.astype(np.float32),
                        pts2=p2.astype(np.float32), mask=mask))
    return out


def reduction_margin(scenes, K, max_iters=10):
    """the model against itself with the residual sums taken in reversed order: (forward results, tied pair indices,
    largest |rms_after| difference in pixels, largest angle between the two R in degrees, between the two t, largest
    |rms_before| difference in pixels).  A pair is tied when the two runs disagree on an accept / reject decision."""
    fwd, ties, d_rms, d_R, d_t, d_rms0 = [], [], 0.0, 0.0, 0.0, 0.0
    for i, s in enumerate(scenes):
        a = refine(s["R0"], s["t0"], s["pts1"], s["pts2"], s["mask"], K, max_iters)
        b = refine(s["R0"], s["t0"], s["pts1"], s["pts2"], s["mask"], K, max_iters, order="reversed")
        fwd.append(a)
        if a["decisions"] != b["decisions"] or a["info"] != b["info"]:
            ties.append(i)
            continue
        d_rms = max(d_rms, abs(a["rms"][1] - b["rms"][1]))
        d_R = max(d_R, rot_angle_deg(a["R"], b["R"]))
        d_t = max(d_t, vec_angle_deg(a["t"], b["t"]))
        d_rms0 = max(d_rms0, abs(a["rms"][0] - b["rms"][0]))
    return fwd, ties, d_rms, d_R, d_t, d_rms0
