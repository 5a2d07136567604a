"""float64 model of rpe_bundle_windows, written from the rule in include/rpe_amd.h ("window bundles"): the points of a
window from the tracks and the two masks, the gauge (everything relative to the window's first frame, the farthest centre
as the unit of scale), the rows of a view, the Schur elimination of the 3 x 3 point blocks into the reduced camera system
of 6 W - 7 parameters, the Levenberg-Marquardt loop of rpe_refine_poses and the maps back into the caller's frame.  NumPy
over the points, a Python loop over the positions of the window; every sum over points goes through one function (np.sum,
or np.sum of the flipped array with order="reversed"), so the model differs from the library by the order of its sums --
what reduction_margin() measures on the model itself.  Independent of the kernel's compaction, pair passes, LDS Cholesky
and state layout.  Used by test_window_bundle_cpu.py and test_gpu_window_bundle.py."""
import math

import numpy as np

from tests import bundle_math_model as mm
from tests import camera_model as cm

WINDOW_OK, WINDOW_NO_BASELINE, WINDOW_TOO_FEW, WINDOW_REJECTED = 0, 1, 2, 3
MAX_VIEWS = 8


# ---------------------------------------------------------------- the points of a window
def observations(tracks, cams):
    """per observation the normalised point (n_obs, 2) and the focal scale (n_obs,)"""
    of = np.asarray(tracks['obs_frame']).reshape(-1)
    xy32 = np.asarray(tracks['obs_xy'], np.float32).reshape(-1, 2)
    xy = np.zeros((len(of), 2)); f = np.zeros(len(of))
    for o, fr in enumerate(of):
        cam = cams if isinstance(cams, cm.Cam) else cams[fr]
        xy[o] = cm.normalise(xy32[o:o + 1], cam)[0]
        f[o] = cam.focal
    return xy, f


def window_points(tracks, frames, obs_use=None, point_use=None, max_points=4096):
    """(point_track (n,), pobs (n, W): the observation of each position or -1, dropped)"""
    ts = np.asarray(tracks['track_start']).reshape(-1); of = np.asarray(tracks['obs_frame']).reshape(-1)
    pos = {int(f): p for p, f in enumerate(frames)}
    ptrack, pobs, cand = [], [], 0
    for k in range(len(ts) - 1):
        if point_use is not None and not point_use[k]:
            continue
        row = [-1] * len(frames)
        for o in range(ts[k], ts[k + 1]):
            if obs_use is not None and obs_use[o] != 1:
                continue
            p = pos.get(int(of[o]))
            if p is not None and row[p] < 0:
                row[p] = o
        if sum(r >= 0 for r in row) >= 2:
            cand += 1
            if len(ptrack) < max_points:
                ptrack.append(k); pobs.append(row)
    W = len(frames)
    return np.array(ptrack, np.int64), np.array(pobs, np.int64).reshape(-1, W), cand - len(ptrack)


# ---------------------------------------------------------------- the rows of a view
def view_rows(p, Q, t, X, x, f, jac=True):
    """position p's view of every point: e (n, 2), y2 (n,), and with jac the rows by (w, d) J (n, 2, 6) and by the point JX
    (n, 2, 3).  Position 0 is the identity: y = X"""
    with np.errstate(all="ignore"):
        if p == 0:
            a = X.copy(); y = X
        else:
            a = np.stack([(Q[k, 0] * X[:, 0] + Q[k, 1] * X[:, 1]) + Q[k, 2] * X[:, 2] for k in range(3)], 1)
            y = a + t
        u = y[:, 0] / y[:, 2]; v = y[:, 1] / y[:, 2]
        e = np.stack([f * (u - x[:, 0]), f * (v - x[:, 1])], 1)
        if not jac:
            return e, y[:, 2]
        s = f / y[:, 2]
        z = np.zeros(len(X))
        J = np.zeros((len(X), 2, 6)); JX = np.zeros((len(X), 2, 3))
        J[:, 0] = np.stack([-s * (u * a[:, 1]), s * (a[:, 2] + u * a[:, 0]), -s * a[:, 1], s, z, -s * u], 1)
        J[:, 1] = np.stack([-s * (a[:, 2] + v * a[:, 1]), s * (v * a[:, 0]), s * a[:, 0], z, s, -s * v], 1)
        for r in range(2):
            for k in range(3):
                JX[:, r, k] = J[:, r, 3 + k] if p == 0 else (J[:, r, 3] * Q[0, k] + J[:, r, 4] * Q[1, k]) + J[:, r, 5] * Q[2, k]
    return e, y[:, 2], J, JX


def anchor_cols(J, b1, b2):
    """the anchor's block (w | tangent step): columns 3, 4 become Jt . b1, Jt . b2, column 5 is dropped (zero)"""
    c3 = (J[:, :, 3] * b1[0] + J[:, :, 4] * b1[1]) + J[:, :, 5] * b1[2]
    c4 = (J[:, :, 3] * b2[0] + J[:, :, 4] * b2[1]) + J[:, :, 5] * b2[2]
    J = J.copy()
    J[:, :, 3] = c3; J[:, :, 4] = c4; J[:, :, 5] = 0.0
    return J


class State:
    """the scaled problem: Q (W, 3, 3), t (W, 3), X (n, 3), with the fixed sets seen (n, W), x (n, W, 2), f (n, W), anchor A"""

    def __init__(self, Q, t, X, seen, x, f, A):
        self.Q, self.t, self.X, self.seen, self.x, self.f, self.A = Q, t, X, seen, x, f, A
        self.W = len(Q)
        self.off = [0] * self.W; self.np_ = [0] * self.W
        o = 0
        for p in range(1, self.W):
            self.off[p] = o; self.np_[p] = 5 if p == A else 6
            o += self.np_[p]
        self.N = o


def linearise(st):
    """per position: e (n, 2), Jc (n, 2, 6) (the anchor's in its own parameters), JX (n, 2, 3); rows of points that do not see
    the position are not to be used"""
    b1, b2 = mm.tangent_basis(st.t[st.A])
    rows = []
    for p in range(st.W):
        e, _, J, JX = view_rows(p, st.Q[p], st.t[p], st.X, st.x[:, p], st.f[:, p])
        if p == st.A:
            J = anchor_cols(J, b1, b2)
        rows.append((e, J, JX))
    return rows


def point_costs(st, Q=None, t=None, X=None):
    Q = st.Q if Q is None else Q; t = st.t if t is None else t; X = st.X if X is None else X
    pc = np.zeros(len(X))
    for p in range(st.W):
        e, _ = view_rows(p, Q[p], t[p], X, st.x[:, p], st.f[:, p], jac=False)
        m = st.seen[:, p]
        with np.errstate(all="ignore"):
            pc[m] = pc[m] + (e[m, 0] * e[m, 0] + e[m, 1] * e[m, 1])
    return pc


def point_blocks(st, rows, lam):
    """Vi (n, 3, 3), ok (n,), g_p (n, 3), W (list per position of (n, 6, 3))"""
    n = len(st.X)
    V = np.zeros((n, 3, 3)); gp = np.zeros((n, 3)); Wm = [None] * st.W
    with np.errstate(all="ignore"):
        for p in range(st.W):
            e, J, JX = rows[p]
            m = st.seen[:, p]
            for r in range(2):                                        # x row before y row
                V[m] += JX[m, r, :, None] * JX[m, r, None, :]
                gp[m] += JX[m, r, :] * e[m, r, None]
            if p:
                Wm[p] = J[:, 0, :, None] * JX[:, 0, None, :] + J[:, 1, :, None] * JX[:, 1, None, :]
    Vi, ok = mm.damped_inverse(V, lam)
    return Vi, ok, gp, Wm


def reduced_system(st, rows, Vi, gp, Wm, lam, S):
    """H (N, N) and g (N,) of the reduced camera system"""
    N = st.N
    H = np.zeros((N, N)); g = np.zeros(N)
    Y = [None] * st.W
    for p in range(1, st.W):
        W = Wm[p]
        Y[p] = (Vi[:, None, :, 0] * W[:, :, None, 0] + Vi[:, None, :, 1] * W[:, :, None, 1]) + Vi[:, None, :, 2] * W[:, :, None, 2]
    for p in range(1, st.W):
        e, J, _ = rows[p]
        m = st.seen[:, p]
        op, n_p = st.off[p], st.np_[p]
        U = S(J[m, 0, :, None] * J[m, 0, None, :] + J[m, 1, :, None] * J[m, 1, None, :])
        gc = S(J[m, 0, :] * e[m, 0, None] + J[m, 1, :] * e[m, 1, None])
        v = S((Y[p][m, :, 0] * gp[m, None, 0] + Y[p][m, :, 1] * gp[m, None, 1]) + Y[p][m, :, 2] * gp[m, None, 2])
        g[op:op + n_p] = (gc - v)[:n_p]
        for q in range(p, st.W):
            both = m & st.seen[:, q]
            oq, n_q = st.off[q], st.np_[q]
            Wq = Wm[q][both]; Yp = Y[p][both]
            Spq = S((Yp[:, :, None, 0] * Wq[:, None, :, 0] + Yp[:, :, None, 1] * Wq[:, None, :, 1]) + Yp[:, :, None, 2] * Wq[:, None, :, 2])
            Spq = np.asarray(Spq, np.float64).reshape(6, 6)
            for k in range(n_p):
                for l in range(k if p == q else 0, n_q):
                    u = U[k, l] if p == q else 0.0
                    if p == q and k == l:
                        u = u + lam * u
                    H[op + k, oq + l] = u - Spq[k, l]
    H = np.triu(H) + np.triu(H, 1).T
    return H, g


def schur_step(st, rows, lam, S):
    """(step_c (N,), dp (n, 3)) or None"""
    Vi, ok, gp, Wm = point_blocks(st, rows, lam)
    if not ok.all():
        return None
    H, g = reduced_system(st, rows, Vi, gp, Wm, lam, S)
    d = mm.solve(H, g, 0.0)
    if d is None:
        return None
    u = gp.copy()
    for p in range(1, st.W):
        m = st.seen[:, p]
        for k in range(st.np_[p]):                                    # ascending position, ascending parameter
            u[m] += Wm[p][m, k, :] * d[st.off[p] + k]
    dp = -((Vi[:, :, 0] * u[:, None, 0] + Vi[:, :, 1] * u[:, None, 1]) + Vi[:, :, 2] * u[:, None, 2])
    return d, dp


def dense_step(st, rows, lam):
    """the same step from the dense (N + 3 n)-parameter system with numpy.linalg.solve"""
    n, N = len(st.X), st.N
    Jr, r = [], []
    for j in range(n):
        for p in range(st.W):
            if not st.seen[j, p]:
                continue
            e, J, JX = rows[p]
            for k in range(2):
                row = np.zeros(N + 3 * n)
                if p:
                    row[st.off[p]:st.off[p] + st.np_[p]] = J[j, k, :st.np_[p]]
                row[N + 3 * j:N + 3 * j + 3] = JX[j, k]
                Jr.append(row); r.append(e[j, k])
    Jr = np.array(Jr); r = np.array(r)
    H = Jr.T @ Jr
    H[np.diag_indices_from(H)] *= 1.0 + lam
    d = np.linalg.solve(H, -(Jr.T @ r))
    return d[:N], d[N:].reshape(n, 3)


def apply_step(st, d, dp):
    Q = st.Q.copy(); t = st.t.copy()
    b1, b2 = mm.tangent_basis(st.t[st.A])
    for p in range(1, st.W):
        o = st.off[p]
        Q[p] = mm.rotate(d[o:o + 3], st.Q[p])
        if p == st.A:
            tn = (st.t[p] + d[o + 3] * b1) + d[o + 4] * b2
            t[p] = tn / math.sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2])
        else:
            t[p] = st.t[p] + d[o + 3:o + 6]
    return Q, t, st.X + dp


# ---------------------------------------------------------------- one window
def gauge(R, T):
    """(Q (W, 3, 3), s (W, 3), n2 (W,), anchor): every position relative to position 0, unscaled"""
    W = len(R)
    Q = np.zeros((W, 3, 3)); s = np.zeros((W, 3)); n2 = np.zeros(W)
    Q[0] = np.eye(3)
    with np.errstate(all="ignore"):
        for p in range(1, W):
            for r in range(3):
                for c in range(3):
                    Q[p, r, c] = (R[p, r, 0] * R[0, c, 0] + R[p, r, 1] * R[0, c, 1]) + R[p, r, 2] * R[0, c, 2]
            for r in range(3):
                s[p, r] = T[p, r] - ((Q[p, r, 0] * T[0, 0] + Q[p, r, 1] * T[0, 1]) + Q[p, r, 2] * T[0, 2])
            n2[p] = mm.dot3(s[p], s[p])
    A, best = 1, n2[1]
    for p in range(2, W):
        if n2[p] > best:
            A, best = p, n2[p]
    return Q, s, n2, A


def bundle_window(tracks, obs_xy_n, obs_f, points0, R_abs, T_abs, frames, obs_use=None, point_use=None, max_points=4096,
                  min_obs=8, max_iters=10, order="forward"):
    """one window as rpe_bundle_windows returns it: dict code, R (W, 3, 3), T (W, 3), points (n, 3), point_track, counts, info,
    rms, decisions"""
    S = mm.SUMS[order]
    frames = [int(f) for f in frames]
    W = len(frames)
    R = np.asarray(R_abs, np.float64).reshape(-1, 3, 3)[frames]; T = np.asarray(T_abs, np.float64).reshape(-1, 3)[frames]
    points0 = np.asarray(points0, np.float64).reshape(-1, 3)
    ptrack, pobs, dropped = window_points(tracks, frames, obs_use, point_use, max_points)
    n = len(ptrack)
    seen = pobs >= 0
    nobs = int(seen.sum())
    P0 = points0[ptrack] if n else np.zeros((0, 3))
    Q, s, n2, A = gauge(R, T)
    with np.errstate(all="ignore"):
        l = math.sqrt(n2[A]) if n2[A] >= 0 else float("nan")
    res = dict(code=WINDOW_OK, R=R.copy(), T=T.copy(), points=P0.copy(), point_track=ptrack, counts=(W, n, nobs, dropped),
               info=(0, 0, 0, A), rms=(0.0, 0.0), decisions=[])
    code = -1
    if not (l > 0.0) or not math.isfinite(l):
        code = WINDOW_NO_BASELINE
    elif any(int(seen[:, p].sum()) < max(min_obs, 6) for p in range(1, W)):
        code = WINDOW_TOO_FEW
    if code >= 0:
        res.update(code=code, info=(code, 0, 0, A))
        return res
    t = s / l
    X = np.stack([(((R[0, r, 0] * P0[:, 0] + R[0, r, 1] * P0[:, 1]) + R[0, r, 2] * P0[:, 2]) + T[0, r]) / l for r in range(3)], 1)
    x = np.zeros((n, W, 2)); f = np.ones((n, W))
    x[seen] = obs_xy_n[pobs[seen]]; f[seen] = obs_f[pobs[seen]]
    st = State(Q, t, X, seen, x, f, A)
    with np.errstate(all="ignore"):
        cost0 = float(S(point_costs(st)))
    cost, iters, acc, dec = cost0, 0, 0, []
    sol = new = None                                                  # the step (d_c, d_p) and the trial state (Q, t, X)

    def step(lam):                                                    # linearised in every iteration, moved or not
        nonlocal sol
        sol = schur_step(st, linearise(st), lam, S)
        return sol is not None

    def trial(lam):
        nonlocal new
        new = apply_step(st, *sol)
        with np.errstate(all="ignore"):
            return float(S(point_costs(st, *new)))

    def accept():
        st.Q, st.t, st.X = new

    if math.isfinite(cost0):
        cost, iters, acc, dec = mm.lm_loop(cost0, max_iters, step, trial, lambda: mm.step_norm(sol[0]), accept)
    take = acc > 0
    if take:
        fin = bool(np.isfinite(st.Q).all() and np.isfinite(st.t).all() and np.isfinite(st.X).all())
        front = True
        for p in range(W):
            z = ((st.Q[p, 2, 0] * st.X[:, 0] + st.Q[p, 2, 1] * st.X[:, 1]) + st.Q[p, 2, 2] * st.X[:, 2]) + st.t[p, 2]
            front = front and bool((z[seen[:, p]] > 0).all())
        take = fin and front
    with np.errstate(all="ignore"):
        before = float(np.sqrt(cost0 / nobs))
    res.update(code=WINDOW_OK if take else WINDOW_REJECTED, info=(WINDOW_OK if take else WINDOW_REJECTED, iters, acc, A),
               rms=(before, float(np.sqrt(cost / nobs)) if take else before), decisions=dec)
    if take:
        Ro = R.copy(); To = T.copy()
        for p in range(1, W):
            Qp = st.Q[p]
            for r in range(3):
                for c in range(3):
                    Ro[p, r, c] = (Qp[r, 0] * R[0, 0, c] + Qp[r, 1] * R[0, 1, c]) + Qp[r, 2] * R[0, 2, c]
                To[p, r] = l * st.t[p, r] + ((Qp[r, 0] * T[0, 0] + Qp[r, 1] * T[0, 1]) + Qp[r, 2] * T[0, 2])
        m = l * st.X - T[0]
        pts = np.stack([(R[0, 0, c] * m[:, 0] + R[0, 1, c] * m[:, 1]) + R[0, 2, c] * m[:, 2] for c in range(3)], 1)
        res.update(R=Ro, T=To, points=pts)
    return res


def bundle_windows(tracks, points0, R_abs, T_abs, windows, cams, obs_use=None, point_use=None, max_points=4096, min_obs=8,
                   max_iters=10, order="forward"):
    """the whole call: one bundle_window() result per window"""
    xy, f = observations(tracks, cams)
    return [bundle_window(tracks, xy, f, points0, R_abs, T_abs, w, obs_use, point_use, max_points, min_obs, max_iters, order)
            for w in windows]


def model_case(case, order="forward"):
    """the model's results of a case of tests/window_bundle_cases.py"""
    return bundle_windows(case['tracks'], case['points0'], case['R_abs'], case['T_abs'], case['windows'], case['cams'],
                          case['obs_use'], case['point_use'], case['max_points'], case['min_obs'], case['max_iters'], order)


def tied(f, r):
    return f["decisions"] != r["decisions"] or f["info"] != r["info"] or f["counts"] != r["counts"]


def differences(a, b):
    """[rms_after px, rotation degrees, translation, point coordinate, rms_before px] between two results of one window"""
    rot = max([mm.rot_angle_deg(x, y) for x, y in zip(a["R"], b["R"])])
    dp = np.abs(np.asarray(a["points"]) - np.asarray(b["points"])).max() if len(a["points"]) else 0.0
    return np.array([abs(a["rms"][1] - b["rms"][1]), rot, np.abs(np.asarray(a["T"]) - np.asarray(b["T"])).max(), dp,
                     abs(a["rms"][0] - b["rms"][0])])


def reduction_margin(results_fwd, results_rev):
    """the model against itself with the sums reversed: (tied indices, largest differences() over the OK windows)"""
    ties, d = [], np.zeros(5)
    for i, (f, r) in enumerate(zip(results_fwd, results_rev)):
        if tied(f, r):
            ties.append(i)
        elif f["code"] == WINDOW_OK:
            d = np.maximum(d, differences(f, r))
    return ties, d


# ---------------------------------------------------------------- accuracy
def pose_errors(R, T, R_true, T_true):
    """a window's poses against the truth, gauge and scale removed: per non-first position the rotation error of the relative
    rotation in degrees and the distance of the relative centre, both in units of the truth's largest centre distance l"""
    Q, s, n2, A = gauge(np.asarray(R), np.asarray(T)); Qt, st_, n2t, At = gauge(np.asarray(R_true), np.asarray(T_true))
    l, lt = math.sqrt(n2[At]), math.sqrt(n2t[At])
    rot, cen = [], []
    for p in range(1, len(Q)):
        rot.append(mm.rot_angle_deg(Q[p], Qt[p]))
        c = -Q[p].T @ s[p] / l; ct = -Qt[p].T @ st_[p] / lt
        cen.append(float(np.linalg.norm(c - ct)))
    return np.array(rot), np.array(cen)


# Twice the model's worst over the noisy cases of window_bundle_cases (NOISE_PX 0.3, POSE_NOISE_DEG / POSE_NOISE_CENTRE on the
# start poses), as test_window_bundle_cpu.py::test_accuracy_table prints them: the median over a window's non-first frames,
# the worst over the windows.  The measured values stand beside the constants, with the medians pooled over all 55
# non-first frames of those windows before and after the bundle.  The worst windows are the weakest: rotation a three-frame
# window (capped), centre a two-frame window (overlapping, frames 6 and 7).  See DESIGN section 8 for the whole table.
WINDOW_ROT_WORST_DEG = 0.6028        # measured 0.60276 (pooled median: input state 0.8972, bundled 0.2108)
WINDOW_CENTRE_WORST = 0.0875         # measured 0.08749 (pooled median: input state 0.0283, bundled 0.0072)
WINDOW_ROT_BAND_DEG = 2 * WINDOW_ROT_WORST_DEG
WINDOW_CENTRE_BAND = 2 * WINDOW_CENTRE_WORST
