"""Scalar float64 model of the track points (include/rpe_amd.h, "track points"), written from the header's rule: Python
floats, + - * / and math.sqrt only, every sum in ascending observation order.  No np.sum, no @, no np.linalg: those
reorder the arithmetic, and the library is compared with this file bit for bit (it has no reduction tree, calls no libm
function but sqrt and is built without contraction).  The normalisation is tests/camera_model.py's.  Used by
test_track_points_cpu.py and test_gpu_track_points.py."""
import math

import numpy as np

from tests import camera_model as cm
from tests.bundle_math_model import dot3, lm_loop, solve, step_norm

OK, TOO_FEW, DEGENERATE, BEHIND, OUTLIERS, LOW_PARALLAX = range(6)


def solve3(H, g, lam):
    """(H + lam diag H) d = -g, H the upper triangle (6 entries, row-major): the Cholesky of rpe_refine_poses (the shared
    scalar solve).  None when not positive definite"""
    d = solve([[H[0], H[1], H[2]], [H[1], H[3], H[4]], [H[2], H[4], H[5]]], g, lam)
    return None if d is None else d.tolist()


class View:
    """What the rule keeps of one observation: normalised point, world bearing, centre, focal scale, pose"""

    def __init__(self, xy, R, T, f):
        self.x, self.y = float(xy[0]), float(xy[1])
        self.R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
        self.T = [float(v) for v in np.asarray(T, np.float64).reshape(3)]
        self.f = float(f)
        R, T = self.R, self.T
        v = [(R[k] * self.x + R[3 + k] * self.y) + R[6 + k] for k in range(3)]
        n = math.sqrt(dot3(v, v))
        self.d = [v[k] / n for k in range(3)]
        self.c = [-((R[k] * T[0] + R[3 + k] * T[1]) + R[6 + k] * T[2]) for k in range(3)]

    def project(self, X):
        """(y2, u, w, e0, e1) at X, or None without positive depth"""
        R, T = self.R, self.T
        y0 = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + T[0]
        y1 = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + T[1]
        y2 = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + T[2]
        if not y2 > 0.0:
            return None
        u = y0 / y2; w = y1 / y2
        return y2, u, w, self.f * (u - self.x), self.f * (w - self.y)


def midpoint(views):
    A = [0.0] * 6; b = [0.0] * 3
    for v in views:
        n = 0
        for i in range(3):
            m = [(1.0 if i == k else 0.0) - v.d[i] * v.d[k] for k in range(3)]
            for k in range(i, 3):
                A[n] = A[n] + m[k]; n += 1
            b[i] = b[i] + ((m[0] * v.c[0] + m[1] * v.c[1]) + m[2] * v.c[2])
    return solve3(A, [-b[0], -b[1], -b[2]], 0.0)


def linearise(views, X):
    """(cost, H, g) of X over the views, or None when one of them has no positive depth"""
    cost = 0.0; H = [0.0] * 6; g = [0.0] * 3
    for v in views:
        p = v.project(X)
        if p is None:
            return None
        y2, u, w, e0, e1 = p
        cost = cost + (e0 * e0 + e1 * e1)
        q = v.f / y2; qa = q * u; qb = q * w
        J0 = [q * v.R[k] - qa * v.R[6 + k] for k in range(3)]
        J1 = [q * v.R[3 + k] - qb * v.R[6 + k] for k in range(3)]
        n = 0
        for i in range(3):
            for k in range(i, 3):
                H[n] = H[n] + (J0[i] * J0[k] + J1[i] * J1[k]); n += 1
            g[i] = g[i] + (J0[i] * e0 + J1[i] * e1)
    return cost, H, g


def solve_round(views, max_iters):
    """steps 2 and 3 over `views`: (code or None, X, iterations begun)"""
    X = midpoint(views)
    if X is None:
        return DEGENERATE, [0.0, 0.0, 0.0], 0
    lin = linearise(views, X)
    if lin is None:
        return BEHIND, X, 0
    cost, H, g = lin
    d = new = None                                          # the step and the trial (point, its linearisation)

    def step(lam):
        nonlocal d
        d = solve3(H, g, lam)
        return d is not None

    def trial(lam):                                         # linearised as it is costed: an accepted one needs no second pass
        nonlocal new
        Xn = [X[0] + d[0], X[1] + d[1], X[2] + d[2]]
        new = (Xn, linearise(views, Xn))
        return math.inf if new[1] is None else new[1][0]    # a view without positive depth vetoes the trial

    def accept():
        nonlocal X, H, g
        X, (_, H, g) = new

    iters = lm_loop(cost, max_iters, step, trial, lambda: step_norm(d), accept)[1]
    return None, X, iters


def track_point(views, groups, threshold_px=2.0, min_views=2, max_cos=1.0, max_iters=10):
    """One track: views[n] (View) and groups[n] (the group of each observation's frame) in observation order.  Returns
    (point[3], info[4], rms, min_cos, flag[n], err[n])"""
    n = len(views)
    zero = [0.0, 0.0, 0.0]
    G = next((g for g in groups if g >= 0), -1)
    used = [o for o in range(n) if G >= 0 and groups[o] == G]
    nU = len(used)
    flag = [0] * n; err = [0.0] * n
    if nU < min_views:
        return zero, [TOO_FEW, nU, 0, 0], 0.0, 0.0, flag, err
    sel = used
    iters = 0
    for rnd in range(2):
        code, X, it = solve_round([views[o] for o in sel], max_iters)
        iters += it
        if code == DEGENERATE:
            return zero, [code, nU, 0, iters], 0.0, 0.0, [0] * n, [0.0] * n
        if code == BEHIND:
            return X, [code, nU, 0, iters], 0.0, 0.0, [2 if o in used else 0 for o in range(n)], [0.0] * n
        ss = 0.0; inl = []
        for o in used:
            p = views[o].project(X)
            if p is None:
                flag[o] = 2; err[o] = -1.0
                continue
            e2 = p[3] * p[3] + p[4] * p[4]
            err[o] = math.sqrt(e2)
            if err[o] <= threshold_px:
                flag[o] = 1; ss = ss + e2; inl.append(o)
            else:
                flag[o] = 2
        rms = math.sqrt(ss / float(len(inl))) if inl else 0.0
        if len(inl) == nU or rnd == 1 or len(inl) < min_views:
            break
        sel = inl
    if len(inl) < min_views:
        return X, [OUTLIERS, nU, len(inl), iters], rms, 0.0, flag, err
    mc = 1.0
    r1 = [views[inl[0]].c[k] - X[k] for k in range(3)]
    n1 = math.sqrt(dot3(r1, r1))
    for o in inl[1:]:
        r = [views[o].c[k] - X[k] for k in range(3)]
        c = dot3(r1, r) / (n1 * math.sqrt(dot3(r, r)))
        if c < mc:
            mc = c
    return X, [LOW_PARALLAX if mc > max_cos else OK, nU, len(inl), iters], rms, mc, flag, err


def normalise_f64(p, cam):
    """camera_model.normalise without its rounding of the pixel to f32"""
    xd = (float(p[0]) - cam.cx) / cam.fx; yd = (float(p[1]) - cam.cy) / cam.fy
    if not np.any(cam.dist != 0.):
        return xd, yd
    x, y = cm.undistort(xd, yd, cam.dist)
    return float(x), float(y)


def make_views(obs_frame, obs_xy, R_abs, T_abs, cams, exact_pixels=None):
    """One View per observation.  cams: one cm.Cam for all frames, or one per frame.  exact_pixels: f64 pixels that take
    the place of the f32 obs_xy (the library has no such input: for what the rule itself recovers from exact data)"""
    obs_xy = np.asarray(obs_xy, np.float32).reshape(-1, 2)
    R_abs = np.asarray(R_abs, np.float64).reshape(-1, 3, 3); T_abs = np.asarray(T_abs, np.float64).reshape(-1, 3)
    views = []
    for o, fr in enumerate(np.asarray(obs_frame).reshape(-1)):
        cam = cams if isinstance(cams, cm.Cam) else cams[fr]
        xy = cm.normalise(obs_xy[o:o + 1], cam)[0] if exact_pixels is None else normalise_f64(exact_pixels[o], cam)
        views.append(View(xy, R_abs[fr], T_abs[fr], cam.focal))
    return views


def triangulate_tracks(tracks, R_abs, T_abs, cams, frame_group=None, exact_pixels=None, **gates):
    """The whole call: the dict of _capi.Engine.triangulate_tracks"""
    ts = np.asarray(tracks['track_start']).reshape(-1)
    of = np.asarray(tracks['obs_frame']).reshape(-1)
    views = make_views(of, tracks['obs_xy'], R_abs, T_abs, cams, exact_pixels)
    grp = [0] * len(of) if frame_group is None else [int(frame_group[f]) for f in of]
    n = len(ts) - 1
    out = {'points': np.zeros((n, 3)), 'code': np.zeros(n, np.int32), 'n_used': np.zeros(n, np.int32),
           'n_inliers': np.zeros(n, np.int32), 'iterations': np.zeros(n, np.int32), 'rms': np.zeros(n), 'min_cos': np.zeros(n),
           'obs_flag': np.zeros(len(of), np.uint8), 'obs_err': np.zeros(len(of))}
    for t in range(n):
        idx = list(range(ts[t], ts[t + 1]))
        X, info, rms, mc, flag, err = track_point([views[o] for o in idx], [grp[o] for o in idx], **gates)
        out['points'][t] = X
        out['code'][t], out['n_used'][t], out['n_inliers'][t], out['iterations'][t] = info
        out['rms'][t] = rms; out['min_cos'][t] = mc
        out['obs_flag'][idx] = flag; out['obs_err'][idx] = err
    return out


def model_case(case, **kw):
    """the model's dict of a case of tests/track_point_cases.py"""
    return triangulate_tracks(case['tracks'], case['R_abs'], case['T_abs'], case['cams'], case['frame_group'], **case['gates'], **kw)


FLOAT_KEYS = ('points', 'rms', 'min_cos', 'obs_err')
INT_KEYS = ('code', 'n_used', 'n_inliers', 'iterations', 'obs_flag')


def assert_equal(got, want, what=""):
    """integers equal, floats bit for bit (NaN never appears: a NaN would be a finding)"""
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8])
    for k in FLOAT_KEYS:
        g = np.ascontiguousarray(got[k], np.float64); w = np.ascontiguousarray(want[k], np.float64)
        assert g.shape == w.shape, (what, k)
        bad = np.flatnonzero(g.view(np.uint64).reshape(-1) != w.view(np.uint64).reshape(-1))
        assert bad.size == 0, (what, k, bad[:8], g.reshape(-1)[bad[:8]], w.reshape(-1)[bad[:8]])
