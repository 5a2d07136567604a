"""Inputs shared by test_link_pose_cpu.py and test_gpu_link_pose.py: seeded exact triples for the minimal solver,
hand-built runs over three synthetic views (no images), the oracle run of the PHYSICS stream with its matched pixels, and
the rotation-only views."""
import numpy as np

from tests import link_pose_model as lp
from tests import scale_model as sc

NOISE_PX, OUTLIER_FRAC = 0.3, 0.25            # as homography_cases
GATE_PX, ITERS = 1.0, 256
COUNTS = (5, 6, 7, 64, 65, 256, 257, 500)

# ---- 1. the minimal solver on exact triples --------------------------------------------------------------------------
# triple_seeds(): the first 200 seeds s of default_rng(TRIPLE_BASE + s) whose quartic has no near-double root (every two
# of its four roots differ by more than 1e-3 of the larger: well_separated()).  TRIPLE_WORST is the model's largest
# deviation max(|R - R_true|, |t - t_true|) of the closest candidate over those seeds (they are seeds 0 .. 199: none of
# them is rejected), printed by test_link_pose_cpu.py::test_solver_on_exact_triples; the bound is ten times it (the margin
# is for root conditioning on another libm or compiler, not for the algorithm).
TRIPLE_BASE, TRIPLE_COUNT = 7_100_000, 200
TRIPLE_WORST = 6.14e-9
TRIPLE_BOUND = 10 * TRIPLE_WORST


def exact_triple(seed):
    """(P f64[3, 3], q f64[3, 2], R, t): three points in front of both cameras, a rotation of 1 .. 20 degrees, |t| = 0.5"""
    rng = np.random.default_rng(TRIPLE_BASE + int(seed))
    P = np.column_stack([rng.uniform(-3, 3, 3), rng.uniform(-2.2, 2.2, 3), rng.uniform(4, 14, 3)])
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    R = lp.rodrigues(np.radians(rng.uniform(1.0, 20.0)) * ax)
    t = rng.normal(size=3); t *= 0.5 / np.linalg.norm(t)
    Y = P @ R.T + t
    return P, Y[:, :2] / Y[:, 2:3], R, t


def well_separated(P, q, rel=1e-3):
    """no two roots of the triple's quartic closer than rel of the larger, in np.roots' view of the coefficients (a
    conjugate pair close to the real axis counts: it is the double root a perturbation makes real)"""
    c = lp.quartic([tuple(p) for p in P], [tuple(v) for v in q])["c"]
    r = np.roots(c[::-1])
    for i in range(len(r)):
        for k in range(i + 1, len(r)):
            if abs(r[i] - r[k]) <= rel * max(abs(r[i]), abs(r[k])):
                return False
    return True


def triple_seeds():
    out, s = [], 0
    while len(out) < TRIPLE_COUNT:
        P, q, _, _ = exact_triple(s)
        if well_separated(P, q):
            out.append(s)
        s += 1
    return out


# ---- 2. hand-built runs ---------------------------------------------------------------------------------------------------
BASE_A, BASE_C = 0.3, 0.45                    # baselines of pair a and of pair b in scene units: true |t| = 1.5


def _project(X, K, rng=None, noise=0.0):
    p = X[:, :2] / X[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    if noise:
        p = p + rng.normal(scale=noise, size=p.shape)
    return p.astype(np.float32)


def hand_run(n, side, K, seed=11, noise=NOISE_PX, outlier_frac=OUTLIER_FRAC, dup_a=0, dup_b=0, a_unusable=0, b_status=0):
    """Views S, A, C of n scene points; pair 0 = pair a (S, A in the order `side` bit 0 asks for), pair 1 = pair b (S, C per
    bit 1); link (0, 1, side).  Pair a carries exact triangulated points on its |t| = 1 scale and all masks set (but its
    last a_unusable matches, which are masked out and so leave the correspondence set); pair b carries f32 pixels with
    noise, a fraction of them gross outliers on C, and any status.  Keypoint indices and match orders are permutations.
    dup_a / dup_b: extra matches behind the real ones that repeat a key of S with a wrong point / observation and must
    lose to the lower index.  Returns (run, pts1, pts2 f32[2, mm, 2], truth (R, t) of pair b in its own convention on pair
    a's scale, n_expected, outlier flags by pair b's match index)."""
    rng = np.random.default_rng(seed * 1000 + n)
    K = np.asarray(K, np.float64)
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2.2, 2.2, n), rng.uniform(4, 14, n)])         # S's frame
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    Ra = lp.rodrigues(np.radians(3.0) * ax); ta = rng.normal(size=3); ta *= BASE_A / np.linalg.norm(ta)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    Rc = lp.rodrigues(np.radians(4.0) * ax); tc = rng.normal(size=3); tc *= BASE_C / np.linalg.norm(tc)
    XA = X @ Ra.T + ta; XC = X @ Rc.T + tc
    a2, b2 = bool(side & 1), bool(side & 2)
    mm = n + max(dup_a, dup_b)
    key = rng.permutation(4 * n)[:n].astype(np.int32)            # keypoint index of point k on S
    oth = rng.permutation(4 * n)[:n].astype(np.int32)            # ... on the pair's other frame
    q = np.full((2, mm), -1, np.int32); t = np.full((2, mm), -1, np.int32)
    rm = np.zeros((2, mm), bool); pm = np.zeros((2, mm), bool); pts = np.zeros((2, mm, 3))
    p1 = np.zeros((2, mm, 2), np.float32); p2 = np.zeros((2, mm, 2), np.float32)
    # pair a: match order = a permutation of the points
    oa = rng.permutation(n)
    ka, ko = key[oa], oth[oa]
    q[0, :n], t[0, :n] = (ko, ka) if a2 else (ka, ko)
    rm[0, :n] = pm[0, :n] = True
    if a_unusable:
        rm[0, n - a_unusable:n] = False
    pts[0, :n] = (XA if a2 else X)[oa] / BASE_A
    if a2:
        R0 = Ra.T; t0 = -(Ra.T @ ta) / BASE_A
    else:
        R0 = Ra; t0 = ta / BASE_A
    for d in range(dup_a):                                       # a usable duplicate of key ka[d] with a wrong point
        q[0, n + d], t[0, n + d] = (4 * n + d, ka[d]) if a2 else (ka[d], 4 * n + d)
        rm[0, n + d] = pm[0, n + d] = True
        pts[0, n + d] = pts[0, d] * 3.0
    # pair b
    ob = rng.permutation(n)
    kb, kc = key[ob], oth[ob]
    q[1, :n], t[1, :n] = (kc, kb) if b2 else (kb, kc)
    pS = _project(X[ob], K, rng, noise); pC = _project(XC[ob], K, rng, noise)
    out = np.zeros(mm, bool)
    bad = rng.choice(n, int(round(outlier_frac * n)), replace=False)
    out[bad] = True
    pC[bad] = rng.uniform([0, 0], [2 * K[0, 2], 2 * K[1, 2]], size=(len(bad), 2)).astype(np.float32)
    p1[1, :n], p2[1, :n] = (pC, pS) if b2 else (pS, pC)
    for d in range(dup_b):                                       # a duplicate of key kb[d] observed somewhere else
        q[1, n + d], t[1, n + d] = (4 * n + d, kb[d]) if b2 else (kb[d], 4 * n + d)
        wrong = np.array([5.0 + d, 7.0], np.float32)
        p1[1, n + d], p2[1, n + d] = (wrong, pS[d]) if b2 else (pS[d], wrong)
        out[n + d] = True
    status = np.array([0, b_status], np.int32)
    nm = np.array([n + dup_a, n + dup_b], np.int32)
    Rb = np.eye(3); tb = np.zeros(3)                            # pair b's own pose is never read
    run = sc.Run(q, t, rm, pm, pts, np.stack([R0, Rb]), np.stack([t0, tb]), status, nm)
    truth = (Rc.T, -(Rc.T @ tc) / BASE_A) if b2 else (Rc, tc / BASE_A)
    n_expected = n - a_unusable                                 # every point has a key of its own
    return run, p1, p2, truth, n_expected, out


# ---- 3. the PHYSICS stream under the oracle ------------------------------------------------------------------------------
class _KeepFeatures:
    """the oracle with its per-frame features kept, so that the matched pixels of scale_model.oracle_run's pairs can be
    rebuilt from its match indices"""

    def __init__(self, oracle):
        self._o, self.feats = oracle, []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def orb_detect_and_compute(self, frame, nfeatures):
        f = self._o.orb_detect_and_compute(frame, nfeatures)
        self.feats.append(f)
        return f


def oracle_run_with_points(oracle, frames, pairs, K, **kw):
    """(run, pts1, pts2 f32[P, mm, 2]) of scale_model.oracle_run over the pair list"""
    keep = _KeepFeatures(oracle)
    run = sc.oracle_run(keep, frames, pairs, K, **kw)
    P, mm = run.qidx.shape
    p1 = np.zeros((P, mm, 2), np.float32); p2 = np.zeros((P, mm, 2), np.float32)
    for p, (i, j) in enumerate(pairs):
        n = int(run.n_matches[p])
        k1, k2 = keep.feats[i][0], keep.feats[j][0]
        qi, ti = run.qidx[p, :n], run.tidx[p, :n]
        p1[p, :n] = np.stack([k1["x"][qi], k1["y"][qi]], 1); p2[p, :n] = np.stack([k2["x"][ti], k2["y"][ti]], 1)
    return run, p1, p2


def truth_link_poses(Rs, ts, pairs, links):
    """true pose of pair b of every link in its own convention on pair a's scale, from absolute poses X_i = Rs[i] X + ts[i]:
    (R [L, 3, 3], t [L, 3])"""
    c = -np.einsum("fji,fj->fi", Rs, ts)
    R, t = [], []
    for a, b, _ in links:
        i, j = pairs[b]
        Rr = Rs[j] @ Rs[i].T
        tr = ts[j] - Rr @ ts[i]
        ia, ja = pairs[a]
        R.append(Rr); t.append(tr / np.linalg.norm(c[ja] - c[ia]))
    return np.array(R), np.array(t)


# ---- 4. rotation-only bridge -----------------------------------------------------------------------------------------------
ROT_ONLY_ANGLES = (3.0, -2.0, 1.5)            # yaw, pitch, roll of C against S, degrees


def rotation_only_poses():
    """absolute poses of S, A, C: S and A are frames 0 and 1 of the PHYSICS stream (one step apart), C is S rotated about
    its own centre.  Pairs (S, A) = (0, 1) and (S, C) = (0, 2), linked at S: link (0, 1, side 0)."""
    from relative_pose_estimation_amd import synthetic
    P = sc.PHYSICS
    Rs, ts = synthetic.stream_poses(2, seed=P["seed"], max_angle_deg=P["max_angle_deg"], step=P["step"])
    Rr = synthetic._rot(*ROT_ONLY_ANGLES)
    return np.stack([Rs[0], Rs[1], Rr @ Rs[0]]), np.stack([ts[0], ts[1], Rr @ ts[0]])


_rot_frames = None


def rotation_only_frames():
    """(frames u8[3, 480, 640], K, Rs, ts), rendered once per process (read-only)"""
    global _rot_frames
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(640, 480)
    Rs, ts = rotation_only_poses()
    if _rot_frames is None:
        _rot_frames = synthetic.make_views(Rs, ts, K, seed=sc.PHYSICS["seed"])
        _rot_frames.setflags(write=False)
    return _rot_frames, K, Rs, ts
