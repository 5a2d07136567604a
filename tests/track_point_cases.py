"""Hand-built scenes for the track points (include/rpe_amd.h, "track points"): random scene points in front of F cameras
on a small random walk, projected through one K or a lens camera per frame, rounded to float32 pixels, with optional pixel
noise.  A case is a dict: 'name', 'tracks' (track_start, obs_frame, obs_xy as rpe_build_tracks writes them), 'R_abs',
'T_abs', 'cams' (one camera_model.Cam for all frames -- the K path -- or a list of one per frame), 'frame_group' (or
None), 'gates' (the call's threshold_px / min_views / max_cos / max_iters), 'truth' (the scene point of each track) and
'pixels' (the f64 pixels before rounding).  Every case keeps every used observation's final error outside 0.9 .. 1.1 x
threshold_px (test_track_points_cpu.py asserts it on the model), so no classification sits on the gate.  Used by
test_track_points_cpu.py and test_gpu_track_points.py."""
import numpy as np

from tests import camera_model as cm

K0 = np.array([[520.0, 0.0, 320.0], [0.0, 515.0, 240.0], [0.0, 0.0, 1.0]])
# a lens weak enough for the library's five fixed-point rounds to converge to the last bit (the noise-free recovery test)
WEAK = (-0.004, 0.001, 0.0001, -0.0001, 0.0)
DEFAULT_GATES = dict(threshold_px=2.0, min_views=2, max_cos=1.0, max_iters=10)
OUTLIER_PX = 20.0
# the gate of the displaced-observation case: a y displacement of 20 px leaves about 20 / n px on each of the other n - 1
# views and 20 (1 - 1 / n) on the displaced one: n = 2: 10 / 10, n = 3: 6.7 / 13.3, n = 8: 2.5 / 17.5 -- all outside
# 0.9 .. 1.1 x 8.2 = 7.38 .. 9.02
OUTLIER_GATE_PX = 8.2


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def walk(rng, F, step=0.25, max_angle_deg=1.5):
    """F world-to-camera poses: centres on a random walk mostly along x (so epipolar lines are near horizontal), small
    random rotations.  Returns (R_abs[F, 3, 3], T_abs[F, 3], centres[F, 3])"""
    c = np.zeros((F, 3)); R = np.zeros((F, 3, 3))
    for i in range(F):
        if i:
            c[i] = c[i - 1] + step * np.array([1.0, 0.0, 0.0]) + step * 0.2 * rng.standard_normal(3)
        R[i] = _rodrigues(np.deg2rad(max_angle_deg) * rng.uniform(-1, 1, 3))
    T = -np.einsum("fij,fj->fi", R, c)
    return R, T, c


def points_in_front(rng, n, centres, depth=(4.0, 8.0), spread=1.0):
    mid = centres.mean(0)
    return mid + np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.uniform(*depth, n)], 1)


def project(X, R, T, cam):
    """f64 pixel of scene point X in the view (R, T) through cam (its lens included)"""
    y = R @ X + T
    x, yy = y[0] / y[2], y[1] / y[2]
    if np.any(cam.dist != 0.0):
        x, yy = cm.distort(x, yy, cam.dist)
    return np.array([x * cam.fx + cam.cx, yy * cam.fy + cam.cy])


def build(name, R, T, cams, X, specs, rng=None, noise=0.0, frame_group=None, gates=None, offsets=None):
    """specs: one (point index, frames in ascending order) per track; offsets: {(track, position in the track): (dx, dy)}
    pixel displacements"""
    ts = [0]; of = []; px = []
    for t, (pi, frames) in enumerate(specs):
        for k, f in enumerate(frames):
            p = project(X[pi], R[f], T[f], cams if isinstance(cams, cm.Cam) else cams[f])
            if noise:
                p = p + noise * rng.standard_normal(2)
            if offsets and (t, k) in offsets:
                p = p + np.asarray(offsets[(t, k)], np.float64)
            of.append(f); px.append(p)
        ts.append(len(of))
    px = np.asarray(px, np.float64).reshape(-1, 2)
    tracks = {'track_start': np.asarray(ts, np.int32), 'obs_frame': np.asarray(of, np.int32), 'obs_xy': px.astype(np.float32)}
    return {'name': name, 'tracks': tracks, 'R_abs': R, 'T_abs': T, 'cams': cams, 'frame_group': frame_group,
            'gates': dict(DEFAULT_GATES, **(gates or {})), 'truth': np.asarray([X[pi] for pi, _ in specs]).reshape(-1, 3),
            'pixels': px}


def lens_cams(F):
    return [cm.Cam(K0 + np.diag([f % 3, -(f % 2), 0.0]), (cm.MILD, cm.RATIONAL, WEAK)[f % 3]) for f in range(F)]


def clean(lens, seed=3, F=8, n=6, weak=False):
    """noise-free tracks of 2, 3 and 8 views, n points each"""
    rng = np.random.default_rng(seed)
    R, T, c = walk(rng, F)
    X = points_in_front(rng, n, c)
    cams = ([cm.Cam(K0, WEAK)] * F if weak else lens_cams(F)) if lens else cm.Cam(K0)
    specs = [(i, [0, 1]) for i in range(n)] + [(i, [2, 4, 7]) for i in range(n)] + [(i, list(range(8))) for i in range(n)]
    return build(f"clean_{'lens' if lens else 'k'}{'_weak' if weak else ''}", R, T, cams, X, specs)


NOISY_FRAMES = {2: [0, 1], 3: [0, 1, 4], 5: [0, 1, 3, 5, 7], 8: list(range(8))}     # each starts with the two-view baseline (0, 1)


def noisy(n_views, seed=11, n=40, noise=0.3, gates=None, name=None):
    """n tracks of n_views views each under pixel noise"""
    rng = np.random.default_rng(seed)               # one scene for every view count
    R, T, c = walk(rng, 8)
    X = points_in_front(rng, n, c)
    frames = NOISY_FRAMES[n_views]
    return build(name or f"noisy_{n_views}", R, T, cm.Cam(K0), X, [(i, frames) for i in range(n)], rng, noise, gates=gates)


def outlier(seed=5):
    """tracks 0 .. 2: 3, 5 and 8 views, the second observation displaced by OUTLIER_PX across the epipolar lines; track 3:
    the point of track 0 as a two-view track with the same displaced observation"""
    rng = np.random.default_rng(seed)
    R, T, c = walk(rng, 8)
    X = points_in_front(rng, 3, c)
    specs = [(0, [0, 3, 6]), (1, [0, 2, 3, 5, 7]), (2, list(range(8))), (0, [0, 3])]
    off = {(t, 1): (0.0, OUTLIER_PX) for t in range(4)}
    return build("outlier", R, T, cm.Cam(K0), X, specs, offsets=off, gates=dict(threshold_px=OUTLIER_GATE_PX))


def _two_fixed(name, x0, x1):
    """two views with R = I at centres (0, 0, 0) and (1, 0, 0), observing the normalised points (x0, 0) and (x1, 0)"""
    R = np.stack([np.eye(3)] * 2); T = np.array([[0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    px = np.array([[K0[0, 0] * x0 + K0[0, 2], K0[1, 2]], [K0[0, 0] * x1 + K0[0, 2], K0[1, 2]]])
    tracks = {'track_start': np.array([0, 2], np.int32), 'obs_frame': np.array([0, 1], np.int32), 'obs_xy': px.astype(np.float32)}
    return {'name': name, 'tracks': tracks, 'R_abs': R, 'T_abs': T, 'cams': cm.Cam(K0), 'frame_group': None,
            'gates': dict(DEFAULT_GATES), 'truth': None, 'pixels': px}


def degenerate():
    """both pixels at the principal point: both bearings are (0, 0, 1) and the midpoint matrix is exactly diag(2, 2, 0)"""
    return _two_fixed("degenerate", 0.0, 0.0)


def behind():
    """the left camera looks left and the right camera looks right: the rays meet at z = -2.5"""
    return _two_fixed("behind", -0.2, 0.2)


def too_few_min_views():
    return dict(clean(False, seed=4, n=2), name="too_few_min_views", gates=dict(DEFAULT_GATES, min_views=3))


def groups(seed=9):
    """8 frames: 0 .. 3 in group 0, 4 without a pose (-1), 5 .. 7 in group 1, whose poses are on another scale (centres
    times 3) and so wrong for the scene.  Track 0 spans all frames (uses 0 .. 3); track 1 is (3, 4): one view, TOO_FEW;
    track 2 is (4, 5, 6): its used set is its last two observations, in group 1; track 3 is (4): no group at all"""
    rng = np.random.default_rng(seed)
    R, T, c = walk(rng, 8)
    X = points_in_front(rng, 2, c)
    case = build("groups", R, T, cm.Cam(K0), X, [(0, list(range(8))), (0, [3, 4]), (1, [4, 5, 6]), (1, [4])],
                 frame_group=np.array([0, 0, 0, 0, -1, 1, 1, 1], np.int32))
    # group 1's world is the scene scaled by 3: observations of track 2 are those of X[1] in the true poses, and the poses
    # handed to the call have three times the centres, so the point comes back as 3 X[1]
    T2 = T.copy()
    T2[4:] = 3 * T[4:]
    T2[4] = np.nan                    # a frame without a pose may hold anything
    case['T_abs'] = T2
    case['truth'] = np.vstack([X[0], X[0], 3 * X[1], X[1]])
    return case


def parallax(max_cos=0.9995):
    """a near point seen over the whole walk (wide angle: OK) and far points over two neighbouring frames (LOW_PARALLAX)"""
    rng = np.random.default_rng(21)
    R, T, c = walk(rng, 8)
    X = np.vstack([points_in_front(rng, 2, c, depth=(3.0, 4.0)), points_in_front(rng, 2, c, depth=(40.0, 50.0))])
    specs = [(0, [0, 7]), (1, [0, 3, 7]), (2, [3, 4]), (3, [2, 3, 4])]
    return build("parallax", R, T, cm.Cam(K0), X, specs, gates=dict(max_cos=max_cos))


def two_view_tracks(n, seed=31):
    """n two-view tracks: the workgroup-tail shapes"""
    rng = np.random.default_rng(seed + n)
    R, T, c = walk(rng, 4)
    X = points_in_front(rng, n, c)
    return build(f"two_view_{n}", R, T, cm.Cam(K0), X, [(i, [i % 3, 3]) for i in range(n)], rng, 0.2)


def mixed_lengths(seed=41):
    """one call with tracks of 2, 3, 64, 65 and 130 views (130 frames on a fine walk)"""
    rng = np.random.default_rng(seed)
    R, T, c = walk(rng, 130, step=0.03)
    X = points_in_front(rng, 5, c)
    specs = [(0, [0, 129]), (1, [5, 60, 120]), (2, list(range(3, 67))), (3, list(range(60, 125))), (4, list(range(130)))]
    return build("mixed_lengths", R, T, cm.Cam(K0), X, specs, rng, 0.2)


def cases():
    return [clean(False), clean(True), noisy(2), noisy(3), noisy(5), noisy(8), outlier(), degenerate(), behind(),
            too_few_min_views(), groups(), parallax(), noisy(5, name="midpoint", gates=dict(max_iters=0)), mixed_lengths()]
