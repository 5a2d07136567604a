"""Hand-built scenes for the window bundles (include/rpe_amd.h, "window bundles"), from the parts of track_point_cases: scene
points in front of cameras on a small random walk, projected through one K or a lens camera per frame, rounded to float32
pixels.  A case is a dict: 'name', 'tracks', 'points0' (a start point per track), 'R_abs', 'T_abs' (the poses handed to the
call), 'cams' (one camera_model.Cam, or a list of one per frame), 'windows' (lists of frames), 'obs_use', 'point_use' (or
None), 'max_points', 'min_obs', 'max_iters', and the truth: 'R_true', 'T_true', 'X_true' (per track).  Noisy cases carry
NOISE_PX of pixel noise and start from poses perturbed by POSE_NOISE_DEG / POSE_NOISE_CENTRE and from the points
track_point_model triangulates under those poses, whose obs_flag and codes become the two masks.  Used by
test_window_bundle_cpu.py and test_gpu_window_bundle.py."""
import numpy as np

from tests import camera_model as cm
from tests import track_point_cases as tc
from tests import track_point_model as tpm

NOISE_PX = 0.3
POSE_NOISE_DEG = 0.57           # rotation of every start pose about a random axis: link_bundle_cases.POSE_NOISE_DEG
POSE_NOISE_CENTRE = 0.05        # displacement of every start centre (sigma per axis), in units of the walk's step (0.25)
START_GATE_PX = 12.0            # the triangulation gate of the start points: the perturbed poses alone cost several pixels


def _case(name, tracks, points0, R, T, cams, windows, truth, obs_use=None, point_use=None, max_points=4096, min_obs=6, max_iters=10):
    return dict(name=name, tracks=tracks, points0=np.asarray(points0, np.float64), R_abs=R, T_abs=T, cams=cams,
                windows=[list(w) for w in windows], obs_use=obs_use, point_use=point_use, max_points=max_points, min_obs=min_obs,
                max_iters=max_iters, R_true=truth[0], T_true=truth[1], X_true=truth[2])


def perturbed(rng, R, T, step=0.25):
    """every pose turned by POSE_NOISE_DEG about a random axis, every centre moved by POSE_NOISE_CENTRE steps"""
    Rn = R.copy(); Tn = T.copy()
    for i in range(len(R)):
        ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
        Rn[i] = tc._rodrigues(np.deg2rad(POSE_NOISE_DEG) * ax) @ R[i]
        c = -R[i].T @ T[i] + step * POSE_NOISE_CENTRE * rng.standard_normal(3)
        Tn[i] = -Rn[i] @ c
    return Rn, Tn


def scene(seed, F, n, specs=None, lens=False, noise=0.0, depth=(4.0, 8.0), step=0.25, spread=1.0):
    """(build() case, R, T, X, rng): n points, by default each seen by all F frames"""
    rng = np.random.default_rng(seed)
    R, T, c = tc.walk(rng, F, step=step)
    X = tc.points_in_front(rng, n, c, depth=depth, spread=spread)
    cams = tc.lens_cams(F) if lens else cm.Cam(tc.K0)
    specs = specs if specs is not None else [(i, list(range(F))) for i in range(n)]
    b = tc.build("scene", R, T, cams, X, specs, rng, noise)
    return b, R, T, X, rng


def exact(W, seed=100, n=40, lens=False, name=None):
    """exact data: true poses, true points, one window over frames 0 .. W-1"""
    b, R, T, X, _ = scene(seed + W, W, n, lens=lens)
    return _case(name or f"exact_w{W}", b['tracks'], b['truth'], R, T, b['cams'], [range(W)], (R, T, b['truth']))


def noisy(W, seed=200, n=60, windows=None, F=None, specs=None, lens=False, name=None, masks=True, geometry=None, **kw):
    """NOISE_PX on every pixel, perturbed start poses, start points and masks from the track-point model.  geometry: step,
    depth and spread of scene() where they are not the defaults"""
    F = F or W
    geometry = geometry or {}
    b, R, T, X, rng = scene(seed + W, F, n, specs=specs, lens=lens, noise=NOISE_PX, **geometry)
    Rn, Tn = perturbed(rng, R, T, geometry.get('step', 0.25))
    tp = tpm.triangulate_tracks(b['tracks'], Rn, Tn, b['cams'], threshold_px=START_GATE_PX, min_views=2, max_cos=1.0, max_iters=10)
    ok = (tp['code'] == tpm.OK).astype(np.uint8)
    assert ok.sum() * 10 >= len(ok) * 9, (name, W, tp['code'])
    return _case(name or f"noisy_w{W}", b['tracks'], tp['points'], Rn, Tn, b['cams'], windows or [range(W)], (R, T, b['truth']),
                 obs_use=tp['obs_flag'] if masks else None, point_use=ok if masks else None, **kw)


def counted(n, seed=300):
    """n points seen by the three frames of one window: the lane-stride and wave-total edges"""
    return noisy(3, seed=seed + n, n=n, name=f"count_{n}")


def mixed_views(seed=400):
    """8 frames; tracks over 2 (frames 0 and 7, 3 and 4), 3 and all 8 views in one window of 8"""
    n = 48
    specs = []
    for i in range(n):
        specs.append((i, [[0, 7], [3, 4], [1, 2, 6], list(range(8)), [0, 2, 4, 5, 7]][i % 5]))
    return noisy(8, seed=seed, n=n, specs=specs, name="mixed_views")


def outside(seed=500):
    """tracks over 8 frames, one window over frames 2, 3, 4: most observations lie outside the window"""
    return noisy(3, seed=seed, n=40, F=8, windows=[[2, 3, 4]], name="outside")


def anchor_first(seed=600):
    """window (2, 7, 3, 5): the farthest centre from frame 2 is frame 7, at position 1; the order is not ascending"""
    return noisy(4, seed=seed, n=50, F=8, windows=[[2, 7, 3, 5]], name="anchor_first")


def overlapping(seed=700):
    """two windows of 5 and 3 frames that share frames 3 and 4, and one of 2"""
    return noisy(5, seed=seed, n=50, F=8, windows=[[0, 1, 2, 3, 4], [3, 4, 5], [6, 7]], name="overlapping")


def lens(seed=800):
    return noisy(5, seed=seed, n=40, lens=True, name="lens")


def no_masks(seed=900):
    return noisy(4, seed=seed, n=30, masks=False, name="no_masks")


def masked(seed=1000):
    """every third track switched off, and the observation on frame 1 of every fourth track"""
    c = noisy(4, seed=seed, n=48, name="masked")
    pu = c['point_use'].copy(); pu[::3] = 0
    ou = c['obs_use'].copy()
    ts = c['tracks']['track_start']; of = c['tracks']['obs_frame']
    for k in range(0, 48, 4):
        for o in range(ts[k], ts[k + 1]):
            if of[o] == 1:
                ou[o] = 2
    c.update(point_use=pu, obs_use=ou)
    return c


def capped(seed=1100):
    """70 tracks under max_points = 64: the last six candidates are dropped"""
    return noisy(3, seed=seed, n=70, name="capped", max_points=64)


def stream_like(seed=1600):
    """the geometry of a chained stream, hand-built: the six true poses of the PHYSICS stream of scale_model
    (synthetic.stream_poses: a step of 0.3 in a RANDOM direction, the optical axis included, rotations up to 2 degrees) in
    the chain's unit of length, the baseline of one step, with 1100 points on the three planes of synthetic.DEPTHS (4, 7
    and 12, that is 13 .. 40 steps away), tracks of 2 .. 6 consecutive frames in the mix a run's tracks have (more than half
    of two frames), and the run form's two windows of four frames.  A point's depth is fixed by its parallax alone, so a
    rounding-level change of the sums moves it by about (depth / baseline)^2 roundings of its own size: 1600 for a two-frame
    track on the far plane against 4 .. 1000 in the other scenes, and without bound for a point near the epipole of a step
    along the optical axis, which the other scenes' sideways walk never has.  With coordinates five times larger and twelve
    times the points to sum over, this is the conditioning the margin of a run form has to be taken from"""
    from relative_pose_estimation_amd import synthetic
    from tests import scale_model as sc
    P = sc.PHYSICS
    step = P["step"]
    R, T = synthetic.stream_poses(P["n_frames"], seed=P["seed"], max_angle_deg=P["max_angle_deg"], step=step)
    T = np.asarray(T, np.float64).reshape(-1, 3) / step
    rng = np.random.default_rng(seed)
    n, F = 1100, P["n_frames"]
    depth = np.asarray(synthetic.DEPTHS)[rng.integers(0, 3, n)] / step
    X = np.stack([rng.uniform(-0.5, 0.5, n) * depth, rng.uniform(-0.4, 0.4, n) * depth, depth], 1)
    length = rng.choice([2, 3, 4, 5, 6], n, p=[0.57, 0.2, 0.1, 0.08, 0.05])
    specs = []
    for i in range(n):
        s0 = int(rng.integers(0, F - length[i] + 1))
        specs.append((i, list(range(s0, s0 + int(length[i])))))
    cams = cm.Cam(tc.K0)
    b = tc.build("scene", R, T, cams, X, specs, rng, NOISE_PX)
    Rn, Tn = perturbed(rng, R, T, 1.0)
    tp = tpm.triangulate_tracks(b['tracks'], Rn, Tn, cams, threshold_px=START_GATE_PX, min_views=2, max_cos=1.0, max_iters=10)
    ok = (tp['code'] == tpm.OK).astype(np.uint8)
    return _case("stream_like", b['tracks'], tp['points'], Rn, Tn, cams, [[0, 1, 2, 3], [2, 3, 4, 5]], (R, T, b['truth']),
                 obs_use=tp['obs_flag'], point_use=ok)


def behind_view(seed=1700):
    """noisy_w3's kind of scene with one more track whose pixels are those of a point BEHIND all three cameras, started at
    that point: its cost is lowest where it stands, the other points let steps be accepted, and the bundled state ends with
    a point behind the views that observe it: REJECTED after iterating"""
    n = 41
    rng = np.random.default_rng(seed)
    R, T, c = tc.walk(rng, 3)
    X = tc.points_in_front(rng, n, c)
    X[n - 1] = c.mean(0) + np.array([0.3, -0.2, -5.0])
    b = tc.build("scene", R, T, cm.Cam(tc.K0), X, [(i, [0, 1, 2]) for i in range(n)], rng, NOISE_PX)
    Rn, Tn = perturbed(rng, R, T)
    tp = tpm.triangulate_tracks(b['tracks'], Rn, Tn, b['cams'], threshold_px=START_GATE_PX, min_views=2, max_cos=1.0, max_iters=10)
    pu = (tp['code'] == tpm.OK).astype(np.uint8); ou = tp['obs_flag'].copy(); p0 = tp['points'].copy()
    pu[n - 1] = 1; ou[3 * (n - 1):] = 1; p0[n - 1] = X[n - 1]
    return _case("behind_view", b['tracks'], p0, Rn, Tn, b['cams'], [[0, 1, 2]], (R, T, b['truth']), obs_use=ou, point_use=pu)


def no_baseline():
    """both frames at one centre"""
    c = exact(2, seed=1200, name="no_baseline")
    R = c['R_abs'].copy(); T = c['T_abs'].copy()
    T[1] = -R[1] @ (-R[0].T @ T[0])
    c.update(R_abs=R, T_abs=T)
    return c


def too_few():
    """frame 2 sees five points only"""
    specs = [(i, [0, 1, 2] if i < 5 else [0, 1]) for i in range(20)]
    b, R, T, X, _ = scene(1300, 3, 20, specs=specs)
    return _case("too_few", b['tracks'], b['truth'], R, T, b['cams'], [[0, 1, 2]], (R, T, b['truth']))


def too_few_min_obs():
    """12 observations per frame under min_obs = 13"""
    c = exact(3, seed=1400, n=12, name="too_few_min_obs")
    c.update(min_obs=13)
    return c


def rejected():
    """the first camera is the identity and one start point lies in its plane z = 0, exactly: the start cost is not finite and
    no iteration runs"""
    c = exact(3, seed=1500, n=12, name="rejected")
    R = c['R_abs'].copy(); T = c['T_abs'].copy(); p = c['points0'].copy()
    R[0] = np.eye(3); T[0] = 0.0
    p[4] = (0.25, -0.125, 0.0)
    c.update(R_abs=R, T_abs=T, points0=p)
    return c


COUNTS = (6, 7, 255, 256, 257)
NOISY_W = (2, 3, 5, 8)


def noisy_cases():
    return [noisy(W) for W in NOISY_W]


def cases():
    return ([exact(W) for W in NOISY_W] + [exact(4, lens=True, name="exact_lens")] + noisy_cases() + [counted(n) for n in COUNTS] +
            [mixed_views(), outside(), anchor_first(), overlapping(), lens(), no_masks(), masked(), capped(), no_baseline(), too_few(),
             too_few_min_obs(), rejected(), behind_view(), stream_like()])
