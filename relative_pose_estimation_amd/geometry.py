"""Accuracy metrics of the reference's evaluator, restated for the benchmark harness.

rotation_error follows reference src/utils/geometry.py:128-149 (geodesic angle of
R_est @ R_gt.T, degrees); translation_direction_error follows :152-174;
default_camera_matrix follows src/core/camera_calibration.py:17-25,65-87.
"""
import numpy as np


def rotation_error(R_est, R_gt):
    R_diff = np.asarray(R_est) @ np.asarray(R_gt).T
    cos_angle = np.clip((np.trace(R_diff) - 1) / 2, -1.0, 1.0)
    return float(np.rad2deg(np.arccos(cos_angle)))


def translation_direction_error(t_est, t_gt):
    a = np.asarray(t_est, float).flatten(); b = np.asarray(t_gt, float).flatten()
    a = a / np.linalg.norm(a); b = b / np.linalg.norm(b)
    return float(np.rad2deg(np.arccos(np.clip(np.dot(a, b), -1.0, 1.0))))


def default_camera_matrix(width, height):
    """CameraCalibration().get_matrix(width, height): base intrinsics scaled to the image size."""
    sx, sy = width / 960, height / 720
    return np.array([[924.82939686 * sx, 0, 468.24930789 * sx],
                     [0, 920.4766382 * sy, 353.65863024 * sy],
                     [0, 0, 1]], dtype=np.float64)


# ---- Euler conventions of the reference's evaluator (harness only) -------------
# follows src/utils/geometry.py:48-125 ('yup': R = Ry(yaw) Rx(pitch) Rz(roll); NB the
# reference's yup pair is not self-inverse, use forward only) and :188-237 ('zyx').
def euler_to_rotation(yaw_deg, pitch_deg, roll_deg, convention="yup"):
    y, p, r = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg), np.deg2rad(roll_deg)
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    if convention == "zyx":
        return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                         [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                         [-sp, cp * sr, cp * cr]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def rotation_to_euler(R, convention="yup"):
    """(yaw, pitch, roll) in degrees."""
    R = np.asarray(R, float)
    if convention == "zyx":
        sy = np.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2)
        if sy >= 1e-6:
            roll = np.arctan2(R[2, 1], R[2, 2]); pitch = np.arctan2(-R[2, 0], sy); yaw = np.arctan2(R[1, 0], R[0, 0])
        else:
            roll = np.arctan2(-R[1, 2], R[1, 1]); pitch = np.arctan2(-R[2, 0], sy); yaw = 0.0
        return float(np.rad2deg(yaw)), float(np.rad2deg(pitch)), float(np.rad2deg(roll))
    pitch = np.arcsin(R[2, 1])
    if abs(R[2, 1]) > 0.9999:
        roll = np.arctan2(-R[1, 2], R[1, 1]); yaw = 0.0
    else:
        yaw = np.arctan2(-R[2, 0], R[0, 0]); roll = np.arctan2(R[1, 0], R[1, 1])
    return float(np.rad2deg(yaw)), float(np.rad2deg(pitch)), float(np.rad2deg(roll))


def bgr_to_gray(rgb):
    """cv2.cvtColor(BGR2GRAY) fixed-point formula applied to an RGB uint8 array
    (image_loader.py:23-28 path): (B*3735 + G*19235 + R*9798 + 16384) >> 15."""
    a = np.asarray(rgb).astype(np.int64)
    return ((a[..., 2] * 3735 + a[..., 1] * 19235 + a[..., 0] * 9798 + 16384) >> 15).astype(np.uint8)


# ---- trajectories from relative poses and scale links (not in the reference) -------------
def chain_trajectory(R_rel, t_rel, status, ratio, code):
    """Absolute poses of F = P + 1 frames from the P relative poses of consecutive pairs and the P - 1 scale links
    between them (PoseEstimator.estimate_trajectory; pure host code).  Convention X_{i+1} = R_rel[i] X_i + t_rel[i],
    |t_rel[i]| = 1; link i joins pair i and pair i + 1 and ratio[i] is its median (_capi.Engine.scale_links: baseline of
    pair i + 1 in units of the baseline of pair i), code[i] its LINK_* code; status[i] is the pair's PAIR_* code.

    baseline[0] = 1, baseline[i + 1] = baseline[i] * ratio[i]; R_{i+1} = R_rel[i] R_i and
    T_{i+1} = R_rel[i] T_i + baseline[i] t_rel[i], frame 0 at the origin.  Returns (R_abs[F, 3, 3], T_abs[F, 3],
    centers[F, 3] = -R^T T, baseline[P], segment[P]).

    ONLY INSIDE A SEGMENT DO DISTANCES SHARE A SCALE.  segment[i] numbers the runs of pairs whose links are all LINK_OK:
    a new segment starts at a failed pair (status != 0), at the pair after a failed pair, and at a pair whose link to its
    predecessor is not LINK_OK.  Across such a boundary the chain continues with ratio 1, so the arrays stay usable, but
    the baselines on the two sides are unrelated; a failed pair contributes the identity rotation and a zero step."""
    R_rel = np.asarray(R_rel, np.float64).reshape(-1, 3, 3)
    P = R_rel.shape[0]
    t_rel = np.asarray(t_rel, np.float64).reshape(P, 3)
    status = np.asarray(status).reshape(P)
    ratio = np.asarray(ratio, np.float64).reshape(-1)
    code = np.asarray(code).reshape(-1)
    if P < 1 or ratio.size != P - 1 or code.size != P - 1:
        raise ValueError(f"chain_trajectory: P >= 1 pairs need P - 1 links, got {P} pairs, {ratio.size} ratios, {code.size} codes")
    ok = status == 0
    baseline = np.ones(P)
    segment = np.zeros(P, np.int32)
    for i in range(1, P):
        joined = bool(ok[i] and ok[i - 1] and code[i - 1] == 0)          # 0 = LINK_OK
        baseline[i] = baseline[i - 1] * (ratio[i - 1] if joined else 1.0)
        segment[i] = segment[i - 1] + (0 if joined else 1)
    R_abs = np.zeros((P + 1, 3, 3)); T_abs = np.zeros((P + 1, 3))
    R_abs[0] = np.eye(3)
    for i in range(P):
        Ri, ti = (R_rel[i], t_rel[i]) if ok[i] else (np.eye(3), np.zeros(3))
        R_abs[i + 1] = Ri @ R_abs[i]
        T_abs[i + 1] = Ri @ T_abs[i] + baseline[i] * ti
    centers = -np.einsum("fji,fj->fi", R_abs, T_abs)
    return R_abs, T_abs, centers, baseline, segment


def frame_groups(status, segment):
    """The scale group of each of the F = P + 1 frames of a chain (frame_group of _capi.Engine.triangulate_tracks), from
    the status[P] the chain was built with and the segment[P] chain_trajectory returned; pure host code.
    g[0] = segment[0]; g[i + 1] = segment[i] where pair i is OK (status 0): the pair placed frame i + 1, on its own
    baseline.  Where pair i failed the chain only repeated frame i's pose, so frame i + 1 is related to nothing before
    it: it is the origin of the segment pair i + 1 starts, g[i + 1] = segment[i + 1], or -1 (no pose) when pair i is the
    last.

    A frame between two OK pairs whose link failed lies in two segments: it ends the earlier one and is the origin of the
    later one.  One integer cannot say both, and it goes with the EARLIER: there its position is a measured one (pair i's
    baseline, which is what a triangulation needs to be on the scale of the other frames), while as an origin it fixes
    nothing but the later segment's gauge.  A track's group is that of its first observation and observations are ordered
    by frame, so a track crossing the boundary keeps this frame's view with the earlier views.  The price: the later
    segment is seen from its second frame on, and a later segment of one pair has a single frame and gives no points."""
    status = np.asarray(status).reshape(-1)
    segment = np.asarray(segment, np.int32).reshape(-1)
    P = status.size
    if P < 1 or segment.size != P:
        raise ValueError(f"frame_groups: status and segment must have one entry per pair, got {P} and {segment.size}")
    g = np.empty(P + 1, np.int32)
    g[0] = segment[0]
    for i in range(P):
        g[i + 1] = segment[i] if status[i] == 0 else (segment[i + 1] if i + 1 < P else -1)
    return g


def windows_of_groups(frame_group, size=8, overlap=2):
    """Sliding windows of frames for _capi.Engine.bundle_windows: inside every run of consecutive frames that share one
    group >= 0 (frame_groups), windows of `size` frames (2 .. 8) that start every size - overlap frames; the last window of
    a run ends at the run's last frame and may be shorter, but never shorter than two frames nor contained in the window
    before it.  No window crosses a group boundary; a run of one frame gives none.  Returns a list of lists of frames."""
    g = np.asarray(frame_group).reshape(-1)
    if not (2 <= size <= 8) or not (0 <= overlap < size):
        raise ValueError(f"windows_of_groups: size must be 2 ... 8 and 0 <= overlap < size, got {size} and {overlap}")
    out = []
    a = 0
    while a < g.size:
        b = a + 1
        while b < g.size and g[b] == g[a]:
            b += 1
        if g[a] >= 0:
            s = a
            while b - s >= 2:
                e = min(s + size, b)
                out.append(list(range(s, e)))
                if e == b:
                    break
                s += size - overlap
        a = b
    return out


def chain_windows(windows, R_win, T_win, code, R_abs, T_abs):
    """Fuses the windows bundle_windows returned with code 0 (WINDOW_OK), in order, into one chain (pure host code).  Starts
    from copies of the input chain R_abs [F, 3, 3], T_abs [F, 3] with no frame placed.  An OK window w with frames
    f_0, f_1, .. and poses (R_win[w], T_win[w]) is aligned by a similarity onto the chain built so far: the chain's pose of
    f_0 fixes rotation and translation; the scale is the chain's centre distance f_0 -- f_1 over the window's, where an
    earlier window placed f_1 (and both distances are > 0), else 1.  The window then places its frames that no earlier
    window placed (f_0 too, at the pose it already has).  Frames of windows that are not OK, and frames in no window, keep
    the input chain's poses.  Returns (R [F, 3, 3], T [F, 3], centers [F, 3], placed bool[F])."""
    R = np.array(R_abs, np.float64).reshape(-1, 3, 3); T = np.array(T_abs, np.float64).reshape(-1, 3)
    placed = np.zeros(len(R), bool)
    for w, frames in enumerate(windows):
        if int(code[w]) != 0:
            continue
        Rw = np.asarray(R_win[w], np.float64).reshape(-1, 3, 3); Tw = np.asarray(T_win[w], np.float64).reshape(-1, 3)
        f0 = int(frames[0])
        # relative to the window's first frame: x_p = Q_p x_0 + s_p
        Q = [Rw[p] @ Rw[0].T for p in range(len(frames))]
        s = [Tw[p] - Q[p] @ Tw[0] for p in range(len(frames))]
        scale = 1.0
        f1 = int(frames[1])
        if placed[f1] and placed[f0]:
            have = float(np.linalg.norm(-R[f1].T @ T[f1] + R[f0].T @ T[f0])); own = float(np.linalg.norm(s[1]))
            if have > 0 and own > 0:
                scale = have / own
        for p, f in enumerate(frames):
            f = int(f)
            if placed[f]:
                continue
            if p:
                R[f] = Q[p] @ R[f0]
                T[f] = Q[p] @ T[f0] + scale * s[p]
            placed[f] = True
    centers = -np.einsum("fji,fj->fi", R, T)
    return R, T, centers, placed


def registered_chain_inputs(R_rel, t_rel, status, ratio, code, R_link, t_link, link_pose_code):
    """chain_trajectory's five inputs with pair i + 1 taken from link pose i (_capi.Engine.link_poses over the links
    (i, i + 1, 1)) where link_pose_code[i] is 0 (LINKPOSE_OK): R_link[i], t_link[i] / |t_link[i]| (zero when the link pose
    has no baseline), ratio |t_link[i]|, status 0, link code 0; the pair's own pose, status and scale link elsewhere.
    Returns copies (R_rel[P, 3, 3], t_rel[P, 3], status[P], ratio[P - 1], code[P - 1])."""
    R = np.array(R_rel, np.float64).reshape(-1, 3, 3)
    P = R.shape[0]
    t = np.array(t_rel, np.float64).reshape(P, 3)
    status = np.array(status).reshape(P)
    ratio = np.array(ratio, np.float64).reshape(-1)
    code = np.array(code).reshape(-1)
    R_link = np.asarray(R_link, np.float64).reshape(-1, 3, 3); t_link = np.asarray(t_link, np.float64).reshape(-1, 3)
    for i in np.flatnonzero(np.asarray(link_pose_code).reshape(-1) == 0):
        norm = float(np.sqrt(t_link[i] @ t_link[i]))
        R[i + 1] = R_link[i]
        t[i + 1] = t_link[i] / norm if norm > 0 else 0.0
        status[i + 1] = 0
        ratio[i] = norm
        code[i] = 0
    return R, t, status, ratio, code


# ---- pose graphs over a chain (not in the reference) -------------
EDGE_METRIC, EDGE_DIRECTION = 0, 1        # RPE_EDGE_*: the kinds of _capi.Engine.optimise_graphs' edges


def _edge_dict(i, j, R, t, w, kind):
    return {'i': np.asarray(i, np.int32).reshape(-1), 'j': np.asarray(j, np.int32).reshape(-1),
            'R': np.asarray(R, np.float64).reshape(-1, 3, 3), 't': np.asarray(t, np.float64).reshape(-1, 3),
            'w': np.asarray(w, np.float64).reshape(-1, 2), 'kind': np.asarray(kind, np.int32).reshape(-1)}


def chain_edges(R_abs, T_abs, frame_group, sigma_rot_deg=0.5, sigma_dir_deg=2.0):
    """The chain as edges of a pose graph (pure host code): one metric edge (f, f + 1) between consecutive frames that share
    one group >= 0 (frame_groups), carrying the chain's own relative pose M = R_(f+1) R_f', m = T_(f+1) - M T_f, so the
    chain has zero residual at the start and only the loop edges pull.  Weights: w_rot = 1 / rad(sigma_rot_deg), w_trans =
    1 / (rad(sigma_dir_deg) * max(|m|, the group's median |m|)): a direction error of sigma_dir on a step of the usual
    length, and never a larger weight on a step that happens to be short.  The sigmas are caller policy: 0.5 degrees is
    the median five-point rotation error this project measures; 2 degrees for the direction is NOT
    measured anywhere in the project.  Returns the dict of edges optimise_graphs takes ('i', 'j', 'R', 't', 'w', 'kind'),
    in ascending f."""
    R_abs = np.asarray(R_abs, np.float64).reshape(-1, 3, 3); T_abs = np.asarray(T_abs, np.float64).reshape(-1, 3)
    g = np.asarray(frame_group).reshape(-1)
    if not (g.size == R_abs.shape[0] == T_abs.shape[0]):
        raise ValueError("chain_edges: R_abs, T_abs and frame_group hold one entry per frame")
    if not (sigma_rot_deg > 0 and sigma_dir_deg > 0):
        raise ValueError("chain_edges: the sigmas must be > 0")
    f = np.flatnonzero((g[:-1] == g[1:]) & (g[:-1] >= 0)) if g.size > 1 else np.zeros(0, int)
    M = np.einsum("fab,fcb->fac", R_abs[f + 1], R_abs[f])
    m = T_abs[f + 1] - np.einsum("fab,fb->fa", M, T_abs[f])
    length = np.sqrt((m * m).sum(1))
    floor = np.zeros(len(f))
    for grp in np.unique(g[f]):
        sel = g[f] == grp
        floor[sel] = np.median(length[sel])
    w = np.zeros((len(f), 2))
    w[:, 0] = 1.0 / np.deg2rad(sigma_rot_deg)
    scale = np.deg2rad(sigma_dir_deg) * np.maximum(length, floor)
    w[:, 1] = np.divide(1.0, scale, out=np.zeros(len(f)), where=scale > 0)      # a group that never moves: rotation only
    return _edge_dict(f, f + 1, M, m, w, np.full(len(f), EDGE_METRIC))


def loop_edges(pairs, R, t, status, frame_group, min_inliers=0, inliers=None, sigma_rot_deg=0.5, sigma_dir_deg=2.0):
    """Loop closures as edges of a pose graph (pure host code): one direction edge per pair (i, j) of pairs[P, 2] whose pose
    X_j = R[p] X_i + t[p] is OK (status[p] == 0, a finite t that is not zero, inliers[p] >= min_inliers where inliers is
    given) and whose two frames share one group >= 0.  Pairs across groups are dropped: the scales of different groups are
    unrelated and the graph has no scale variable.  Weights: w_rot = 1 / rad(sigma_rot_deg), w_trans = 1 /
    rad(sigma_dir_deg) (the rows are a difference of unit vectors); the sigmas as in chain_edges -- the 2 degrees are not
    measured.  Returns (the dict of edges, in the order of the kept pairs; the indices of the pairs it dropped)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = pairs.shape[0]
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3)
    status = np.asarray(status).reshape(-1)
    g = np.asarray(frame_group).reshape(-1)
    if not (R.shape[0] == t.shape[0] == status.size == P) or (inliers is not None and np.asarray(inliers).size != P):
        raise ValueError("loop_edges: R, t, status (and inliers) hold one entry per pair")
    if P and (pairs.min() < 0 or pairs.max() >= g.size):
        raise ValueError("loop_edges: a pair names a frame outside frame_group")
    if not (sigma_rot_deg > 0 and sigma_dir_deg > 0):
        raise ValueError("loop_edges: the sigmas must be > 0")
    keep = (status == 0) & (pairs[:, 0] != pairs[:, 1]) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1) & ((t != 0).any(1))
    keep &= (g[pairs[:, 0]] == g[pairs[:, 1]]) & (g[pairs[:, 0]] >= 0)
    if inliers is not None:
        keep &= np.asarray(inliers).reshape(-1) >= min_inliers
    k = np.flatnonzero(keep)
    w = np.tile([1.0 / np.deg2rad(sigma_rot_deg), 1.0 / np.deg2rad(sigma_dir_deg)], (len(k), 1))
    return _edge_dict(pairs[k, 0], pairs[k, 1], R[k], t[k], w, np.full(len(k), EDGE_DIRECTION)), np.flatnonzero(~keep).astype(np.int32)


def graphs_of_groups(frame_group):
    """One graph per group >= 0 of two or more frames (frame_groups), in the order of the groups' first frames; a graph's
    frames ascend, so the group's first frame is at position 0, the one optimise_graphs keeps fixed.  A list of lists."""
    g = np.asarray(frame_group).reshape(-1)
    out, seen = [], set()
    for f in range(g.size):
        if g[f] >= 0 and int(g[f]) not in seen:
            seen.add(int(g[f]))
            frames = np.flatnonzero(g == g[f])
            if frames.size >= 2:
                out.append([int(x) for x in frames])
    return out


def edges_of_graphs(graphs, *edge_dicts):
    """The edges of chain_edges / loop_edges dealt to the graphs of graphs_of_groups: per graph one dict, holding the edges
    whose two frames are both in the graph, the first dict's before the second's.  Edges in no graph are left out."""
    out = []
    for frames in graphs:
        s = np.asarray(frames).reshape(-1)
        part = []
        for e in edge_dicts:
            k = np.flatnonzero(np.isin(e['i'], s) & np.isin(e['j'], s))
            part.append({key: e[key][k] for key in ('i', 'j', 'R', 't', 'w', 'kind')})
        out.append({key: np.concatenate([p[key] for p in part]) for key in ('i', 'j', 'R', 't', 'w', 'kind')} if part
                   else _edge_dict([], [], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 2)), []))
    return out


# ---- which model a pair obeys (not in the reference) -------------
def classify_pair(n_matches, n_E, n_H, n_rot, rotation_ratio=0.7, planar_ratio=0.8):
    """Names the geometric model a pair obeys from the inlier counts of PoseEstimator.last_homographies /
    _capi.Engine.pair_homographies: n_E of findEssentialMat, n_H of the homography, n_rot of the rotation fitted to the
    homography's inliers, out of n_matches matches.
      "rotation"  n_rot >= rotation_ratio * max(n_H, 1): a rotation alone explains what the homography explains -- no
                  usable baseline; the five-point (R, t) of such a pair is not to be trusted, R_rot is the rotation
      "planar"    otherwise, n_H >= planar_ratio * max(n_E, 1): one plane carries the matches
      "general"   otherwise
    THE RATIOS ARE CALLER POLICY, not properties of the library: the defaults separate the rendered pairs of
    DESIGN.md section 8 with a wide margin, and a scene, a matcher or a gate of your own may want others.  n_matches
    takes no part in the rule; it is an argument so that a caller's policy can use it."""
    if n_rot >= rotation_ratio * max(n_H, 1):
        return "rotation"
    if n_H >= planar_ratio * max(n_E, 1):
        return "planar"
    return "general"


def pixel_homography(H, K1, K2):
    """K2 H K1^-1: a homography of normalised coordinates (pair_homographies' H) as one of pixels, image 1 -> image 2"""
    return np.asarray(K2, np.float64) @ np.asarray(H, np.float64) @ np.linalg.inv(np.asarray(K1, np.float64))


def track_lengths(tracks):
    """Observations per track of a tracks dict (_capi.Engine.build_tracks / tracks_from_matches): i32[n_tracks]."""
    return np.diff(np.asarray(tracks['track_start'], np.int64)).astype(np.int32)


def tracks_of_frames(tracks, frames):
    """The tracks seen by ALL of the given frames: (track i32[n], obs i32[n, len(frames)]), one row per track (ascending
    track index) with the index into 'obs_frame' / 'obs_kp' / 'obs_xy' of its observation on frames[0], frames[1], ...
    The gather an N-view solver (or _capi.Engine.bundle_three_view) needs.  A track has at most one observation per
    frame, so the row is unique."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    if np.unique(frames).size != frames.size:
        raise ValueError("tracks_of_frames: the frames must be distinct")
    start = np.asarray(tracks['track_start'], np.int64)
    of = np.asarray(tracks['obs_frame'], np.int64)
    n_tracks = start.size - 1
    track_of_obs = np.repeat(np.arange(n_tracks), np.diff(start))
    obs = np.full((n_tracks, frames.size), -1, np.int64)
    for c, f in enumerate(frames):
        hit = np.nonzero(of == f)[0]
        obs[track_of_obs[hit], c] = hit
    keep = (obs >= 0).all(axis=1) if frames.size else np.zeros(n_tracks, bool)
    return np.nonzero(keep)[0].astype(np.int32), obs[keep].astype(np.int32)


def pairs_of_candidates(q_ids, t_ids, cand, cand_score):
    """The pair list of a candidate table (_capi.Engine.frames_similar / similarity_hamming with k > 0), a pure function:
    (pairs i32[P, 2], scores i32[P]).  q_ids[r] / t_ids[c] are the frames (store slots) of query row r and target column c;
    cand[r, m] is a column position or -1, cand_score[r, m] its score.  Every candidate (r, c) becomes the unordered pair
    (min, max) of its two frames; a pair proposed from both sides, or by repeated rows, appears once, with its largest
    score (the score is symmetric, so the sides agree).  Order: score descending, then the pair ascending."""
    q_ids = np.asarray(q_ids, np.int64).reshape(-1); t_ids = np.asarray(t_ids, np.int64).reshape(-1)
    cand = np.asarray(cand, np.int64); cand_score = np.asarray(cand_score, np.int64)
    if cand.ndim != 2 or cand.shape != cand_score.shape or cand.shape[0] != q_ids.size:
        raise ValueError(f"pairs_of_candidates: cand and cand_score must both be [len(q_ids), k], got {cand.shape}, {cand_score.shape}")
    if (cand >= t_ids.size).any():
        raise ValueError("pairs_of_candidates: a candidate is no position of t_ids")
    r, m = np.nonzero(cand >= 0)
    a, b = q_ids[r], t_ids[cand[r, m]]
    if (a == b).any():
        raise ValueError("pairs_of_candidates: a candidate pairs a frame with itself")
    lo, hi, sc = np.minimum(a, b), np.maximum(a, b), cand_score[r, m]
    o = np.lexsort((hi, lo, -sc))                      # score descending, then the pair: the first of equal pairs has its largest score
    lo, hi, sc = lo[o], hi[o], sc[o]
    _, first = np.unique(np.stack([lo, hi], 1), axis=0, return_index=True) if lo.size else (None, np.zeros(0, np.int64))
    first = np.sort(first)
    return np.stack([lo[first], hi[first]], 1).astype(np.int32).reshape(-1, 2), sc[first].astype(np.int32)
