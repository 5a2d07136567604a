"""Link bundles on the GPU (rpe_link_bundles / rpe_bundle_three_view, through the C-ABI): the gather, the compaction, the
Schur step and the Levenberg-Marquardt loop equal the float64 model (tests/link_bundle_model.py) fed with the GPU's own
fetched run -- every integer output and the view codes exactly, poses, points and rms within the model's own
reduction-order margin -- for the stage form at the lane-stride and wave-total edges, streams and pair lists, every
`side`, duplicate keys, the edges of min_shared, failed and skipped links, both state forms and the camera path; the
poses lie inside the bands fixed from the CPU model, the call is refused where it must be and changes nothing it reads."""
import numpy as np
import pytest

from tests import camera_model as cm
from tests import link_bundle_cases as bc
from tests import link_bundle_model as bm
from tests import link_pose_cases as lc
from tests import link_pose_model as lp
from tests import scale_model as sc
from tests import test_gpu_scale as tgs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


@pytest.fixture(scope="module")
def stage_problems():
    out = []
    for n in bc.STAGE_COUNTS:
        for n_c in (n, max(n // 2, 6), 6):
            out.append(bc.stage_problem(n, n_c))
    for spread in (0.15, 0.08):                                          # a cluster of a few points: the weakest conditioning
        for n, n_c in ((20, 6), (22, 9), (21, 13)):
            out.append(bc.stage_problem(n, n_c, spread=spread))
    out.append(bc.stage_problem(9, 5))                                   # five C observations: TOO_FEW
    return out


@pytest.fixture(scope="module")
def stage_models(stage_problems):
    """the model on the stage problems, forward and reversed, computed once"""
    return [bm.bundle(p) for p in stage_problems], [bm.bundle(p, order="reversed") for p in stage_problems]


@pytest.fixture(scope="module")
def margin(oracle, K_vga, stage_models):
    """ten times the largest forward / reversed difference of the model over the hand-built scenes -- the noisy hand runs
    (every count of link_bundle_cases.COUNTS, all four sides, fed with the link pose model's polished pose) and the
    stage problems (6 to 500 points, down to six observations on C, and clusters of about 20 points in one corner of the
    image, as the 64 strongest corners of a frame are: the weakest conditioning the tests below cover):
    (rms_after px, R degrees, t, point coordinate, rms_before px).  Recomputed here, never hard-coded."""
    fwd, rev = [], []
    for n in bc.COUNTS:
        for side in range(4):
            run, p1, p2 = bc.hand_run(n, side, K_vga)[:3]
            x1, x2, f = lp.observations(p1, p2, K_vga)
            pose = lp.link_pose(run, x1, x2, f, (0, 1, side), oracle.ransac_subsets, iters=lc.ITERS, threshold_px=lc.GATE_PX, min_shared=6)
            args = (run, x1, x2, f, (0, 1, side), pose["R"], pose["t"])
            fwd.append(bm.link_bundle(*args, threshold_px=lc.GATE_PX, min_shared=6))
            rev.append(bm.link_bundle(*args, threshold_px=lc.GATE_PX, min_shared=6, order="reversed"))
    ties, d = bm.reduction_margin(fwd, rev)
    ties2, d2 = bm.reduction_margin(*stage_models)
    print("forward / reversed: hand runs %s (ties %s), stage problems %s (ties %s)" % (d, ties, d2, ties2))
    d = np.maximum(d, d2)
    assert (d > 0).all() and (len(ties) + len(ties2)) * 16 <= len(fwd) + len(stage_models[0]), (d, ties, ties2)
    print("bundle margin (10 x forward / reversed): rms %.3e px, R %.3e deg, t %.3e, point %.3e, rms_before %.3e px" % tuple(10 * d))
    return 10 * d


def _inputs(e, P, K=None, cams=None):
    run = tgs._fetch_run(e, P)
    p1, p2 = e.fetch_matched_points(P)
    return (run,) + lp.observations(p1, p2, K, cams)


def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrs]


def _compare(got, l, f, r, margin, worst, run_form=True):
    """output l of a call against the forward model f (r: the reversed one); True when the link is tied"""
    Ra, ta, Rb, tb, pts, views, counts, info, rms = got
    if f["decisions"] != r["decisions"] or f["info"] != r["info"] or f["counts"] != r["counts"]:
        return True
    assert tuple(info[l]) == tuple(f["info"]), (l, info[l], f["info"])
    assert tuple(counts[l]) == tuple(f["counts"]), (l, counts[l], f["counts"])
    kR, kt, kS, ku, kp = ("R_a", "t_a", "R_b", "t_b", "points") if run_form else ("RA", "tA", "RC", "tC", "X")
    if run_form:
        assert np.array_equal(views[l], f["views"]), l
    if f["code"] in (bm.BUNDLE_PAIR_FAILED, bm.BUNDLE_TOO_FEW, bm.BUNDLE_SKIPPED):
        assert not any(a[l].any() for a in (Ra, ta, Rb, tb, pts, views, rms)), l
        return False
    n = len(f[kp])
    if f["code"] == bm.BUNDLE_REJECTED:                                  # the input state, bit for bit
        assert np.array_equal(Ra[l], f[kR]) and np.array_equal(ta[l], f[kt]) and np.array_equal(Rb[l], f[kS]) and np.array_equal(tb[l], f[ku])
        assert np.array_equal(pts[l, :n], f[kp]) and rms[l, 0] == rms[l, 1]
        assert abs(rms[l, 0] - f["rms"][0]) <= margin[4]
        return False
    d = (abs(rms[l, 1] - f["rms"][1]), max(lp.rot_angle_deg(Ra[l], f[kR]), lp.rot_angle_deg(Rb[l], f[kS])),
         max(np.abs(ta[l] - f[kt]).max(), np.abs(tb[l] - f[ku]).max()), np.abs(pts[l, :n] - f[kp]).max(), abs(rms[l, 0] - f["rms"][0]))
    worst[:] = np.maximum(worst, d)
    assert not pts[l, n:].any()
    assert rms[l, 1] <= rms[l, 0]
    return False


def _check(e, P, links, margin, K=None, cams=None, min_shared=8, threshold_px=None, poses=None):
    """rpe_link_bundles fed with rpe_link_poses' poses (both called BEFORE any structure fetch) == the model; returns
    (got, link poses, run)"""
    links = np.asarray(links, np.int32).reshape(-1, 3)
    a, b, s = links[:, 0], links[:, 1], links[:, 2]
    if poses is None:
        poses = e.link_poses(a, b, s, min_shared=min_shared)[:2]
    got = e.link_bundles(a, b, s, poses[0], poses[1], threshold_px=threshold_px, min_shared=min_shared)
    run, x1, x2, f = _inputs(e, P, K, cams)
    thr = e.cfg.ransac_threshold if threshold_px is None else threshold_px
    worst, ties = np.zeros(5), []
    for l, link in enumerate(links):
        kw = dict(threshold_px=thr, min_shared=min_shared)
        fw = bm.link_bundle(run, x1, x2, f, link, poses[0][l], poses[1][l], **kw)
        rv = bm.link_bundle(run, x1, x2, f, link, poses[0][l], poses[1][l], order="reversed", **kw)
        if _compare(got, l, fw, rv, margin, worst):
            ties.append(l)
    print("links %d ties %s codes %s counts %s: worst d_rms %.3e d_R %.3e d_t %.3e d_X %.3e d_rms0 %.3e" %
          (len(links), ties, got[7][:, 0].tolist(), got[6].tolist(), *worst))
    assert len(ties) * 4 <= len(links), ties
    assert (worst <= margin).all(), (worst, margin)
    return got, poses, run


# ------------------------------------------------------------------ 1. the stage form at exact counts
def test_stage_form_at_the_edges(capi, stage_problems, stage_models, margin):
    """6, 7, 255, 256, 257 and 500 points with has_c all set, half set and exactly 6 set, and the clustered problems, one call"""
    P = stage_problems
    e = capi.Engine(640, 480, max_batch=len(P), nfeatures=1000, max_matches=500)
    got = e.bundle_three_view([p["obs"][:, 0:2] for p in P], [p["obs"][:, 2:4] for p in P], [p["obs"][:, 4:6] for p in P],
                              [p["hc"] for p in P], [p["X0"] for p in P], [p["RA"] for p in P], [p["tA"] for p in P],
                              [p["RC"] for p in P], [p["tC"] for p in P], P[0]["fa"], P[0]["fc"])
    worst, ties = np.zeros(5), []
    for l, p in enumerate(P):
        fw, rv = stage_models[0][l], stage_models[1][l]
        if _compare(got, l, fw, rv, margin, worst, run_form=False):
            ties.append(l)
            continue
        want = np.zeros(500, np.uint8)
        if fw["code"] != bm.BUNDLE_TOO_FEW:
            want[:len(p["hc"])] = np.where(p["hc"], 3, 1)
        assert np.array_equal(got[5][l], want), l
    print("stage problems %d ties %s codes %s: worst d_rms %.3e d_R %.3e d_t %.3e d_X %.3e d_rms0 %.3e" % (len(P), ties, got[7][:, 0].tolist(), *worst))
    assert len(ties) * 4 <= len(P) and (worst <= margin).all(), (worst, margin)
    assert got[7][-1, 0] == bm.BUNDLE_TOO_FEW and tuple(got[6][-1]) == (9, 5)
    assert (got[7][:-1, 0] == bm.BUNDLE_OK).sum() >= len(P) - 3
    again = e.bundle_three_view([p["obs"][:, 0:2] for p in P], [p["obs"][:, 2:4] for p in P], [p["obs"][:, 4:6] for p in P],
                                [p["hc"] for p in P], [p["X0"] for p in P], [p["RA"] for p in P], [p["tA"] for p in P],
                                [p["RC"] for p in P], [p["tC"] for p in P], P[0]["fa"], P[0]["fc"])
    for x, y in zip(_bits(got), _bits(again)):
        assert np.array_equal(x, y)
    e.close()


# ------------------------------------------------------------------ 2. stream, physics
def test_stream_links_equal_model_and_physics(capi, physics, margin):
    """4 VGA frames of the PHYSICS stream, ORB-1000 / 500, the two consecutive links"""
    from relative_pose_estimation_amd import synthetic
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(frames[:4], K)
    assert not res[4].any()
    links = [(0, 1, 1), (1, 2, 1)]
    got, poses, _ = _check(e, 3, links, margin, K, min_shared=sc.PHYSICS_MIN_SHARED)
    Ra, ta, Rb, tb, pts, views, counts, info, rms = got
    assert (info[:, 0] == bm.BUNDLE_OK).all() and (counts[:, 1] >= sc.PHYSICS_MIN_SHARED).all()
    P = sc.PHYSICS
    Rs, ts = synthetic.stream_poses(P["n_frames"], seed=P["seed"], max_angle_deg=P["max_angle_deg"], step=P["step"])
    pairs = [(0, 1), (1, 2), (2, 3)]
    Rt, tt = lc.truth_link_poses(Rs, ts, pairs, links)
    for l, (a, b, _) in enumerate(links):
        Rta = Rs[pairs[a][1]] @ Rs[pairs[a][0]].T
        ra, rb, nt = lp.rot_angle_deg(Ra[l], Rta), lp.rot_angle_deg(Rb[l], Rt[l]), float(np.linalg.norm(tb[l]))
        print("stream link", links[l], "counts", counts[l].tolist(), "rot a %.4f (own %.4f) rot b %.4f (link pose %.4f) |t_b| %.4f (link pose %.4f) rms %s" %
              (ra, lp.rot_angle_deg(res[0][a], Rta), rb, lp.rot_angle_deg(poses[0][l], Rt[l]), nt, np.linalg.norm(poses[1][l]), rms[l].tolist()))
        assert abs(np.linalg.norm(ta[l]) - 1.0) <= 1e-12
        assert ra <= bm.BUNDLE_ROT_A_BAND_DEG and rb <= bm.BUNDLE_ROT_B_BAND_DEG and abs(nt - 1.0) <= bm.BUNDLE_SCALE_BAND   # constant step
    e.close()


# ------------------------------------------------------------------ 3. pair list, every side
def test_pair_list_links_all_sides(capi, physics, margin):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    s1, s2 = np.array(tgs.PAIRS, np.int32).T
    res = e.estimate_pairs(s1, s2, K)
    assert not res[4].any()
    assert sorted(set(l[2] for l in tgs.LIST_LINKS)) == [0, 1, 2, 3]
    got, _, _ = _check(e, 6, tgs.LIST_LINKS, margin, K)
    assert np.isin(got[7][:, 0], (bm.BUNDLE_OK, bm.BUNDLE_REJECTED)).all() and (got[7][:, 0] == bm.BUNDLE_OK).any()
    e.close()


# ------------------------------------------------------------------ 4. duplicate keys
def test_ratio_mode_duplicate_train_keypoints(capi, physics, margin):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=300, max_matches=200, match_mode=capi.MATCH_RATIO, match_ratio=0.9)
    e.frames_reserve(3)
    e.frames_put(frames[:3], [0, 1, 2])
    res = e.estimate_pairs([0, 2, 1], [1, 1, 2], K)
    assert not res[4].any()
    _, _, run = _check(e, 3, [(0, 1, 3), (1, 0, 3), (0, 2, 1), (2, 1, 1)], margin, K, min_shared=6)
    for p in (0, 1):
        n = int(run.n_matches[p])
        assert (np.unique(run.tidx[p, :n], return_counts=True)[1] > 1).any(), p
    e.close()


# ------------------------------------------------------------------ 5. edges and codes
def test_min_shared_sweep_with_few_matches(capi, physics, margin):
    """nfeatures = 64, max_matches = 32: min_shared swept across every n3 gives TOO_FEW on either side, never OK below 6"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=5, nfeatures=64, max_matches=32)
    e.estimate_stream(frames, K)
    links = [(i, i + 1, 1) for i in range(4)] + [(i + 1, i, 2) for i in range(4)]
    a, b, s = np.array(links, np.int32).T
    poses = e.link_poses(a, b, s, min_shared=1)[:2]
    got, _, _ = _check(e, 5, links, margin, K, min_shared=1, threshold_px=3.0, poses=poses)
    n3 = got[6][:, 1].copy()
    skipped = got[7][:, 0] == bm.BUNDLE_SKIPPED
    print("few matches: counts", got[6].tolist(), "codes", got[7][:, 0].tolist())
    seen = set()
    for ms in range(1, int(n3.max()) + 2):
        g, _, _ = _check(e, 5, links, margin, K, min_shared=ms, threshold_px=3.0, poses=poses)
        assert np.array_equal(g[6][:, 1], n3)
        assert ((g[7][:, 0] == bm.BUNDLE_TOO_FEW) == ((n3 < max(ms, 6)) & ~skipped)).all()
        seen |= set(g[7][:, 0].tolist())
    assert bm.BUNDLE_TOO_FEW in seen
    e.close()


def test_blank_frame_and_skipped_codes(capi, physics, margin):
    """a frame without keypoints: PAIR_FAILED as pair a, TOO_FEW as pair b (its match list is empty); the failed link poses
    are all zero and come back SKIPPED where pair a is fine"""
    frames, K = physics
    f = np.stack([frames[0], frames[1], frames[2], np.full((480, 640), 128, np.uint8), frames[4], frames[5], frames[4]])
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(f, K)
    assert res[4].tolist() == [0, 0, capi.PAIR_NO_DESCRIPTORS, capi.PAIR_NO_DESCRIPTORS, 0, 0]
    links = [(i, i + 1, 1) for i in range(5)] + [(2, 1, 2), (4, 3, 2)]
    got, poses, _ = _check(e, 6, links, margin, K)
    OK, FAILED, SKIP = bm.BUNDLE_OK, bm.BUNDLE_PAIR_FAILED, bm.BUNDLE_SKIPPED
    codes = got[7][:, 0].tolist()
    assert codes[1] == SKIP and codes[6] == SKIP and codes[2] == codes[3] == codes[5] == FAILED, codes   # link pose TOO_FEW: zero R0
    assert codes[0] in (OK, bm.BUNDLE_REJECTED) and codes[4] in (OK, bm.BUNDLE_REJECTED)
    assert got[6][1, 0] > 0 and got[6][1, 1] == 0 and not got[6][[2, 3, 5]].any()
    # the same links under a pose that is not zero: pair b has no matches, TOO_FEW with n3 = 0
    R0 = np.tile(np.eye(3), (7, 1, 1)); t0 = np.tile([0.0, 0.0, 1.0], (7, 1))
    g2, _, _ = _check(e, 6, links, margin, K, poses=(R0, t0))
    assert g2[7][[1, 6], 0].tolist() == [bm.BUNDLE_TOO_FEW] * 2 and not g2[6][[1, 6], 1].any() and (g2[6][[1, 6], 0] > 0).all()
    e.close()


def test_above_the_lds_cut(capi, physics, margin):
    """max_matches = 1500: the point state lives in device memory, walked in the same order"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=2, nfeatures=4000, max_matches=1500)
    res = e.estimate_stream(frames[:3], K)
    assert not res[4].any() and (res[3] > 1024).all(), res[3]
    got, _, _ = _check(e, 2, [(0, 1, 1), (1, 0, 2)], margin, K)
    assert np.isin(got[7][:, 0], (bm.BUNDLE_OK, bm.BUNDLE_REJECTED)).all() and (got[6][:, 1] > 100).all(), got[6]
    e.close()


def test_camera_pair_list_links(capi, physics, margin):
    frames, K = physics
    K2 = K.copy(); K2[0, 0] *= 1.01; K2[1, 1] *= 1.01
    dA, dB = [-0.02, 0.005, 0.0004, -0.0003], [0.015, -0.004, 0.0, 0.0002, 0.001]
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    e.frames_set_cameras([0, 1, 2, 3], [capi.Camera(K, dA), capi.Camera(K2, dB), capi.Camera(K, dA), capi.Camera(K2, dB)])
    res = e.estimate_pairs_cameras([0, 1, 2], [1, 2, 3])
    assert not res[4].any()
    slot = [cm.Cam(K, dA), cm.Cam(K2, dB), cm.Cam(K, dA), cm.Cam(K2, dB)]
    cams = [(slot[0], slot[1]), (slot[1], slot[2]), (slot[2], slot[3])]
    got, _, _ = _check(e, 3, [(0, 1, 1), (1, 2, 1), (2, 1, 2)], margin, cams=cams)
    assert np.isin(got[7][:, 0], (bm.BUNDLE_OK, bm.BUNDLE_REJECTED)).all(), got[7]
    e.close()


def test_rotation_only_bridge(capi, margin):
    """C = S turned about its own centre: the bundle keeps the rotation inside the band and |t_b| near 0"""
    frames, K, Rs, ts = lc.rotation_only_frames()
    e = capi.Engine(640, 480, max_batch=2, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(3)
    e.frames_put(frames, [0, 1, 2])
    res = e.estimate_pairs([0, 0], [1, 2], K)
    assert not res[4].any()
    got, poses, _ = _check(e, 2, [(0, 1, 0)], margin, K)
    Rt, _ = lc.truth_link_poses(Rs, ts, [(0, 1), (0, 2)], [(0, 1, 0)])
    rot = lp.rot_angle_deg(got[2][0], Rt[0]); nt = float(np.linalg.norm(got[3][0]))
    print("rotation-only: code %d counts %s rot err %.4f (link pose %.4f) |t_b| %.4f (link pose %.4f)" %
          (got[7][0, 0], got[6][0].tolist(), rot, lp.rot_angle_deg(poses[0][0], Rt[0]), nt, np.linalg.norm(poses[1][0])))
    assert got[7][0, 0] == bm.BUNDLE_OK and rot <= bm.BUNDLE_ROT_B_BAND_DEG and nt <= bm.BUNDLE_SCALE_BAND
    e.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    ok = ([0, 1], [1, 2], [1, 1])
    R0 = np.tile(np.eye(3), (2, 1, 1)); t0 = np.tile([0.0, 0.0, 1.0], (2, 1))

    def refused(match, a=ok[0], b=ok[1], s=ok[2], R=R0, t=t0, **kw):
        with pytest.raises(capi.RpeError, match=match):
            e.link_bundles(a, b, s, None if R is None else R[:max(len(a), 1)], None if t is None else t[:max(len(a), 1)], **kw)

    refused("rpe_link_bundles")                                           # before any run
    e.estimate_batch(frames[:2], frames[1:3], K)
    refused("share no frame", [0], [1], [1])                              # a 2-pair batch
    want = e.estimate_stream(frames[:4], K)
    R0, t0 = e.link_poses(*ok)[:2]
    good = e.link_bundles(*ok, R0, t0)
    refused("max_iters", max_iters=0)
    refused("max_iters", max_iters=101)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        refused("threshold_px", threshold_px=thr)
    bad = R0.copy(); bad[1, 2, 2] = np.nan
    refused("non-finite", R=bad)
    bad = t0.copy(); bad[0, 1] = np.inf
    refused("non-finite", t=bad)
    refused("R0 and t0", R=None)
    refused("R0 and t0", t=None)
    refused("R0 and t0", R=None, t=None)
    refused("two different pairs", [0, 1], [0, 2], [1, 1])
    refused("do not share", [0], [2], [1])
    refused("side must be", [0], [1], [4])
    refused("min_shared", min_shared=0)
    with pytest.raises(capi.RpeError, match="4\\*max_batch") as ei:
        e.link_bundles([0] * 13, [1] * 13, [1] * 13, np.tile(np.eye(3), (13, 1, 1)), np.zeros((13, 3)))
    assert "-3" in str(ei.value)                                           # RPE_ERR_CAPACITY
    again = e.link_bundles(*ok, R0, t0)                                    # the handle is still usable
    for x, y in zip(_bits(good), _bits(again)):
        assert np.array_equal(x, y)
    p1, p2 = e.fetch_matched_points(1)
    m = int(want[3][0])
    e.find_essential([p1[0, :m]], [p2[0, :m]], K)                          # a stage call
    refused("stage-API")
    e.estimate_stream(frames[:4], K)
    out = e.link_bundles([], [], [], np.zeros((0, 3, 3)), np.zeros((0, 3)))         # L = 0 is legal
    assert out[0].shape == (0, 3, 3) and out[6].shape == (0, 2)
    out = e.link_bundles([], [], [], None, None)
    assert out[4].shape == (0, sc.PHYSICS_MAX_MATCHES, 3)
    e.close()


# ------------------------------------------------------------------ 7. no side effects, determinism
def test_no_side_effects_and_determinism(capi, physics, stage_problems):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=5, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.estimate_stream(frames, K)
    links = ([0, 1, 2, 3, 1], [1, 2, 3, 4, 0], [1, 1, 1, 1, 2])

    def everything():
        return (_bits(e.fetch_results(5)) + _bits(e.fetch_structure(5)) + _bits(e.refine_poses(5)) + _bits(e.scale_links(*links)) +
                _bits(e.link_poses(*links)) + _bits(e.pair_homographies(5)))

    before = everything()
    R0, t0 = e.link_poses(*links)[:2]
    first = e.link_bundles(*links, R0, t0)
    assert (first[7][:, 0] == bm.BUNDLE_OK).any()
    p = stage_problems[4]                                                  # the stage form leaves the run alone too
    e.bundle_three_view([p["obs"][:, 0:2]], [p["obs"][:, 2:4]], [p["obs"][:, 4:6]], [p["hc"]], [p["X0"]], [p["RA"]], [p["tA"]],
                        [p["RC"]], [p["tC"]], p["fa"], p["fc"])
    for x, y in zip(before, everything()):
        assert np.array_equal(x, y)
    second = e.link_bundles(*links, R0, t0)
    for x, y in zip(_bits(first), _bits(second)):
        assert np.array_equal(x, y)
    fresh = capi.Engine(640, 480, max_batch=5, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    fresh.estimate_stream(frames, K)
    for x, y in zip(_bits(first), _bits(fresh.link_bundles(*links, R0, t0))):       # no structure fetch in front of it
        assert np.array_equal(x, y)
    e.close(); fresh.close()


# ------------------------------------------------------------------ 8. trajectory
def test_estimate_trajectory_bundle(capi, physics):
    from relative_pose_estimation_amd import PoseEstimator, geometry
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    reg = pe.estimate_trajectory(frames, register=True)
    d = pe.estimate_trajectory(frames, bundle=True)
    new = {'R_bundle', 't_bundle', 'bundle_code', 'bundle_counts', 'R_abs_ba', 'centers_ba'}
    assert set(d) == set(reg) | new
    for k in reg:
        assert np.array_equal(reg[k], d[k]), k
    i = np.arange(4)
    ba = pe.last_link_bundles(np.stack([i, i + 1, np.ones(4, int)], 1))
    for k, v in (('R_bundle', ba[2]), ('t_bundle', ba[3]), ('bundle_code', ba[7][:, 0]), ('bundle_counts', ba[6])):
        assert np.array_equal(d[k], v), k
    ok = ba[7][:, 0] == bm.BUNDLE_OK
    assert ok.any()
    Rb = np.where(ok[:, None, None], ba[2], d['R_link']); tb = np.where(ok[:, None], ba[3], d['t_link'])
    want = geometry.chain_trajectory(*geometry.registered_chain_inputs(d['R'], d['t'], d['status'], d['ratio_stats'][:, 1],
                                                                       d['link_code'], Rb, tb, d['link_pose_code']))
    assert np.array_equal(d['R_abs_ba'], want[0]) and np.array_equal(d['centers_ba'], want[2])
    pe.close()
