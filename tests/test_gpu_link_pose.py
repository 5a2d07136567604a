"""Link poses on the GPU (rpe_link_poses, through the C-ABI): the kernel's join, ordered list, P3P rounds, election and
polish equal the float64 model (tests/link_pose_model.py) fed with the GPU's own fetched run -- every integer output and
the mask exactly, R and t bit for bit without the polish and within the model's own reduction-order margin with it -- for
streams and pair lists, every `side`, duplicate keys, the edges of min_shared and of the round, failed pairs, both list
forms, the largest table and the camera path; the poses lie inside the bands fixed from the CPU oracle, the call is
refused where it must be and changes nothing it reads."""
import numpy as np
import pytest

from tests import camera_model as cm
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
def subsets(oracle):
    cache = {}

    def get(n, iters):
        if n not in cache or len(cache[n]) < iters:
            cache[n] = oracle.ransac_subsets(n, max(iters, 257))
        return cache[n]
    return get


@pytest.fixture(scope="module")
def margin(oracle, K_vga):
    """the polish margin, as test_gpu_refine takes its own from fixed scenes: the hand-built runs of the CPU tests (every
    count of link_pose_cases.COUNTS from 6 up, all four sides: 6 to 500 correspondences, the conditioning the tests below
    cover), the model against itself with the sums reversed, ten times the largest difference: (rms_after px, R degrees,
    t, rms_before px).  Recomputed here, never hard-coded."""
    d = np.zeros(4)
    ties = scenes = 0
    for n in lc.COUNTS[1:]:
        for side in range(4):
            run, p1, p2 = lc.hand_run(n, side, K_vga)[:3]
            x1, x2, f = lp.observations(p1, p2, K_vga)
            _, t, d_rms, d_R, d_t, d_rms0 = lp.reduction_margin(run, x1, x2, f, [(0, 1, side)], oracle.ransac_subsets, iters=lc.ITERS,
                                                               threshold_px=lc.GATE_PX, min_shared=6, refine_iters=10)
            ties += len(t); scenes += 1
            d = np.maximum(d, [d_rms, d_R, d_t, d_rms0])
    assert (d > 0).all() and ties * 16 <= scenes, (d, ties)
    print("polish margin (10 x forward / reversed): rms %.3e px, R %.3e deg, t %.3e, rms_before %.3e px" % tuple(10 * d))
    return 10 * d


def _inputs(e, P, K=None, cams=None):
    """the last run as the model takes it: the fetched run and the normalised matched points"""
    run = tgs._fetch_run(e, P)
    p1, p2 = e.fetch_matched_points(P)
    return (run,) + lp.observations(p1, p2, K, cams)


def _same_integers(got, models, what=""):
    R, t, mask, counts, info, rms = got
    for l, m in enumerate(models):
        assert tuple(info[l]) == tuple(m["info"]), (what, l, info[l], m["info"])
        assert tuple(counts[l]) == tuple(m["counts"]), (what, l, counts[l], m["counts"])
        assert np.array_equal(mask[l], m["mask"]), (what, l)
        if m["code"] != lp.LINKPOSE_OK:
            assert not R[l].any() and not t[l].any() and not rms[l].any() and not mask[l].any() and counts[l, 1] == 0 and not info[l, 1:].any()


def _check(e, P, links, subsets, K=None, cams=None, iters=lc.ITERS, min_shared=8, threshold_px=None, polish=None):
    """rpe_link_poses (called BEFORE any structure fetch: it launches the structure kernels itself) == the model: without
    the polish bit for bit, with it (polish = the margin fixture) within the margin; a link on which the model's forward
    and reversed runs disagree on a decision is tied and skipped.  Returns (minimal, polished, run)."""
    links = np.asarray(links, np.int32).reshape(-1, 3)
    kw = dict(iters=iters, min_shared=min_shared, threshold_px=threshold_px)
    got0 = e.link_poses(links[:, 0], links[:, 1], links[:, 2], refine_iters=0, **kw)
    run, x1, x2, f = _inputs(e, P, K, cams)
    mkw = dict(iters=iters, min_shared=min_shared, threshold_px=e.cfg.ransac_threshold if threshold_px is None else threshold_px)
    m0 = lp.link_poses(run, x1, x2, f, links, subsets, refine_iters=0, **mkw)
    _same_integers(got0, m0, "minimal")
    for l, m in enumerate(m0):
        assert np.array_equal(got0[0][l], m["R"]) and np.array_equal(got0[1][l], m["t"]), (l, got0[0][l] - m["R"], got0[1][l] - m["t"])
        assert got0[5][l, 0] == got0[5][l, 1]
    if polish is None:
        return got0, None, run
    got = e.link_poses(links[:, 0], links[:, 1], links[:, 2], refine_iters=10, **kw)
    fwd, ties = lp.reduction_margin(run, x1, x2, f, links, subsets, refine_iters=10, **mkw)[:2]
    worst = [0.0, 0.0, 0.0, 0.0]
    for l, m in enumerate(fwd):
        if l in ties:
            continue
        _same_integers(tuple(g[l:l + 1] for g in got), [m], "polished")
        if m["code"] != lp.LINKPOSE_OK:
            continue
        d = (abs(got[5][l, 1] - m["rms"][1]), lp.rot_angle_deg(got[0][l], m["R"]), float(np.abs(got[1][l] - m["t"]).max()),
             abs(got[5][l, 0] - m["rms"][0]))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print("links %d ties %s: worst d_rms %.3e d_R %.3e d_t %.3e d_rms0 %.3e, margin %.3e %.3e %.3e %.3e" % (len(links), ties, *worst, *polish))
    assert len(ties) * 4 <= len(links), ties
    assert (np.array(worst) <= polish).all(), (worst, polish)
    assert (got[5][:, 1] <= got[5][:, 0]).all()
    return got0, got, run


# ------------------------------------------------------------------ 1. stream
def test_stream_links_equal_model_and_physics(capi, physics, subsets, margin):
    """4 VGA frames of the PHYSICS stream, ORB-1000 / 500, the two consecutive links"""
    from relative_pose_estimation_amd import synthetic
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(frames[:4], K)
    assert not res[4].any()
    links = [(0, 1, 1), (1, 2, 1)]
    got0, got, _ = _check(e, 3, links, subsets, K, min_shared=sc.PHYSICS_MIN_SHARED, polish=margin)
    R, t, mask, counts, info, rms = got
    assert (info[:, 0] == lp.LINKPOSE_OK).all() and (counts[:, 0] >= sc.PHYSICS_MIN_SHARED).all()
    P = sc.PHYSICS
    Rs, ts = synthetic.stream_poses(P["n_frames"], seed=P["seed"], max_angle_deg=P["max_angle_deg"], step=P["step"])
    Rt, tt = lc.truth_link_poses(Rs, ts, [(0, 1), (1, 2), (2, 3)], links)
    for l in range(2):
        rot = lp.rot_angle_deg(R[l], Rt[l]); nt = np.linalg.norm(t[l])
        print("stream link", links[l], "n", counts[l].tolist(), "rot err %.4f |t| %.4f" % (rot, nt))
        assert rot <= lp.LINK_POSE_ROT_BAND_DEG and abs(nt - 1.0) <= lp.LINK_POSE_SCALE_BAND      # constant step: true ratio 1
    e.close()


# ------------------------------------------------------------------ 2. pair list, every side
def test_pair_list_links_all_sides(capi, physics, subsets, margin):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    s1, s2 = np.array(tgs.PAIRS, np.int32).T
    res = e.estimate_pairs(s1, s2, K)
    assert not res[4].any()
    assert sorted(set(l[2] for l in tgs.LIST_LINKS)) == [0, 1, 2, 3]
    got0, got, _ = _check(e, 6, tgs.LIST_LINKS, subsets, K, polish=margin)
    assert (got[4][:, 0] == lp.LINKPOSE_OK).all()
    # (1, 2) against (0, 1) and (2, 1) against (0, 1): one geometry named from both ends, inverse poses within the bands
    a = e.link_poses([0, 0], [2, 3], [1, 3])
    Ra, ta, Rb, tb = a[0][0], a[1][0], a[0][1], a[1][1]
    assert lp.rot_angle_deg(Ra, Rb.T) <= lp.LINK_POSE_ROT_BAND_DEG and abs(np.linalg.norm(ta) - np.linalg.norm(tb)) <= lp.LINK_POSE_SCALE_BAND
    e.close()


# ------------------------------------------------------------------ 3. duplicate keys
def test_ratio_mode_duplicate_train_keypoints(capi, physics, subsets, margin):
    """RPE_MATCH_RATIO with few features: several matches of a pair name one train keypoint, in pair a and in pair b"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=300, max_matches=200, match_mode=capi.MATCH_RATIO, match_ratio=0.9)
    e.frames_reserve(3)
    e.frames_put(frames[:3], [0, 1, 2])
    res = e.estimate_pairs([0, 2, 1], [1, 1, 2], K)
    assert not res[4].any()
    links = [(0, 1, 3), (1, 0, 3), (0, 2, 1), (2, 1, 1)]
    _, _, run = _check(e, 3, links, subsets, K, min_shared=6, polish=margin)
    for p in (0, 1):                                                     # pairs joined on their train side
        n = int(run.n_matches[p])
        assert (np.unique(run.tidx[p, :n], return_counts=True)[1] > 1).any(), p
    e.close()


# ------------------------------------------------------------------ 4. edges
def test_min_shared_sweep_with_few_matches(capi, physics, subsets, margin):
    """nfeatures = 64, max_matches = 32: n around 6; min_shared swept across every n gives OK and TOO_FEW on either side,
    and never OK below the floor of 6"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=5, nfeatures=64, max_matches=32)
    e.estimate_stream(frames, K)
    links = [(i, i + 1, 1) for i in range(4)] + [(i + 1, i, 2) for i in range(4)]
    got0, _, _ = _check(e, 5, links, subsets, K, min_shared=1)
    n = got0[3][:, 0]
    print("few matches: n", n.tolist(), "codes", got0[4][:, 0].tolist())
    seen = set()
    for ms in range(1, int(n.max()) + 2):
        g, _, _ = _check(e, 5, links, subsets, K, min_shared=ms, polish=margin if ms == 6 else None)
        assert np.array_equal(g[3][:, 0], n)
        assert ((g[4][:, 0] == lp.LINKPOSE_TOO_FEW) == (n < max(ms, 6))).all()
        seen |= set(g[4][:, 0].tolist())
    assert lp.LINKPOSE_TOO_FEW in seen
    e.close()


@pytest.mark.parametrize("iters", [1, 255, 256, 257])
def test_round_edges(capi, physics, subsets, iters, margin):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=2, nfeatures=500, max_matches=250)
    e.estimate_stream(frames[:3], K)
    got0, got, _ = _check(e, 2, [(0, 1, 1), (1, 0, 2)], subsets, K, iters=iters, polish=margin)
    assert (got0[4][:, 1] < iters).all()
    e.close()


def test_blank_frame_codes(capi, physics, subsets, margin):
    """a frame without keypoints: its pairs are RPE_PAIR_NO_DESCRIPTORS with n_matches = 0.  As pair a that is
    PAIR_FAILED; as pair b the match list is defined and empty: TOO_FEW with n = 0, as the header says"""
    frames, K = physics
    f = np.stack([frames[0], frames[1], frames[2], np.full((480, 640), 128, np.uint8), frames[4], frames[5], frames[4]])
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(f, K)
    assert res[4].tolist() == [0, 0, capi.PAIR_NO_DESCRIPTORS, capi.PAIR_NO_DESCRIPTORS, 0, 0]
    assert res[3][2] == 0 and res[3][3] == 0
    links = [(i, i + 1, 1) for i in range(5)] + [(2, 1, 2), (4, 3, 2)]
    got0, got, _ = _check(e, 6, links, subsets, K, polish=margin)
    OK, FAILED, FEW = lp.LINKPOSE_OK, lp.LINKPOSE_PAIR_FAILED, lp.LINKPOSE_TOO_FEW
    assert got[4][:, 0].tolist() == [OK, FEW, FAILED, FAILED, OK, FAILED, FEW]
    assert not got[3][[1, 2, 3, 5, 6]].any()
    e.close()


# ------------------------------------------------------------------ 5. list forms and the largest table
def test_above_the_lds_cut(capi, physics, subsets, margin):
    """max_matches = 1500: the correspondence lists live in device memory, walked in the same order"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=2, nfeatures=4000, max_matches=1500)
    res = e.estimate_stream(frames[:3], K)
    assert not res[4].any() and (res[3] > 1024).all(), res[3]
    got0, got, _ = _check(e, 2, [(0, 1, 1), (1, 0, 2)], subsets, K, polish=margin)
    assert (got[4][:, 0] == lp.LINKPOSE_OK).all() and (got[3][:, 0] > 300).all(), got[3]
    e.close()


def test_capacity_sift_uncapped(capi, subsets, margin):
    """uncapped SIFT at 320 x 240: 16384 + 64 table entries and 8064 matches, the largest layout"""
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(320, 240)
    frames = synthetic.make_stream(3, K, 320, 240, seed=sc.PHYSICS["seed"], step=sc.PHYSICS["step"])[0]
    e = capi.Engine(320, 240, max_batch=2, nfeatures=0, max_matches=capi.MAX_MATCHES_LIMIT, feature_method=capi.FEATURE_SIFT,
                    norm_type=capi.NORM_L2)
    assert e.kcap == capi.SIFT_UNCAPPED_CAPACITY + 64
    res = e.estimate_stream(frames, K)
    assert not res[4].any()
    got0, got, _ = _check(e, 2, [(0, 1, 1), (1, 0, 2)], subsets, K, polish=margin)
    assert (got[4][:, 0] == lp.LINKPOSE_OK).all(), got[4]
    e.close()


# ------------------------------------------------------------------ 6. camera path
def test_camera_pair_list_links(capi, physics, subsets, margin):
    """a pair list on the slots' cameras, two different lenses: the observation is undistorted with C's camera and the
    gate scales with pair b's mean focal length"""
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
    got0, got, _ = _check(e, 3, [(0, 1, 1), (1, 2, 1), (2, 1, 2)], subsets, cams=cams, polish=margin)
    assert (got[4][:, 0] == lp.LINKPOSE_OK).all(), got[4]
    e.close()


# ------------------------------------------------------------------ 7. rotation-only bridge
def test_rotation_only_bridge(capi, subsets, margin):
    """C = S turned about its own centre: the pair's own pose is degenerate as the CPU table says (status OK, hundreds of
    RANSAC inliers, a handful of pose inliers), the link pose has the rotation and |t| ~ 0 inside the bands"""
    frames, K, Rs, ts = lc.rotation_only_frames()
    e = capi.Engine(640, 480, max_batch=2, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(3)
    e.frames_put(frames, [0, 1, 2])
    res = e.estimate_pairs([0, 0], [1, 2], K)
    assert not res[4].any()
    got0, got, run = _check(e, 2, [(0, 1, 0)], subsets, K, polish=margin)
    Rt, _ = lc.truth_link_poses(Rs, ts, [(0, 1), (0, 2)], [(0, 1, 0)])
    rot = lp.rot_angle_deg(got[0][0], Rt[0]); nt = float(np.linalg.norm(got[1][0]))
    print("rotation-only: own pose inliers %d of %d RANSAC inliers; link pose n %s rot err %.4f |t| %.4f" %
          (res[2][1], run.ransac_mask[1].sum(), got[3][0].tolist(), rot, nt))
    assert run.ransac_mask[1].sum() >= 400 and res[2][1] <= 15          # 429 .. 482 -> 0 .. 15
    assert got[4][0, 0] == lp.LINKPOSE_OK and rot <= lp.LINK_POSE_ROT_BAND_DEG and nt <= lp.LINK_POSE_SCALE_BAND
    e.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    ok = ([0, 1], [1, 2], [1, 1])

    def refused(match, a=ok[0], b=ok[1], s=ok[2], **kw):
        with pytest.raises(capi.RpeError, match=match):
            e.link_poses(a, b, s, **kw)

    refused("rpe_link_poses")                                             # before any run
    e.estimate_batch(frames[:2], frames[1:3], K)
    refused("share no frame", [0], [1], [1])                              # a 2-pair batch
    want = e.estimate_stream(frames[:4], K)
    good = e.link_poses(*ok)
    refused("iters", iters=0)
    refused("iters", iters=e.cfg.ransac_max_iters + 1)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        refused("threshold_px", threshold_px=thr)
    refused("refine_iters", refine_iters=-1)
    refused("refine_iters", refine_iters=101)
    refused("two different pairs", [0, 1], [0, 2], [1, 1])
    refused("do not share", [0], [2], [1])
    refused("do not share", [0], [1], [2])
    refused("side must be", [0], [1], [4])
    refused("min_shared", min_shared=0)
    refused("outside the last run", [0], [3], [1])
    with pytest.raises(capi.RpeError, match="4\\*max_batch") as ei:
        e.link_poses([0] * 13, [1] * 13, [1] * 13)
    assert "-3" in str(ei.value)                                           # RPE_ERR_CAPACITY
    again = e.link_poses(*ok)                                              # the handle is still usable
    for x, y in zip(good, again):
        assert np.array_equal(x, y)
    p1, p2 = e.fetch_matched_points(1)
    m = int(want[3][0])
    e.find_essential([p1[0, :m]], [p2[0, :m]], K)                          # a stage call
    refused("stage-API")
    e.estimate_stream(frames[:4], K)
    out = e.link_poses([], [], [])                                         # L = 0 is legal
    assert out[0].shape == (0, 3, 3) and out[3].shape == (0, 2)
    e.close()


# ------------------------------------------------------------------ 9. no side effects, determinism
def test_no_side_effects_and_determinism(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=5, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.estimate_stream(frames, K)
    links = ([0, 1, 2, 3, 1], [1, 2, 3, 4, 0], [1, 1, 1, 1, 2])

    def everything():
        return (tgs._bits(e.fetch_results(5)) + tgs._bits(e.fetch_structure(5)) + tgs._bits(e.refine_poses(5)) +
                tgs._bits(e.scale_links(*links)) + tgs._bits(e.pair_homographies(5)))

    before = everything()
    first = e.link_poses(*links)
    for x, y in zip(before, everything()):
        assert np.array_equal(x, y)
    second = e.link_poses(*links)
    for x, y in zip(tgs._bits(first), tgs._bits(second)):
        assert np.array_equal(x, y)
    fresh = capi.Engine(640, 480, max_batch=5, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    fresh.estimate_stream(frames, K)
    for x, y in zip(tgs._bits(first), tgs._bits(fresh.link_poses(*links))):       # no structure fetch in front of it
        assert np.array_equal(x, y)
    e.close(); fresh.close()


# ------------------------------------------------------------------ 10. trajectory
def test_estimate_trajectory_register(capi, physics):
    from relative_pose_estimation_amd import PoseEstimator, geometry
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    plain = pe.estimate_trajectory(frames)
    again = pe.estimate_trajectory(frames, register=False)
    d = pe.estimate_trajectory(frames, register=True)
    today = {'R', 't', 'inliers', 'status', 'ratio_stats', 'n_shared', 'link_code', 'R_abs', 'T_abs', 'centers', 'baseline', 'segment'}
    assert set(plain) == set(again) == today
    assert set(d) == today | {'R_link', 't_link', 'link_pose_code', 'link_pose_counts', 'R_abs_reg', 'centers_reg'}
    for k in today:
        assert np.array_equal(plain[k], again[k]) and np.array_equal(plain[k], d[k]), k
    i = np.arange(4)
    R, t, mask, counts, info, rms = pe.last_link_poses(np.stack([i, i + 1, np.ones(4, int)], 1))
    for k, v in (('R_link', R), ('t_link', t), ('link_pose_code', info[:, 0]), ('link_pose_counts', counts)):
        assert np.array_equal(d[k], v), k
    want = geometry.chain_trajectory(*geometry.registered_chain_inputs(d['R'], d['t'], d['status'], d['ratio_stats'][:, 1],
                                                                       d['link_code'], R, t, info[:, 0]))
    assert np.array_equal(d['R_abs_reg'], want[0]) and np.array_equal(d['centers_reg'], want[2])
    assert (info[:, 0] == lp.LINKPOSE_OK).all()
    # the registered baselines are the products of the |t_link|: constant step, each inside its band
    assert np.allclose(want[3][1:] / want[3][:-1], np.linalg.norm(t, axis=1), rtol=1e-12)
    assert (np.abs(np.linalg.norm(t, axis=1) - 1.0) <= lp.LINK_POSE_SCALE_BAND).all(), np.linalg.norm(t, axis=1)
    pe.close()
