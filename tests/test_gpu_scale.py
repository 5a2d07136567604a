"""Scale links on the GPU (rpe_fetch_match_indices / rpe_scale_links, through the C-ABI): the kernel's join, ratios and
order statistics equal the float64 model (tests/scale_model.py) fed with the GPU's own fetched indices, structure and
poses -- for streams and pair lists, every `side`, duplicate keys, the edges of min_shared, failed pairs, the largest
LDS layouts and the camera path -- the medians lie inside the band fixed from the CPU oracle, the call is refused where
it must be and changes nothing it reads."""
import numpy as np
import pytest

from tests import scale_model as sc

pytestmark = pytest.mark.gpu

RTOL = 1e-12      # same doubles in, about five correctly rounded operations: a few ulp; far below the spacing of the ratios


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


def _fetch_run(e, P):
    """the last run as the model takes it, from the C-ABI's fetches"""
    R, t, inl, nm, st = e.fetch_results(P)
    q, ti = e.fetch_match_indices(P)
    rm, pm, pts = e.fetch_structure(P)
    for p in range(P):
        n = min(int(nm[p]), e.max_matches)
        assert (q[p, n:] == -1).all() and (ti[p, n:] == -1).all(), p
        assert (q[p, :n] >= 0).all() and (q[p, :n] < e.kcap).all() and (ti[p, :n] >= 0).all() and (ti[p, :n] < e.kcap).all(), p
    return sc.Run(q, ti, rm, pm, pts, R, t, st, nm)


def _check_links(e, P, links, min_shared=8):
    """rpe_scale_links (called BEFORE any structure fetch: it launches the structure kernels itself) == the model"""
    links = np.asarray(links, np.int32).reshape(-1, 3)
    stats, n, code = e.scale_links(links[:, 0], links[:, 1], links[:, 2], min_shared)
    run = _fetch_run(e, P)
    ms, mn, mc = sc.scale_links(run, links, min_shared)
    assert np.array_equal(n, mn), (n, mn)
    assert np.array_equal(code, mc), (code, mc)
    assert np.allclose(stats, ms, rtol=RTOL, atol=0), (stats, ms)
    assert not stats[code != sc.LINK_OK].any()
    return stats, n, code, run


# ------------------------------------------------------------------ 1. stream
def test_stream_links_equal_model_and_physics(capi, physics):
    """4 VGA frames of the PHYSICS stream, ORB-1000 / 500, the two consecutive links"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(frames[:4], K)
    assert not res[4].any()
    stats, n, code, _ = _check_links(e, 3, [(0, 1, 1), (1, 2, 1)])
    print("stream links: n_shared", n.tolist(), "quartiles / median", stats.tolist())
    assert (code == sc.LINK_OK).all() and (n >= sc.PHYSICS_MIN_SHARED).all()
    assert (np.abs(stats[:, 1] - 1.0) <= sc.SCALE_BAND).all(), stats[:, 1]          # constant step: true ratio 1
    assert (stats[:, 0] <= stats[:, 1]).all() and (stats[:, 1] <= stats[:, 2]).all()
    e.close()


# ------------------------------------------------------------------ 2. pair list, every side
PAIRS = [(0, 1), (0, 2), (1, 2), (2, 1), (1, 3), (2, 3)]
LIST_LINKS = [(0, 1, 0),      # (0,1) (0,2) at slot 0: image 1 of both
              (0, 2, 1),      # (0,1) (1,2) at slot 1: image 2 of a, image 1 of b
              (2, 0, 2),      # (1,2) (0,1) at slot 1: image 1 of a, image 2 of b
              (1, 2, 3),      # (0,2) (1,2) at slot 2: image 2 of both
              (2, 3, 2),      # (1,2) and its reverse (2,1) at slot 1
              (2, 3, 1),      # ... and at slot 2
              (3, 5, 0),      # (2,1) (2,3) at slot 2
              (4, 5, 3)]      # (1,3) (2,3) at slot 3


def test_pair_list_links_all_sides(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    kps, _, cnt = e.orb_detect_and_compute(frames[:4])                  # the keypoints the slots will hold
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    s1, s2 = np.array(PAIRS, np.int32).T
    res = e.estimate_pairs(s1, s2, K)
    assert not res[4].any()
    assert sorted(set(l[2] for l in LIST_LINKS)) == [0, 1, 2, 3]
    stats, n, code, run = _check_links(e, 6, LIST_LINKS)
    assert (code == sc.LINK_OK).all() and (n >= sc.PHYSICS_MIN_SHARED).all()
    assert np.array_equal(n[4], n[5])           # crossCheck: (1,2) and (2,1) share the same keypoints at either frame
    # the indices of the reversed pair (2, 1) name the keypoints of slots 2 and 1 its matched points came from
    p1, p2 = e.fetch_matched_points(6)
    m = int(res[3][3])
    q, t = run.qidx[3, :m], run.tidx[3, :m]
    assert (q < cnt[2]).all() and (t < cnt[1]).all()
    assert np.array_equal(p1[3, :m, 0], kps[2]["x"][q]) and np.array_equal(p1[3, :m, 1], kps[2]["y"][q])
    assert np.array_equal(p2[3, :m, 0], kps[1]["x"][t]) and np.array_equal(p2[3, :m, 1], kps[1]["y"][t])
    assert len(set(q.tolist())) == m and len(set(t.tolist())) == m      # crossCheck: one match per keypoint
    e.close()


# ------------------------------------------------------------------ 3. duplicate keys
def test_ratio_mode_duplicate_train_keypoints(capi, physics):
    """RPE_MATCH_RATIO with few features: several usable matches of a pair name one train keypoint (configuration picked
    on the CPU with oracle.match_hamming_ratio: 20 .. 33 such keypoints per pair), in pair a and in pair b"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=300, max_matches=200, match_mode=capi.MATCH_RATIO, match_ratio=0.9)
    e.frames_reserve(3)
    e.frames_put(frames[:3], [0, 1, 2])
    res = e.estimate_pairs([0, 2, 1], [1, 1, 2], K)
    assert not res[4].any()
    links = [(0, 1, 3), (1, 0, 3), (0, 2, 1), (2, 1, 1)]
    stats, n, code, run = _check_links(e, 3, links, min_shared=4)
    for p in (0, 1):                                                     # pairs joined on their train side
        us = run.ransac_mask[p] & run.pose_mask[p]
        keys, counts = np.unique(run.tidx[p][us], return_counts=True)
        assert (counts > 1).any(), p
    assert (code == sc.LINK_OK).all()
    e.close()


# ------------------------------------------------------------------ 4. edges
def test_min_shared_sweep_with_few_matches(capi, physics):
    """nfeatures = 64, max_matches = 32: a handful of shared keypoints per link; min_shared swept from 1 to past the
    largest n_shared gives LINK_OK and LINK_TOO_FEW on either side of every n_shared"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=5, nfeatures=64, max_matches=32)
    e.estimate_stream(frames, K)
    links = [(i, i + 1, 1) for i in range(4)] + [(i + 1, i, 2) for i in range(4)]
    _, n, _, _ = _check_links(e, 5, links, min_shared=1)
    print("few matches: n_shared", n.tolist())
    seen = set()
    for ms in range(1, int(n.max()) + 2):
        _, n2, code, _ = _check_links(e, 5, links, min_shared=ms)
        assert np.array_equal(n2, n)
        seen |= set(code.tolist())
    assert sc.LINK_TOO_FEW in seen
    e.close()


def test_blank_frame_fails_its_links(capi, physics):
    frames, K = physics
    f = np.stack([frames[0], frames[1], frames[2], np.full((480, 640), 128, np.uint8), frames[4], frames[5], frames[4]])
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(f, K)
    assert res[4].tolist() == [0, 0, capi.PAIR_NO_DESCRIPTORS, capi.PAIR_NO_DESCRIPTORS, 0, 0]
    stats, n, code, _ = _check_links(e, 6, [(i, i + 1, 1) for i in range(5)])
    assert code.tolist() == [sc.LINK_OK, sc.LINK_PAIR_FAILED, sc.LINK_PAIR_FAILED, sc.LINK_PAIR_FAILED, sc.LINK_OK]
    assert not n[1:4].any() and not stats[1:4].any()
    e.close()


# ------------------------------------------------------------------ 5. capacity
def test_capacity_orb_8000_untruncated(capi, physics):
    """ORB nfeatures = 8000, max_matches = None (8064): 64 KB of ratios + 31.5 KB of table, above the default LDS limit"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=2, nfeatures=8000, max_matches=capi.MAX_MATCHES_LIMIT)
    res = e.estimate_stream(frames[:3], K)
    assert not res[4].any() and (res[3] > 1000).all()
    stats, n, code, _ = _check_links(e, 2, [(0, 1, 1), (1, 0, 2)])
    assert (code == sc.LINK_OK).all() and (n > 500).all(), n
    assert n[0] == n[1]                         # the same link named from either end
    e.close()


def test_capacity_sift_uncapped(capi):
    """uncapped SIFT at 320 x 240: 16384 table entries + 8192 ratios, the largest LDS layout (128 KB)"""
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(320, 240)
    frames = synthetic.make_stream(3, K, 320, 240, seed=sc.PHYSICS["seed"], step=sc.PHYSICS["step"])[0]
    e = capi.Engine(320, 240, max_batch=2, nfeatures=0, max_matches=capi.MAX_MATCHES_LIMIT, feature_method=capi.FEATURE_SIFT,
                    norm_type=capi.NORM_L2)
    assert e.kcap == capi.SIFT_UNCAPPED_CAPACITY + 64
    res = e.estimate_stream(frames, K)
    assert not res[4].any()
    stats, n, code, _ = _check_links(e, 2, [(0, 1, 1), (1, 0, 2)])
    assert (code == sc.LINK_OK).all(), (code, n)
    e.close()


# ------------------------------------------------------------------ 6. camera path
def test_camera_pair_list_links(capi, physics):
    """a pair list on the slots' cameras, two different lenses: the points are in normalised coordinates, the call is the
    same"""
    frames, K = physics
    K2 = K.copy(); K2[0, 0] *= 1.01; K2[1, 1] *= 1.01
    camA = capi.Camera(K, [-0.02, 0.005, 0.0004, -0.0003]); camB = capi.Camera(K2, [0.015, -0.004, 0.0, 0.0002, 0.001])
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    e.frames_set_cameras([0, 1, 2, 3], [camA, camB, camA, camB])
    res = e.estimate_pairs_cameras([0, 1, 2], [1, 2, 3])
    assert not res[4].any()
    stats, n, code, _ = _check_links(e, 3, [(0, 1, 1), (1, 2, 1), (2, 1, 2)])
    assert (code == sc.LINK_OK).all(), (code, n)
    e.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    ok = ([0, 1], [1, 2], [1, 1])

    def refused(match, a=ok[0], b=ok[1], s=ok[2], min_shared=8):
        with pytest.raises(capi.RpeError, match=match):
            e.scale_links(a, b, s, min_shared)

    refused("rpe_scale_links")                                            # before any run
    e.estimate_batch(frames[:2], frames[1:3], K)
    refused("share no frame", [0], [1], [1])                              # a 2-pair batch
    want = e.estimate_stream(frames[:4], K)
    good = e.scale_links(*ok)
    p1, p2 = e.fetch_matched_points(1)
    m = int(want[3][0])
    e.find_essential([p1[0, :m]], [p2[0, :m]], K)                          # a stage call
    refused("stage-API")
    e.frames_reserve(4)
    e.estimate_stream(frames[:4], K)
    e.frames_put(frames[:2], [0, 1])                                       # a put
    refused("rpe_scale_links")
    e.estimate_stream(frames[:4], K)
    refused("two different pairs", [0, 1], [0, 2], [1, 1])                 # a == b
    refused("do not share", [0], [2], [1])                                 # stream: frames differ
    refused("do not share", [0], [1], [2])
    refused("side must be", [0], [1], [4])
    refused("min_shared", min_shared=0)
    refused("outside the last run", [0], [3], [1])
    with pytest.raises(capi.RpeError, match="4\\*max_batch") as ei:
        e.scale_links([0] * 13, [1] * 13, [1] * 13)
    assert "-3" in str(ei.value)                                           # RPE_ERR_CAPACITY
    again = e.scale_links(*ok)                                             # the handle is still usable
    for x, y in zip(good, again):
        assert np.array_equal(x, y)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    e.estimate_pairs([0, 1, 2], [1, 2, 3], K)
    refused("do not share", [0], [2], [1])                                 # list: slots 1 and 2 differ
    lst = e.scale_links(*ok)
    for x, y in zip(good, lst):                                            # the same pairs as the stream's
        assert np.array_equal(x, y)
    stats, n, code = e.scale_links([], [], [])                             # L = 0 is legal
    assert stats.shape == (0, 3) and n.size == 0
    e.close()


# ------------------------------------------------------------------ 8. no side effects, determinism
def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrs]


def test_no_side_effects_and_determinism(capi, physics):
    from relative_pose_estimation_amd import synthetic
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=16, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    plain = capi.Engine(640, 480, max_batch=16, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.estimate_stream(frames, K)
    before = _bits(e.fetch_results(5)) + _bits(e.fetch_structure(5)) + _bits(e.refine_poses(5))
    links = ([0, 1, 2, 3, 1], [1, 2, 3, 4, 0], [1, 1, 1, 1, 2])
    first = e.scale_links(*links)
    after = _bits(e.fetch_results(5)) + _bits(e.fetch_structure(5)) + _bits(e.refine_poses(5))
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    second = e.scale_links(*links)
    for x, y in zip(_bits(first), _bits(second)):
        assert np.array_equal(x, y)
    # streams of B = 1 .. 16 pairs: the same results with and without the call in between
    long = synthetic.make_stream(17, K, seed=sc.PHYSICS["seed"], step=sc.PHYSICS["step"])[0]
    for B in range(1, 17):
        ra = e.estimate_stream(long[:B + 1], K)
        if B >= 2:
            i = np.arange(B - 1)
            e.scale_links(i, i + 1, np.ones(B - 1, np.int32))
        rb = plain.estimate_stream(long[:B + 1], K)
        for x, y in zip(_bits(ra), _bits(rb)):
            assert np.array_equal(x, y), B
        for x, y in zip(_bits(e.fetch_results(B)), _bits(rb)):
            assert np.array_equal(x, y), B
    e.close(); plain.close()


# ------------------------------------------------------------------ 9. trajectory
def test_estimate_trajectory(capi, physics):
    from relative_pose_estimation_amd import PoseEstimator, geometry
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    d = pe.estimate_trajectory(frames)
    assert set(d) == {'R', 't', 'inliers', 'status', 'ratio_stats', 'n_shared', 'link_code', 'R_abs', 'T_abs', 'centers', 'baseline', 'segment'}
    R, t, inl, st = pe.estimate_sequence(frames)
    i = np.arange(4)
    stats, n, code = pe.last_scale_links(np.stack([i, i + 1, np.ones(4, int)], 1))
    for k, v in (('R', R), ('t', t), ('inliers', inl), ('status', st), ('ratio_stats', stats), ('n_shared', n), ('link_code', code)):
        assert np.array_equal(d[k], v), k
    want = geometry.chain_trajectory(R, t, st, stats[:, 1], code)
    for k, v in zip(('R_abs', 'T_abs', 'centers', 'baseline', 'segment'), want):
        assert np.array_equal(d[k], v), k
    assert not st.any() and (code == sc.LINK_OK).all() and not d['segment'].any()
    print("trajectory baselines", d['baseline'].tolist())
    assert (np.abs(d['baseline'] - 1.0) <= sc.SCALE_BAND).all(), d['baseline']      # constant step: every baseline is 1
    assert (np.abs(d['baseline'][1:] / d['baseline'][:-1] - 1.0) <= sc.SCALE_BAND).all()
    with pytest.raises(capi.RpeError, match="share no frame"):
        pe.estimate_batch(frames[:2], frames[1:3])
        pe.last_scale_links(np.array([[0, 1, 1]]))
    pe.close()
