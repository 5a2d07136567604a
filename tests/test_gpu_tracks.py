"""Multi-view tracks on the GPU (rpe_tracks_from_matches / rpe_build_tracks, through the C-ABI) against the plain Python
model (tests/track_model.py) on all six outputs, exactly: the hand-built graphs of tests/track_cases.py (chains, stars,
repeated / reversed / self pairs, every kind of conflict, the pigeonhole path, tracks of 63 .. 130 frames, min_len, edge
masks, the obs_xy rule, the last node), random graphs, and the run form over a stream and a pair list fed with the GPU's own
fetched indices, masks, statuses and points.  The calls are refused where they must be, change nothing they read and repeat
bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import scale_model as sc
from tests import track_cases as tc
from tests import track_model as tm

pytestmark = pytest.mark.gpu

STAGE_BATCH, STAGE_MM = 136, 32          # chain130 has 129 pairs; the random graphs 24 matches per pair


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def eng(capi):
    """the handle of the stage-form tests: its images are never touched"""
    e = capi.Engine(640, 480, max_batch=STAGE_BATCH, nfeatures=64, max_matches=STAGE_MM)
    assert e.kcap >= 64
    yield e
    e.close()


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


def _ragged(a, m):
    return [a[p, :m[p]] for p in range(len(m))]


def _both(e, case, points=True):
    """(the library's dict, the model's dict) of a case of tests/track_cases.py"""
    P, mm, kc = len(case["frame1"]), e.max_matches, e.kcap
    m = [len(x) for x in case["q"]]
    q, t = tm.pad(case["q"], mm), tm.pad(case["t"], mm)
    edge = np.zeros((P, mm), bool)
    for p in range(P):
        edge[p, :m[p]] = True if case["edge"] is None else np.asarray(case["edge"][p], bool)
    p1, p2 = tc.edge_points(P, mm) if points else (None, None)
    got = e.tracks_from_matches(case["frame1"], case["frame2"], case["q"], case["t"], case["n_frames"],
                                edge=None if case["edge"] is None else case["edge"],
                                pts1=_ragged(p1, m) if points else None, pts2=_ragged(p2, m) if points else None, min_len=case["min_len"])
    want = tm.build_tracks(case["n_frames"], kc, case["frame1"], case["frame2"], q, t, edge, p1, p2, case["min_len"])
    return got, want


# ------------------------------------------------------------------ stage form
@pytest.mark.parametrize("name", [c["name"] for c in tc.cases(64)])
def test_stage_hand_built_cases(eng, name):
    case = {c["name"]: c for c in tc.cases(eng.kcap)}[name]
    got, want = _both(eng, case)
    assert tm.as_lists(want) == case["tracks"]                  # the model still says what was written out by hand
    tm.assert_equal(got, want, name)
    assert got["n_tracks"] == len(case["tracks"]) and got["dropped_conflict"] == case["dropped_conflict"]
    assert got["dropped_short"] == case["dropped_short"] and got["n_edges"] == case["n_edges"]


def test_stage_without_points(eng):
    case = {c["name"]: c for c in tc.cases(eng.kcap)}["conflict_shifts_indices"]
    got, want = _both(eng, case, points=False)
    tm.assert_equal(got, want)
    assert got["n_obs"] == 7 and not got["obs_xy"].any()


@pytest.mark.parametrize("seed", range(10))
def test_stage_random_graphs(eng, seed):
    got, want = _both(eng, tc.random_graph(seed))
    for k, v in tc.RANDOM_FLOORS.items():
        assert want[k] >= v, (k, want[k])
    assert int(np.diff(want["track_start"]).max()) in tc.RANDOM_LONGEST
    tm.assert_equal(got, want, seed)


def test_stage_same_call_twice_identical_bytes(eng):
    g = tc.random_graph(3)
    a, _ = _both(eng, g)
    b, _ = _both(eng, g)
    tm.assert_equal(a, b)


def test_stage_no_pairs_and_no_matches(eng):
    got = eng.tracks_from_matches([], [], [], [], 3)
    assert [got[k] for k in tm.COUNTS] == [0] * 6 and got["track_start"].tolist() == [0] and got["match_track"].shape == (0, STAGE_MM)
    case = dict(n_frames=3, frame1=[0, 1], frame2=[1, 2], q=[[], []], t=[[], []], edge=None, min_len=2)
    got, want = _both(eng, case)
    tm.assert_equal(got, want)
    assert got["n_tracks"] == 0 and got["n_edges"] == 0 and (got["match_track"] == -1).all()


def _raw(e, P, n_frames, f1, f2, m, q, t, edge=None, p1=None, p2=None, min_len=2):
    """rpe_tracks_from_matches itself (the wrapper checks some arguments before the library sees them): the return code"""
    mm = e.max_matches
    n = max(P, 1) * mm
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    f1, f2, m, q, t = i32(f1), i32(f2), i32(m), i32(q), i32(t)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    outs = [np.zeros(6, np.int32), np.zeros(n + 1, np.int32), np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32),
            np.zeros(4 * n, np.float32), np.zeros(n, np.int32)]
    return e.lib.rpe_tracks_from_matches(e.h, P, n_frames, ptr(f1), ptr(f2), ptr(m), ptr(q), ptr(t), ptr(edge), ptr(p1), ptr(p2),
                                         min_len, *map(ptr, outs))


def test_stage_refusals_leave_the_handle_usable(eng, capi):
    e, mm, kc = eng, eng.max_matches, eng.kcap
    case = {c["name"]: c for c in tc.cases(kc)}["chain5"]
    good, want = _both(e, case)
    tm.assert_equal(good, want)
    q = np.zeros((2, mm), np.int32); t = np.zeros((2, mm), np.int32)
    pts = np.zeros((2, mm, 2), np.float32)
    ok = dict(P=2, n_frames=3, f1=[0, 1], f2=[1, 2], m=[1, 1], q=q, t=t)
    INVALID, CAPACITY = -1, -3
    assert _raw(e, **ok) == 0

    def bad(code, **kw):
        assert _raw(e, **{**ok, **kw}) == code, kw
        assert e.lib.rpe_last_error(e.h)
    bad(INVALID, P=-1)
    big = STAGE_BATCH + 1
    zq = np.zeros((big, mm), np.int32)
    bad(CAPACITY, P=big, f1=[0] * big, f2=[1] * big, m=[0] * big, q=zq, t=zq)
    bad(INVALID, n_frames=0)
    bad(INVALID, n_frames=(1 << 31) // kc + 1)                               # n_frames * KC >= 2^31
    bad(INVALID, f1=[0, 3])
    bad(INVALID, f2=[-1, 2])
    bad(INVALID, m=[1, mm + 1])
    bad(INVALID, m=[-1, 1])
    qb = q.copy(); qb[1, 0] = kc
    bad(INVALID, q=qb)
    tb = t.copy(); tb[0, 0] = -1
    bad(INVALID, t=tb)
    qt = q.copy(); qt[1, 1] = kc                                              # past m[1]: not looked at
    assert _raw(e, **{**ok, "q": qt}) == 0
    bad(INVALID, p1=pts)
    bad(INVALID, p2=pts)
    bad(INVALID, min_len=1)
    again, _ = _both(e, case)                                                 # the next valid call succeeds, same bytes
    tm.assert_equal(again, good)


# ------------------------------------------------------------------ run form
def _fetch_run(e, P):
    """the last run as the model takes it, from the C-ABI's fetches"""
    R, t, inl, nm, st = e.fetch_results(P)
    q, ti = e.fetch_match_indices(P)
    rm, pm, pts = e.fetch_structure(P)
    p1, p2 = e.fetch_matched_points(P)
    return sc.Run(q, ti, rm, pm, pts, R, t, st, nm), p1, p2


def _check_run(e, P, n_frames, f1, f2, rule, min_len=2, use_pair=None):
    got = e.build_tracks(use_pair=use_pair, edge_rule=rule, min_len=min_len)        # before any structure fetch
    run, p1, p2 = _fetch_run(e, P)
    want = tm.build_tracks(n_frames, e.kcap, f1, f2, run.qidx, run.tidx, tm.run_edges(run, rule, use_pair), p1, p2, min_len)
    tm.assert_equal(got, want, (rule, min_len))
    return got


def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrs]


def test_stream_three_rules_no_side_effects(capi, physics):
    """4 VGA frames of the PHYSICS stream, ORB-1000 / 500: each edge rule equals the model, the run's fetches return the bits
    they returned before, and a stage-form call between the run and its fetches leaves the run fetchable"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(frames[:4], K)
    assert not res[4].any()
    f1, f2 = np.arange(3), np.arange(3) + 1
    n_edges = []
    for rule in (capi.TRACK_EDGES_USABLE, capi.TRACK_EDGES_RANSAC, capi.TRACK_EDGES_ALL):
        got = _check_run(e, 3, 4, f1, f2, rule)
        print("stream rule", rule, {k: got[k] for k in tm.COUNTS}, "lengths", np.bincount(np.diff(got["track_start"])).tolist())
        assert got["n_tracks"] > 100 and int(np.diff(got["track_start"]).max()) >= 3 and got["n_frames_seen"] == 4
        n_edges.append(got["n_edges"])
    assert n_edges[0] <= n_edges[1] <= n_edges[2] == int(res[3].sum())
    _check_run(e, 3, 4, f1, f2, capi.TRACK_EDGES_USABLE, min_len=4)
    before = _bits(e.fetch_results(3)) + _bits(e.fetch_structure(3)) + _bits(e.fetch_match_indices(3)) + _bits(e.fetch_matched_points(3))
    first = e.build_tracks()
    e.tracks_from_matches([0], [1], [[1]], [[1]], 2)                                # the stage form uses buffers of its own
    second = e.build_tracks()
    tm.assert_equal(first, second)
    after = _bits(e.fetch_results(3)) + _bits(e.fetch_structure(3)) + _bits(e.fetch_match_indices(3)) + _bits(e.fetch_matched_points(3))
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    e.close()


def test_pair_list_window_with_reversed_pair(capi, physics):
    """window 2 over 5 slots of an 8-slot store, pair (2, 3) reversed: the shared slot is image 2 of one pair and image 1 of
    another; with every pair and with one switched off"""
    frames, K = physics
    slots = [1, 2, 3, 5, 6]
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (3, 2), (2, 4), (3, 4)]
    s1 = np.array([slots[a] for a, _ in pairs], np.int32); s2 = np.array([slots[b] for _, b in pairs], np.int32)
    e = capi.Engine(640, 480, max_batch=7, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    e.frames_reserve(8)
    e.frames_put(frames[:5], slots)
    res = e.estimate_pairs(s1, s2, K)
    assert not res[4].any()
    full = _check_run(e, 7, 8, s1, s2, capi.TRACK_EDGES_USABLE)
    assert set(full["obs_frame"].tolist()) == set(slots) and full["n_frames_seen"] == 5
    assert int(np.diff(full["track_start"]).max()) >= 4                            # longer than a link's three views
    print("pair list", {k: full[k] for k in tm.COUNTS}, "lengths", np.bincount(np.diff(full["track_start"])).tolist())
    use = np.array([1, 1, 1, 1, 0, 1, 1], bool)
    part = _check_run(e, 7, 8, s1, s2, capi.TRACK_EDGES_USABLE, use_pair=use)
    assert part["n_edges"] < full["n_edges"] and (part["match_track"][4] == -1).all()
    _check_run(e, 7, 8, s1, s2, capi.TRACK_EDGES_ALL, min_len=3, use_pair=use)
    with pytest.raises(ValueError):
        e.build_tracks(use_pair=[1, 1])
    e.close()


def test_estimate_trajectory_carries_the_tracks(capi, physics):
    from relative_pose_estimation_amd import PoseEstimator, geometry
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    plain = pe.estimate_trajectory(frames)
    assert set(plain) == {'R', 't', 'inliers', 'status', 'ratio_stats', 'n_shared', 'link_code', 'R_abs', 'T_abs', 'centers', 'baseline', 'segment'}
    d = pe.estimate_trajectory(frames, tracks=True)
    assert set(d) == set(plain) | {'tracks'}
    for k in plain:
        assert np.array_equal(np.ascontiguousarray(d[k]).view(np.uint8), np.ascontiguousarray(plain[k]).view(np.uint8)), k
    tm.assert_equal(d['tracks'], pe.last_tracks())
    tm.assert_equal(pe.last_tracks(edge_rule=capi.TRACK_EDGES_ALL, min_len=3), pe._last_engine.build_tracks(None, capi.TRACK_EDGES_ALL, 3))
    lengths = geometry.track_lengths(d['tracks'])
    assert lengths.sum() == d['tracks']['n_obs'] and lengths.min() >= 2 and lengths.max() >= 4
    t, obs = geometry.tracks_of_frames(d['tracks'], [0, 1, 2])
    assert t.size > 0 and (d['tracks']['obs_frame'][obs] == [0, 1, 2]).all()
    with pytest.raises(capi.RpeError, match="share no frame"):
        pe.estimate_batch(frames[:2], frames[1:3])
        pe.last_tracks()
    pe.close()


def test_run_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)

    def refused(match, **kw):
        with pytest.raises(capi.RpeError, match=match) as ei:
            e.build_tracks(**kw)
        assert "error -1" in str(ei.value)                                     # RPE_ERR_INVALID

    refused("rpe_build_tracks")                                               # before any run
    e.estimate_batch(frames[:2], frames[1:3], K)
    refused("share no frame")                                                 # a 2-pair batch
    want = e.estimate_stream(frames[:4], K)
    good = e.build_tracks()
    refused("edge_rule", edge_rule=3)
    refused("edge_rule", edge_rule=-1)
    refused("min_len", min_len=1)
    tm.assert_equal(e.build_tracks(), good)
    p1, p2 = e.fetch_matched_points(1)
    m = int(want[3][0])
    e.find_essential([p1[0, :m]], [p2[0, :m]], K)                              # a stage call
    refused("stage-API")
    e.frames_reserve(4)
    e.estimate_stream(frames[:4], K)
    e.frames_put(frames[:2], [0, 1])                                           # a put
    refused("rpe_build_tracks")
    e.frames_put(frames[:4], [0, 1, 2, 3])
    e.estimate_pairs([0, 1, 2], [1, 2, 3], K)
    lst = e.build_tracks()
    tm.assert_equal(lst, good)                                                 # the same pairs as the stream's, slots = frames
    e.frames_reserve(6)                                                        # the store resized under the list
    refused("resized")
    e.estimate_pairs([0, 1, 2], [1, 2, 3], K)
    bigger = e.build_tracks()                                                  # 6 slots now: the node arrays grow
    tm.assert_equal(bigger, good)
    e.close()


def test_refused_after_a_chunked_host_batch(capi, K_vga):
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(1, K_vga, cfg=2)
    B = 512
    a = np.ascontiguousarray(np.broadcast_to(i1, (B, 480, 640))); b = np.ascontiguousarray(np.broadcast_to(i2, (B, 480, 640)))
    e = capi.Engine(640, 480, max_batch=B, nfeatures=200, max_matches=100)
    e.estimate_batch(a, b, K_vga)                                              # >= 512 pairs, 150 MiB per set: chunked
    with pytest.raises(capi.RpeError, match="ran in chunks"):
        e.build_tracks()
    e.close()


def test_outputs_are_sized_by_the_library_pair_count(capi, physics):
    """estimate() is a batch of ONE pair, which the library serves as the stream of its two images: last_tracks() returns its
    tracks of two observations.  The outputs follow rpe_last_run_pairs, whatever ran before and whatever was refused since."""
    from relative_pose_estimation_amd import PoseEstimator
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    pe.estimate_sequence(frames)                                              # 5 pairs first: nothing of it may linger
    e = pe._last_engine
    assert e.lib.rpe_last_run_pairs(e.h) == 5
    long = pe.last_tracks()
    assert long["match_track"].shape == (5, e.max_matches)
    pe.estimate(frames[0], frames[1])
    assert pe._last_engine is e and e.lib.rpe_last_run_pairs(e.h) == 1
    got = pe.last_tracks()
    run, p1, p2 = _fetch_run(e, 1)
    want = tm.build_tracks(2, e.kcap, [0], [1], run.qidx, run.tidx, tm.run_edges(run, tm.EDGES_USABLE), p1, p2, 2)
    tm.assert_equal(got, want)
    assert got["match_track"].shape == (1, e.max_matches) and got["n_tracks"] > 100 and (np.diff(got["track_start"]) == 2).all()
    pe.estimate_batch(frames[:2], frames[1:3])                                # two pairs: refused, nothing written
    assert e.lib.rpe_last_run_pairs(e.h) == 2
    with pytest.raises(capi.RpeError, match="share no frame"):
        pe.last_tracks()
    pe.estimate_sequence(frames[:4])                                          # 3 pairs
    with pytest.raises(capi.RpeError):
        e.estimate_pairs([0], [1], K)                                         # refused (no store): the stream stays the last run
    assert e.lib.rpe_last_run_pairs(e.h) == 3
    assert pe.last_tracks()["match_track"].shape == (3, e.max_matches)
    pe.close()
    fresh = capi.Engine(640, 480, max_batch=2, nfeatures=64, max_matches=32)
    assert fresh.lib.rpe_last_run_pairs(fresh.h) == 0
    with pytest.raises(capi.RpeError, match="rpe_build_tracks"):
        fresh.build_tracks()
    fresh.close()
