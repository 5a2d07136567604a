"""CPU tests of the multi-view tracks: the model (tests/track_model.py) against scipy's connected components and against the
hand-built cases with their tracks written out by hand, the model on the CPU oracle's run of a short stream, the C-ABI
surface, and the two geometry helpers."""
import os
import re

import numpy as np
import pytest

from tests import track_cases as tc
from tests import track_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KC, MM = 64, 32


def model_of(case, kc=KC, mm=MM, points=True):
    """the model's dict of a case of tests/track_cases.py"""
    P = len(case["frame1"])
    q, t = tm.pad(case["q"], mm), tm.pad(case["t"], mm)
    e = np.zeros((P, mm), bool)
    for p in range(P):
        e[p, :len(case["q"][p])] = True if case["edge"] is None else np.asarray(case["edge"][p], bool)
    p1, p2 = tc.edge_points(P, mm) if points else (None, None)
    return tm.build_tracks(case["n_frames"], kc, case["frame1"], case["frame2"], q, t, e, p1, p2, case["min_len"])


def check_consistency(tr, frame1, qidx, edge, kc):
    """what any tracks dict must satisfy: CSR offsets, ordered observations in distinct frames, match_track naming the track
    that holds the edge's node"""
    s = tr["track_start"]
    assert s[0] == 0 and s[-1] == tr["n_obs"] == len(tr["obs_frame"]) and len(s) == tr["n_tracks"] + 1 and (np.diff(s) >= 2).all()
    ids = tr["obs_frame"].astype(np.int64) * kc + tr["obs_kp"]
    assert len(set(ids.tolist())) == len(ids)
    for j in range(tr["n_tracks"]):
        f = tr["obs_frame"][s[j]:s[j + 1]]
        assert len(set(f.tolist())) == len(f), j                                   # one keypoint per frame
        assert (np.diff(ids[s[j]:s[j + 1]]) > 0).all(), j                          # observations by ascending node id
    assert (np.diff(ids[s[:-1]]) > 0).all()                                        # tracks by ascending smallest node id
    assert tr["n_frames_seen"] == len(set(tr["obs_frame"].tolist()))
    mt = tr["match_track"]
    assert (mt[~edge] == -1).all() and mt.max(initial=-1) < tr["n_tracks"]
    for p, i in zip(*np.nonzero(mt >= 0)):
        j = mt[p, i]
        assert frame1[p] * kc + qidx[p, i] in ids[s[j]:s[j + 1]], (p, i)
    assert set(mt[mt >= 0].tolist()) == set(range(tr["n_tracks"]))                 # every track has an edge


@pytest.mark.parametrize("case", tc.cases(KC), ids=lambda c: c["name"])
def test_model_on_hand_built_cases(case):
    tr = model_of(case)
    assert tm.as_lists(tr) == case["tracks"]
    for k in ("dropped_conflict", "dropped_short", "n_edges"):
        assert tr[k] == case[k], k
    check_consistency(tr, case["frame1"], tm.pad(case["q"], MM), _edges(case), KC)


def _edges(case):
    e = np.zeros((len(case["frame1"]), MM), bool)
    for p in range(len(case["frame1"])):
        e[p, :len(case["q"][p])] = True if case["edge"] is None else np.asarray(case["edge"][p], bool)
    return e


def test_model_xy_rule_by_hand():
    """obs_xy: the point of the lowest edge id that names the node, image 1's when that edge names it on both sides"""
    cs = {c["name"]: c for c in tc.cases(KC)}
    p1, p2 = tc.edge_points(2, MM)
    tr = model_of(cs["xy_lowest_edge"])
    assert np.array_equal(tr["obs_xy"], np.stack([p1[0, 0], p2[0, 0], p2[1, 0]]))           # (1, 1): pair 0's image 2, not pair 1's image 1
    tr = model_of(cs["xy_both_sides"])
    assert np.array_equal(tr["obs_xy"], np.stack([p1[1, 0], p1[0, 0]]))                     # (1, 1): the self pair's image 1
    assert not model_of(cs["xy_both_sides"], points=False)["obs_xy"].any()


@pytest.mark.parametrize("seed", range(10))
def test_model_partition_equals_scipy(seed):
    """a second opinion on the partition: scipy.sparse.csgraph.connected_components over the same edges"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = tc.random_graph(seed)
    tr = model_of(g)
    q, t = tm.pad(g["q"], MM), tm.pad(g["t"], MM)
    e = _edges(g)
    f1, f2 = np.array(g["frame1"]), np.array(g["frame2"])
    a = (f1[:, None] * KC + q)[e]; b = (f2[:, None] * KC + t)[e]
    N = g["n_frames"] * KC
    _, lab = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(N, N)), directed=False)
    used = np.unique(np.concatenate([a, b]))
    want, conflict, short = [], 0, 0
    for c in np.unique(lab[used]):
        nodes = used[lab[used] == c]
        if len(set((nodes // KC).tolist())) != len(nodes):
            conflict += 1
        elif len(nodes) < g["min_len"]:
            short += 1
        else:
            want.append([(int(n // KC), int(n % KC)) for n in nodes])
    want.sort()
    assert tm.as_lists(tr) == want
    assert (tr["dropped_conflict"], tr["dropped_short"], tr["n_edges"]) == (conflict, short, int(e.sum()))
    check_consistency(tr, f1, q, e, KC)
    # the floors of the generator: no branch goes unexercised
    for k, v in tc.RANDOM_FLOORS.items():
        assert tr[k] >= v, (k, tr[k])
    assert int(np.diff(tr["track_start"]).max()) in tc.RANDOM_LONGEST


def test_model_on_the_oracle_stream(oracle, K_vga):
    """the CPU oracle's run of a 4-frame stream under the three edge rules"""
    from tests import scale_model as sc
    frames, K = sc.physics_frames()
    pairs = [(0, 1), (1, 2), (2, 3)]
    run = sc.oracle_run(oracle, frames[:4], pairs, K, nfeatures=300, max_matches=200)
    f1, f2 = np.array(pairs).T
    kc = int(max(run.qidx.max(), run.tidx.max())) + 1
    n_edges = []
    for rule in (tm.EDGES_USABLE, tm.EDGES_RANSAC, tm.EDGES_ALL):
        e = tm.run_edges(run, rule)
        tr = tm.build_tracks(4, kc, f1, f2, run.qidx, run.tidx, e, None, None, 2)
        check_consistency(tr, f1, run.qidx, e, kc)
        assert tr["n_edges"] == int(e.sum()) and tr["n_tracks"] > 20 and int(np.diff(tr["track_start"]).max()) == 4
        n_edges.append(tr["n_edges"])
    assert n_edges[0] <= n_edges[1] <= n_edges[2] == int(run.n_matches.sum())
    off = tm.run_edges(run, tm.EDGES_ALL, use_pair=[1, 0, 1])
    assert not off[1].any() and off[0].sum() == run.n_matches[0]


def test_track_surface_exists():
    """the binding table names both entries and the header declares them (fails without the feature)"""
    from relative_pose_estimation_amd import _capi
    src = open(os.path.join(ROOT, "include", "rpe_amd.h")).read()
    for name, nargs in (("rpe_build_tracks", 10), ("rpe_tracks_from_matches", 18)):
        assert name in _capi.EXPORTS
        assert len(_capi.SIGNATURES[name][1]) == nargs
        m = re.search(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", src)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert "rpe_last_run_pairs" in _capi.EXPORTS and re.search(r"\bint\s+rpe_last_run_pairs\s*\(\s*const rpe_handle \*h\s*\)\s*;", src)
    assert _capi.load().rpe_last_run_pairs(None) == 0
    assert (_capi.TRACK_EDGES_USABLE, _capi.TRACK_EDGES_RANSAC, _capi.TRACK_EDGES_ALL) == (0, 1, 2)
    assert re.search(r"RPE_TRACK_EDGES_USABLE\s*=\s*0\s*,\s*RPE_TRACK_EDGES_RANSAC\s*=\s*1\s*,\s*RPE_TRACK_EDGES_ALL\s*=\s*2", src)
    assert _capi.TRACK_COUNTS == tm.COUNTS
    assert hasattr(_capi.load(), "rpe_build_tracks") and hasattr(_capi.load(), "rpe_tracks_from_matches")
    from relative_pose_estimation_amd import PoseEstimator
    assert callable(PoseEstimator.last_tracks)


def test_geometry_helpers():
    from relative_pose_estimation_amd import geometry
    cs = {c["name"]: c for c in tc.cases(KC)}
    tr = model_of(cs["min_len2"])            # tracks: frames 0 .. 4, frames 0 .. 2, frames 3 .. 4
    assert geometry.track_lengths(tr).tolist() == [5, 3, 2]
    t, obs = geometry.tracks_of_frames(tr, [0, 2])
    assert t.tolist() == [0, 1] and obs.tolist() == [[0, 2], [5, 7]]
    t, obs = geometry.tracks_of_frames(tr, [4, 3])
    assert t.tolist() == [0, 2] and obs.tolist() == [[4, 3], [9, 8]]
    assert (tr["obs_frame"][obs] == [4, 3]).all()
    t, obs = geometry.tracks_of_frames(tr, [0, 4])
    assert t.tolist() == [0] and obs.tolist() == [[0, 4]]
    t, obs = geometry.tracks_of_frames(tr, [1, 3, 4])
    assert t.tolist() == [0] and obs.shape == (1, 3)
    t, obs = geometry.tracks_of_frames(model_of(cs["edge_mask_all_zero"]), [0, 1])
    assert t.size == 0 and obs.shape == (0, 2)
    with pytest.raises(ValueError):
        geometry.tracks_of_frames(tr, [1, 1])
    assert geometry.track_lengths(model_of(cs["edge_mask_all_zero"])).size == 0
