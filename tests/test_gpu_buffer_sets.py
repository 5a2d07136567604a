"""The buffer sets of the first-use features (rpe_bufset_fit: one device block per feature, carved afresh by every call)
keep nothing from call to call and survive their own growth: one handle calls every feature behind a stream -- refined
poses, guided matches, homographies, scale links, link poses, link bundles, tracks, track points, and (on inputs of their
own, they read no run) window bundles and pose graphs --, then makes the sets that grow grow (tracks over more frames; more
tracks, observations and frames to triangulate; more tracks, observations and windows to bundle; more frames, edges and
graphs to optimise), repeats the small calls inside the larger blocks, does the same with the pair proposals (small, larger
in every list, small again: the stage form ends the run, so it comes last behind the stream), and runs the other features
again behind another stream and behind a pair list.  Every result equals, bit for bit, what the same call returns on a
fresh handle that has called no other feature.
np.array_equal on the raw bits (floats viewed as unsigned integers); nothing here has a tolerance or an oracle.

Scenes: the interleaved frames of test_gpu_call_sequences.py (a0, b0, a1, b1, ...), as a stream of seven pairs and as the
list of every same-scene pair and its reverse, whose links join two pairs over the same two frames.  Every link of that
stream joins a pair inside a scene to a pair across two scenes: no scale link and no bundle of it is OK (codes TOO_FEW /
SKIPPED, measured; they are compared all the same), so the link calls also run behind the PHYSICS stream of
tests/scale_model.py, whose consecutive links test_gpu_link_pose.py and test_gpu_link_bundle.py establish as OK."""
import numpy as np
import pytest

from tests import pose_graph_cases as pgc
from tests import scale_model as sc
from tests import similarity_cases as smc
from tests import track_cases
from tests import track_point_cases as tpc
from tests import window_bundle_cases as wbc

pytestmark = pytest.mark.gpu

PAIRS = [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6)]
# (pair_a, pair_b, side): side bit 0 / 1 = the shared frame is image 2 of pair_a / of pair_b
LINKS = {"stream": ([0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 1, 1]),
         "physics": ([0, 1, 2, 3], [1, 2, 3, 4], [1, 1, 1, 1]),
         "list": ([0, 0, 2, 4, 6], [1, 1, 3, 5, 7], [1, 2, 1, 2, 1])}
N_PAIRS = {"stream": 7, "physics": 5, "list": 8}
LINK_FAMILIES = ("scale_links", "link_poses", "link_bundles")
RUN_FAMILIES = ("refine", "guided", "homography") + LINK_FAMILIES
# what runs behind each run, beside the tracks and the track points of the first
FAMILIES = {"stream": RUN_FAMILIES, "physics": LINK_FAMILIES, "list": RUN_FAMILIES}
BIG_TRACK_FRAMES = 40                     # against the 8 frames of the runs
BIG_POINTS = dict(n=4000, F=16)           # against at most 7 * 500 tracks over 8 frames
# Window bundles: one window of 3 frames over 60 tracks, then two windows of 4 over 1100 tracks of 6 frames.  Pose graphs: one
# graph of 2 frames and 1 edge, then one of 301 frames and 306 edges (every per-frame and per-edge piece grows) and three
# graphs in one call (every per-graph piece grows, and the pieces behind them move inside the grown block)
WINDOWS = {"windows": lambda: wbc.noisy(3), "big_windows": wbc.stream_like}
GRAPHS = {"graphs": pgc.two_frames, "big_graphs": pgc.big300, "many_graphs": pgc.three_graphs}
# Pair proposals over descriptors of their own (similarity_cases.random_frames; the handle's keypoint capacity is 1064):
# frames, query rows, target columns, candidates per row; times on both lists, so every piece of the set has bytes
SIMILAR = {"similar": dict(seed=11, counts=[33, 64, 40], nq=3, nt=2, k=1),
           "big_similar": dict(seed=12, counts=[257, 0, 64, 1064, 33, 500, 128, 65, 1, 300, 256, 40], nq=12, nt=10, k=3)}


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def scenes(K_vga):
    """per run: (frames, K)"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(4, K_vga, cfg=9)
    f = np.empty((8, 480, 640), np.uint8)
    f[0::2] = i1; f[1::2] = i2
    return {"stream": (f, K_vga), "list": (f, K_vga), "physics": sc.physics_frames()}


def _engine(capi):
    return capi.Engine(640, 480, max_batch=8, nfeatures=1000, max_matches=500)


def _run(e, kind, scenes):
    """the run of `kind` on handle e: its five results"""
    frames, K = scenes[kind]
    if kind != "list":
        return e.estimate_stream(frames, K)
    e.frames_reserve(8)
    e.frames_put(frames, np.arange(8))
    p = np.asarray(PAIRS)
    return e.estimate_pairs(p[:, 0], p[:, 1], K)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.itemsize]) if x.dtype.kind == "f" else x


def _arrays(r):
    """a call's result as a tuple of arrays (the track, window and graph calls return dicts; a list in one, an array per
    window or graph, counts as its arrays in order)"""
    if not isinstance(r, dict):
        return tuple(r)
    return tuple(np.asarray(x) for k in sorted(r) for x in (r[k] if isinstance(r[k], list) else [r[k]]))


def _same(a, b, what):
    a, b = _arrays(a), _arrays(b)
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, "field", k, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), (what, "field", k)


def big_tracks():
    """8 pairs that chain 9 of BIG_TRACK_FRAMES frames, 20 matches each: 20 tracks of 9 observations"""
    P, n = 8, 20
    f = [min(5 * k, BIG_TRACK_FRAMES - 1) for k in range(P + 1)]
    p1, p2 = track_cases.edge_points(P, n)
    return dict(frame1=f[:-1], frame2=f[1:], qidx=[list(range(n))] * P, tidx=[list(range(n))] * P, n_frames=BIG_TRACK_FRAMES,
                pts1=list(p1), pts2=list(p2))


def big_points():
    """BIG_POINTS['n'] two-view tracks over BIG_POINTS['F'] frames: track_point_cases.two_view_tracks on a longer walk"""
    n, F = BIG_POINTS["n"], BIG_POINTS["F"]
    rng = np.random.default_rng(77)
    R, T, c = tpc.walk(rng, F)
    X = tpc.points_in_front(rng, n, c)
    return tpc.build("big", R, T, tpc.cm.Cam(tpc.K0), X, [(i, [i % (F - 1), F - 1]) for i in range(n)], rng, 0.2)


def _triangulate(e, case):
    return e.triangulate_tracks(case["tracks"], case["R_abs"], case["T_abs"], K=case["cams"].K, **case["gates"])


def run_points_case(tracks, res, K):
    """the run's tracks under poses of its own: the even frame of every same-scene pair at the origin, the odd one at the
    pair's pose (pairs 0, 2, 4, 6 of either run), each scene a group"""
    R, t = res[0], res[1]
    R_abs = np.stack([np.eye(3) if f % 2 == 0 else R[f - 1] for f in range(8)])
    T_abs = np.stack([np.zeros(3) if f % 2 == 0 else t[f - 1].reshape(3) for f in range(8)])
    return dict(tracks=tracks, R_abs=R_abs, T_abs=T_abs, K=K, frame_group=np.arange(8, dtype=np.int32) // 2)


def _run_points(e, c):
    return e.triangulate_tracks(c["tracks"], c["R_abs"], c["T_abs"], K=c["K"], frame_group=c["frame_group"])


def _windows(e, case):
    return e.bundle_windows(case["tracks"], case["points0"], case["R_abs"], case["T_abs"], case["windows"], K=case["cams"].K,
                            obs_use=case["obs_use"], point_use=case["point_use"], max_points=case["max_points"],
                            min_obs=case["min_obs"], max_iters=case["max_iters"])


def _graphs(e, case):
    return e.optimise_graphs(**case)


def _similar(e, c):
    """the stage form: rows over the last nq frames, columns over the first nt, times that exclude neighbours"""
    F = len(c["counts"])
    q = np.arange(F - c["nq"], F, dtype=np.int32); t = np.arange(c["nt"], dtype=np.int32)
    return e.similarity_hamming(smc.random_frames(c["seed"], c["counts"]), None, q, t, step=2, max_distance=64,
                                q_time=10 * q, t_time=10 * t, exclude=5, min_score=1, k=c["k"])


def _family(e, kind, fam, bundle_start=None):
    P, links = N_PAIRS[kind], LINKS[kind]
    if fam == "refine":
        return e.refine_poses(P, 10)
    if fam == "guided":
        return e.guided_matches(P)
    if fam == "homography":
        return e.pair_homographies(P)
    if fam == "scale_links":
        return e.scale_links(*links)
    if fam == "link_poses":
        return e.link_poses(*links)
    if fam == "link_bundles":
        return e.link_bundles(*links, *bundle_start)
    assert fam == "build_tracks"
    return e.build_tracks()


@pytest.fixture(scope="module")
def ref(capi, scenes, K_vga):
    """every call of the sequence on a handle of its own, behind nothing but the run it needs"""
    out = {}

    def fresh(fn, kind=None):
        e = _engine(capi)
        try:
            if kind:
                out[kind, "run"] = _run(e, kind, scenes)
            return fn(e)
        finally:
            e.close()

    for kind in FAMILIES:
        for fam in FAMILIES[kind]:
            start = out[kind, "link_poses"][:2] if fam == "link_bundles" else None
            out[kind, fam] = fresh(lambda e: _family(e, kind, fam, start), kind)
    out["stream", "build_tracks"] = fresh(lambda e: _family(e, "stream", "build_tracks"), "stream")
    out["points_case"] = run_points_case(out["stream", "build_tracks"], out["stream", "run"], K_vga)
    out["stream", "track_points"] = fresh(lambda e: _run_points(e, out["points_case"]))
    out["big_tracks"] = fresh(lambda e: e.tracks_from_matches(**big_tracks()))
    out["big_points"] = fresh(lambda e: _triangulate(e, big_points()))
    for name, case in WINDOWS.items():
        out[name] = fresh(lambda e: _windows(e, case()))
    for name, case in GRAPHS.items():
        out[name] = fresh(lambda e: _graphs(e, case()))
    for name, c in SIMILAR.items():
        out[name] = fresh(lambda e: _similar(e, c))
    return out


@pytest.fixture(scope="module")
def seq(capi, scenes, ref):
    """the sequence on one handle: what every step returned"""
    got = {}
    e = _engine(capi)
    try:
        _run(e, "stream", scenes)
        for fam in RUN_FAMILIES + ("build_tracks",):
            got["stream", fam] = _family(e, "stream", fam, ref["stream", "link_poses"][:2])
        got["stream", "track_points"] = _run_points(e, ref["points_case"])
        got["windows"] = _windows(e, WINDOWS["windows"]())
        got["graphs"] = _graphs(e, GRAPHS["graphs"]())
        # the sets that grow, then the small calls carved inside the larger blocks
        got["big_tracks"] = e.tracks_from_matches(**big_tracks())
        got["big_points"] = _triangulate(e, big_points())
        got["big_windows"] = _windows(e, WINDOWS["big_windows"]())
        got["big_graphs"] = _graphs(e, GRAPHS["big_graphs"]())
        got["many_graphs"] = _graphs(e, GRAPHS["many_graphs"]())
        got["again", "build_tracks"] = _family(e, "stream", "build_tracks")
        got["again", "track_points"] = _run_points(e, ref["points_case"])
        got["again", "windows"] = _windows(e, WINDOWS["windows"]())
        got["again", "graphs"] = _graphs(e, GRAPHS["graphs"]())
        for fam in RUN_FAMILIES:
            got["again", fam] = _family(e, "stream", fam, ref["stream", "link_poses"][:2])
        # the pair proposals: the stage form overwrites the workspace's features and ends the run
        got["similar"] = _similar(e, SIMILAR["similar"])
        got["big_similar"] = _similar(e, SIMILAR["big_similar"])
        got["again", "similar"] = _similar(e, SIMILAR["similar"])
        for kind in ("physics", "list"):
            _run(e, kind, scenes)
            for fam in FAMILIES[kind]:
                got[kind, fam] = _family(e, kind, fam, ref[kind, "link_poses"][:2])
    finally:
        e.close()
    return got


def test_references_are_not_empty(capi, ref):
    for kind in FAMILIES:
        R, t, inl, nm, st = ref[kind, "run"]
        link, pose, bundle = ref[kind, "scale_links"][2], ref[kind, "link_poses"][4][:, 0], ref[kind, "link_bundles"][7][:, 0]
        print(kind, "status", st.tolist(), "n_matches", nm.tolist(), "inliers", inl.tolist(), "scale link codes", link.tolist(),
              "link pose codes", pose.tolist(), "bundle codes", bundle.tolist())
        assert not st.any() and (nm >= 100).all(), (kind, st, nm)
        if kind == "physics":
            assert (link == capi.LINK_OK).any() and (pose == capi.LINKPOSE_OK).any() and (bundle == capi.BUNDLE_OK).any(), (link, pose, bundle)
            continue
        print(kind, "guided", ref[kind, "guided"][5].tolist(), "homography codes", ref[kind, "homography"][4][:, 0].tolist(),
              "refine codes", ref[kind, "refine"][3][:, 0].tolist())
        assert (ref[kind, "guided"][5] > 0).any() and (ref[kind, "refine"][3][:, 0] == capi.REFINE_OK).any()
        assert (ref[kind, "homography"][4][:, 0] == capi.HOMOGRAPHY_OK).any()
    tracks, pts = ref["stream", "build_tracks"], ref["stream", "track_points"]
    print("tracks", tracks["n_tracks"], "observations", tracks["n_obs"], "point codes", np.bincount(pts["code"], minlength=6).tolist())
    assert tracks["n_tracks"] >= 1 and (pts["code"] == capi.TRACKPT_OK).any()
    big_t, big_p = ref["big_tracks"], ref["big_points"]
    assert big_t["n_tracks"] == 20 and big_t["n_obs"] == 180 and big_t["n_frames_seen"] == 9
    assert (big_p["code"] == capi.TRACKPT_OK).sum() >= BIG_POINTS["n"] // 2
    # the grown calls are larger than the run's in every count the sets are sized by
    assert len(big_p["code"]) > tracks["n_tracks"] and len(big_p["obs_flag"]) > tracks["n_obs"] and BIG_POINTS["F"] > 8
    # window bundles: tracks, observations, frames, windows, window frames, point slots; an OK window in either call
    w, big_w = WINDOWS["windows"](), WINDOWS["big_windows"]()
    for key in ("track_start", "obs_frame"):
        assert len(big_w["tracks"][key]) > len(w["tracks"][key]), key
    assert len(big_w["R_abs"]) > len(w["R_abs"]) and len(big_w["windows"]) > len(w["windows"])
    assert sum(map(len, big_w["windows"])) > sum(map(len, w["windows"]))
    assert len(big_w["windows"]) * big_w["max_points"] > len(w["windows"]) * w["max_points"]
    print("window codes", ref["windows"]["code"].tolist(), ref["big_windows"]["code"].tolist())
    assert (ref["windows"]["code"] == capi.WINDOW_OK).any() and (ref["big_windows"]["code"] == capi.WINDOW_OK).any()
    # pose graphs: big_graphs is larger in frames, graph positions, edges, free frames and used edges (so in the adjacency,
    # two entries per used edge with a free end), many_graphs in graphs; an OK graph in every call
    g, big_g, many_g = (ref[k] for k in GRAPHS)
    small_case, big_case = GRAPHS["graphs"](), GRAPHS["big_graphs"]()
    assert len(big_case["R_abs"]) > len(small_case["R_abs"]) and len(many_g["code"]) > len(g["code"])
    for key in ("frames", "free", "used_edges"):
        assert big_g[key].sum() > g[key].sum(), key
    assert sum(len(e["i"]) for e in big_case["edges"]) > sum(len(e["i"]) for e in small_case["edges"])
    print("graph codes", g["code"].tolist(), big_g["code"].tolist(), many_g["code"].tolist())
    assert all((r["code"] == capi.GRAPH_OK).any() for r in (g, big_g, many_g))
    # pair proposals: frames, rows, columns and candidates per row; both calls score and select something
    s, big_s = SIMILAR["similar"], SIMILAR["big_similar"]
    assert all(big_s[key] > s[key] for key in ("nq", "nt", "k")) and len(big_s["counts"]) > len(s["counts"])
    for name in SIMILAR:
        print(name, "scores", ref[name]["scores"].tolist(), "n_cand", ref[name]["n_cand"].tolist())
        assert ref[name]["scores"].any() and ref[name]["n_cand"].any(), name


STEPS = ([(("stream", fam), ("stream", fam)) for fam in RUN_FAMILIES + ("build_tracks", "track_points")]
         + [("big_tracks", "big_tracks"), ("big_points", "big_points")]
         + [(("again", fam), ("stream", fam)) for fam in ("build_tracks", "track_points") + RUN_FAMILIES]
         + [(name, name) for name in list(WINDOWS) + list(GRAPHS) + list(SIMILAR)]
         + [(("again", name), name) for name in ("windows", "graphs", "similar")]
         + [((kind, fam), (kind, fam)) for kind in ("physics", "list") for fam in FAMILIES[kind]])


def _id(step):
    return step if isinstance(step, str) else "-".join(step)


@pytest.mark.parametrize("step,name", STEPS, ids=[_id(s) for s, _ in STEPS])
def test_step_equals_fresh_handle(seq, ref, step, name):
    _same(seq[step], ref[name], f"{_id(step)} vs a fresh handle's {_id(name)}")
