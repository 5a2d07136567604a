"""Link poses (rpe_link_poses / PoseEstimator.last_link_poses): the float64 model (tests/link_pose_model.py) checked on
the CPU -- the minimal solver on exact triples, the rule on hand-built runs, and the physics bands fixed from the CPU
oracle (the tables are printed; run with -s)."""
import numpy as np
import pytest

from tests import link_pose_cases as lc
from tests import link_pose_model as lp
from tests import scale_model as sc


def test_link_pose_surface_exists():
    """the entry point is exported and declared, and the Python surface binds it"""
    import inspect
    from relative_pose_estimation_amd import _capi, PoseEstimator, geometry, synthetic
    lib = _capi.load()
    assert "rpe_link_poses" in _capi.EXPORTS and hasattr(lib, "rpe_link_poses")
    assert (_capi.LINKPOSE_OK, _capi.LINKPOSE_PAIR_FAILED, _capi.LINKPOSE_TOO_FEW, _capi.LINKPOSE_NONE) == (0, 1, 2, 3) == \
        (lp.LINKPOSE_OK, lp.LINKPOSE_PAIR_FAILED, lp.LINKPOSE_TOO_FEW, lp.LINKPOSE_NONE)
    p = inspect.signature(_capi.Engine.link_poses).parameters
    assert (p["iters"].default, p["threshold_px"].default, p["min_shared"].default, p["refine_iters"].default) == (256, None, 8, 10)
    assert callable(getattr(PoseEstimator, "last_link_poses", None))
    assert inspect.signature(PoseEstimator.estimate_trajectory).parameters["register"].default is False
    assert callable(getattr(synthetic, "make_views", None)) and callable(getattr(geometry, "registered_chain_inputs", None))


def test_make_views_is_make_stream_on_its_poses(K_vga):
    from relative_pose_estimation_amd import synthetic
    Rs, ts = synthetic.stream_poses(3, seed=77, step=0.2)
    want = synthetic.make_stream(3, K_vga, 160, 120, seed=77, step=0.2)[0]
    assert np.array_equal(synthetic.make_views(Rs, ts, K_vga, 160, 120, seed=77), want)
    with pytest.raises(ValueError):
        synthetic.make_views(Rs, ts[:2], K_vga)


# ------------------------------------------------------------------ 1. the solver on exact triples
def test_root_finder_against_np_roots():
    rng = np.random.default_rng(5)
    for _ in range(200):
        r = np.sort(rng.uniform(-3, 3, 4))
        if np.diff(r).min() < 0.05:
            continue
        c = np.poly(r)[::-1] * rng.uniform(0.5, 2.0)
        got = lp.real_roots(c)
        assert len(got) == 4 and np.allclose(got, r, rtol=0, atol=1e-9), (r, got)
    assert lp.real_roots([1.0, 0.0, 1.0, 0.0, 0.0]) == []                     # x^2 + 1, trimmed from degree 4
    assert lp.real_roots([-2.0, 1.0, 0.0, 0.0, 0.0]) == [2.0]                  # trimmed to degree 1
    assert lp.real_roots([3.0, 0.0, 0.0, 0.0, 0.0]) == [] and lp.real_roots([0.0] * 5) == []


def test_solver_on_exact_triples():
    """every candidate reproduces its three bearings and the three side lengths, the true pose is among the candidates
    within TRIPLE_BOUND = 10 x the worst deviation of this very set (written beside the seeds)"""
    seeds = lc.triple_seeds()
    worst = worst_b = worst_s = 0.0
    for s in seeds:
        P, q, R, t = lc.exact_triple(s)
        cands = lp.p3p(P, q)
        assert 1 <= len(cands) <= 4, s
        assert [c[0] for c in cands] == sorted(c[0] for c in cands)
        for _, Rc, tc in cands:
            Y = P @ Rc.T + tc
            assert (Y[:, 2] > 0).all(), s
            worst_b = max(worst_b, float(np.abs(Y[:, :2] / Y[:, 2:3] - q).max()))
            for i, k in ((0, 1), (0, 2), (1, 2)):
                worst_s = max(worst_s, abs(np.linalg.norm(Y[i] - Y[k]) / np.linalg.norm(P[i] - P[k]) - 1.0))
            assert np.allclose(Rc @ Rc.T, np.eye(3), atol=1e-12) and np.linalg.det(Rc) > 0
        worst = max(worst, min(max(np.abs(Rc - R).max(), np.abs(tc - t).max()) for _, Rc, tc in cands))
    print("exact triples: %d seeds (last %d), worst pose deviation %.3e, bearings %.3e, side lengths %.3e" %
          (len(seeds), seeds[-1], worst, worst_b, worst_s))
    assert worst <= lc.TRIPLE_BOUND
    # the candidate is a rigid map, so the side lengths hold to round-off; how well it reproduces the bearings is the
    # accuracy of its root, like the pose deviation, and shares its bound
    assert worst_s <= 1e-12 and worst_b <= lc.TRIPLE_BOUND


@pytest.mark.parametrize("name", ["collinear", "repeated", "behind", "zero"])
def test_degenerate_triples_give_no_candidate(name):
    P, q, R, t = lc.exact_triple(0)
    if name == "collinear":
        P = np.array([P[0], P[0] + (P[1] - P[0]) * 0.5, P[1]])
        Y = P @ R.T + t; q = Y[:, :2] / Y[:, 2:3]
    elif name == "repeated":
        P = np.array([P[0], P[0], P[2]]); q = np.array([q[0], q[0], q[2]])
    elif name == "behind":
        # the true pose has the three points BEHIND the camera: (x / z, y / z) then names the opposite rays.  Three points
        # are congruent to their mirror image through the centre by a proper rotation, so candidates may exist -- but
        # only with positive depths: none is the true pose, every one has the triple in front
        t = t - np.array([0.0, 0.0, 40.0])
        Y = P @ R.T + t
        assert (Y[:, 2] < 0).all()
        q = Y[:, :2] / Y[:, 2:3]
        for _, Rc, tc in lp.p3p(P, q):
            assert ((P @ Rc.T + tc)[:, 2] > 0).all() and np.abs(tc - t).max() > 1.0
        return
    else:
        P = np.zeros((3, 3)); q = np.zeros((3, 2))
    assert lp.p3p(P, q) == []


# ------------------------------------------------------------------ 2. hand-built runs
def _model(run, p1, p2, K, side, oracle, **kw):
    x1, x2, f = lp.observations(p1, p2, K)
    args = dict(iters=lc.ITERS, threshold_px=lc.GATE_PX, min_shared=6)
    args.update(kw)
    return lp.link_pose(run, x1, x2, f, (0, 1, side), oracle.ransac_subsets, **args)


def _gate_bounds(K):
    """what a pose may be off by when >= half the correspondences reproject within the gate: three gate angles in
    rotation (gate / f radians each), and three gate widths at the mean scene depth (9 scene units = 9 / BASE_A on pair
    a's scale) in translation"""
    f = (K[0, 0] + K[1, 1]) / 2
    return np.degrees(3 * lc.GATE_PX / f), 3 * lc.GATE_PX / f * 9.0 / lc.BASE_A


@pytest.mark.parametrize("n", lc.COUNTS)
def test_hand_built_counts_and_sides(n, K_vga, oracle):
    """every count around the round, wave and list edges, all four sides: one geometry, one pose"""
    rot_bound, t_bound = _gate_bounds(K_vga)
    solved = []
    for side in range(4):
        run, p1, p2, truth, n_exp, out = lc.hand_run(n, side, K_vga)
        r = _model(run, p1, p2, K_vga, side, oracle)
        assert r["n"] == n_exp == n and r["counts"][0] == n
        if n < 6:
            assert r["code"] == lp.LINKPOSE_TOO_FEW and not r["R"].any() and not r["t"].any() and not r["mask"].any()
            assert r["counts"] == (n, 0) and r["info"] == (lp.LINKPOSE_TOO_FEW, 0, 0, 0) and r["rms"] == (0.0, 0.0)
            continue
        assert r["code"] == lp.LINKPOSE_OK, (n, side, r["code"])
        assert r["counts"][1] == int(r["mask"].sum()) and r["rms"][1] <= r["rms"][0]
        assert not (r["mask"] & out).sum() > 0.1 * n, "gross outliers inside the gate"
        R, t = r["R"], r["t"]
        if side & 2:
            R, t = R.T, -(R.T @ t)
            truth = (truth[0].T, -(truth[0].T @ truth[1]))
        solved.append((R, t))
        if n >= 64:
            assert r["counts"][1] >= 0.6 * n, (n, side, r["counts"])
            assert lp.rot_angle_deg(R, truth[0]) <= rot_bound and np.abs(t - truth[1]).max() <= t_bound, (n, side)
    for R, t in solved[1:]:                       # the map of side bit 0 is R X + t of the other: equal up to its rounding
        assert np.allclose(R, solved[0][0], atol=1e-9) and np.allclose(t, solved[0][1], atol=1e-8)


def test_hand_built_rules(K_vga, oracle):
    n = 64
    base = _model(*lc.hand_run(n, 0, K_vga)[:3], K_vga, 0, oracle)
    # pair b's status plays no part; pair a's does
    for st in (1, 2, 3, 4):
        run, p1, p2 = lc.hand_run(n, 0, K_vga, b_status=st)[:3]
        r = _model(run, p1, p2, K_vga, 0, oracle)
        assert np.array_equal(r["R"], base["R"]) and np.array_equal(r["t"], base["t"]) and r["info"] == base["info"]
    run, p1, p2 = lc.hand_run(n, 0, K_vga)[:3]
    run.status[0] = 3
    r = _model(run, p1, p2, K_vga, 0, oracle)
    assert r["code"] == lp.LINKPOSE_PAIR_FAILED and r["counts"] == (0, 0) and not r["R"].any() and not r["mask"].any()
    # duplicate keys on either side lose to the lower match index: the same correspondences, the same bits
    for side in range(4):
        plain = _model(*lc.hand_run(n, side, K_vga)[:3], K_vga, side, oracle)
        for kw in (dict(dup_a=5), dict(dup_b=5), dict(dup_a=3, dup_b=7)):
            run, p1, p2 = lc.hand_run(n, side, K_vga, **kw)[:3]
            r = _model(run, p1, p2, K_vga, side, oracle)
            assert r["n"] == n and np.array_equal(r["R"], plain["R"]) and np.array_equal(r["t"], plain["t"]), (side, kw)
            assert np.array_equal(r["mask"][:n], plain["mask"][:n]) and not r["mask"][n:].any()
    # unusable matches of pair a leave the set; min_shared on both sides of n
    run, p1, p2, _, n_exp, _ = lc.hand_run(n, 1, K_vga, a_unusable=9)
    assert n_exp == n - 9
    for ms, code in ((n_exp - 1, lp.LINKPOSE_OK), (n_exp, lp.LINKPOSE_OK), (n_exp + 1, lp.LINKPOSE_TOO_FEW)):
        r = _model(run, p1, p2, K_vga, 1, oracle, min_shared=ms)
        assert r["n"] == n_exp and r["code"] == code, (ms, r["code"])
    r = _model(run, p1, p2, K_vga, 1, oracle, min_shared=1)                  # the floor of 6 is the subset stream's
    assert r["code"] == lp.LINKPOSE_OK
    run7, q1, q2 = lc.hand_run(7, 0, K_vga, a_unusable=2)[:3]
    assert _model(run7, q1, q2, K_vga, 0, oracle, min_shared=1)["code"] == lp.LINKPOSE_TOO_FEW


def test_hand_built_polish(K_vga, oracle):
    """the polish never raises the rms, refine_iters = 0 is the minimal pose, a polish that moved nothing or was rejected
    returns it too (a rejection that does occur is pinned in test_physics_with_the_oracle), and the analytic Jacobian is
    the derivative of the residuals"""
    run, p1, p2, truth, _, _ = lc.hand_run(256, 0, K_vga)
    r0 = _model(run, p1, p2, K_vga, 0, oracle, refine_iters=0)
    r10 = _model(run, p1, p2, K_vga, 0, oracle, refine_iters=10)
    assert r0["info"][3] == 0 and r0["rms"][0] == r0["rms"][1] and r0["info"][:3] == r10["info"][:3]
    assert r10["info"][3] > 0 and r10["rms"][0] == r0["rms"][0] and r10["rms"][1] < r10["rms"][0]
    assert lp.rot_angle_deg(r10["R"], truth[0]) < lp.rot_angle_deg(r0["R"], truth[0])
    # rejected: a gate so tight that the polished pose, which spreads the error, keeps fewer inliers than the minimal
    # pose, which is exact on its own three points
    seen = set()
    for gate in (0.05, 0.1, 0.2, 0.3):
        a = _model(run, p1, p2, K_vga, 0, oracle, refine_iters=0, threshold_px=gate)
        b = _model(run, p1, p2, K_vga, 0, oracle, refine_iters=10, threshold_px=gate)
        seen.add(b["info"][3] < 0)
        if b["info"][3] <= 0:
            assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["mask"], b["mask"])
            assert b["rms"][0] == b["rms"][1] and a["counts"] == b["counts"]
        else:
            assert b["counts"][1] >= a["counts"][1]
    print("polish rejected at some gate:", True in seen)
    # Jacobian
    rng = np.random.default_rng(3)
    X = np.column_stack([rng.uniform(-3, 3, 20), rng.uniform(-2, 2, 20), rng.uniform(4, 14, 20)])
    R = lp.rodrigues([0.02, -0.03, 0.01]); t = np.array([0.1, -0.2, 0.3]); q = rng.uniform(-0.3, 0.3, (20, 2))
    r, J = lp.residuals(R, t, X, q, 500.0, True)
    for k in range(6):
        d = np.zeros(6); d[k] = 1e-6
        num = (lp.residuals(lp.rodrigues(d[:3]) @ R, t + d[3:], X, q, 500.0) - lp.residuals(lp.rodrigues(-d[:3]) @ R, t - d[3:], X, q, 500.0)) / 2e-6
        assert np.allclose(J[:, :, k], num, rtol=1e-5, atol=1e-5), k


# ------------------------------------------------------------------ 3. physics with the oracle
@pytest.fixture(scope="module")
def physics_run(oracle):
    frames, K = sc.physics_frames()
    pairs, links = sc.physics_pairs_and_links()
    run, p1, p2 = lc.oracle_run_with_points(oracle, frames, pairs, K)
    return run, p1, p2, K, pairs, links


def test_physics_with_the_oracle(physics_run, oracle):
    """the table behind LINK_POSE_ROT_BAND_DEG and LINK_POSE_SCALE_BAND (link_pose_model.py): per link the rotation error
    and | |t| - true baseline ratio | of the model on the oracle's run, the scale link's median beside it"""
    from relative_pose_estimation_amd import synthetic
    run, p1, p2, K, pairs, links = physics_run
    x1, x2, f = lp.observations(p1, p2, K)
    P = sc.PHYSICS
    Rs, ts = synthetic.stream_poses(P["n_frames"], seed=P["seed"], max_angle_deg=P["max_angle_deg"], step=P["step"])
    Rt, tt = lc.truth_link_poses(Rs, ts, pairs, links)
    truth = sc.physics_truth(pairs, links)
    assert np.allclose(np.linalg.norm(tt, axis=1), truth, rtol=1e-12)
    med = sc.scale_links(run, links, sc.PHYSICS_MIN_SHARED)[0][:, 1]
    res = lp.link_poses(run, x1, x2, f, links, oracle.ransac_subsets, iters=lc.ITERS, threshold_px=lc.GATE_PX,
                        min_shared=sc.PHYSICS_MIN_SHARED)
    print("link (a, b, side)  n    inliers  rot err deg  |t|     truth   deviation  scale-link median")
    worst_rot = worst_dev = 0.0
    for l, r in zip(links, res):
        assert r["code"] == lp.LINKPOSE_OK, l
        k = links.index(l)
        rot = lp.rot_angle_deg(r["R"], Rt[k]); nt = float(np.linalg.norm(r["t"])); dev = abs(nt - truth[k])
        print("%-18s %-4d %-8d %-12.4f %-7.4f %-7.4f %-10.4f %.4f" % (tuple(l), r["counts"][0], r["counts"][1], rot, nt, truth[k], dev, med[k]))
        worst_rot = max(worst_rot, rot); worst_dev = max(worst_dev, dev)
    print("largest: rot %.4f deg, deviation %.4f" % (worst_rot, worst_dev))
    # a polish that lost inliers is rejected: the minimal pose comes back, bit for bit (link (3, 8, 0) of the table)
    rejected = [k for k, r in enumerate(res) if r["info"][3] < 0]
    assert rejected, "no rejected polish on this stream any more: find another case for the rule"
    for k in rejected:
        m = lp.link_pose(run, x1, x2, f, links[k], oracle.ransac_subsets, iters=lc.ITERS, threshold_px=lc.GATE_PX,
                         min_shared=sc.PHYSICS_MIN_SHARED, refine_iters=0)
        r = res[k]
        assert np.array_equal(r["R"], m["R"]) and np.array_equal(r["t"], m["t"]) and np.array_equal(r["mask"], m["mask"])
        assert r["counts"] == m["counts"] and r["rms"] == m["rms"] and r["rms"][0] == r["rms"][1]
    assert np.isclose(lp.LINK_POSE_ROT_BAND_DEG, 2 * worst_rot, rtol=0.01)
    assert np.isclose(lp.LINK_POSE_SCALE_BAND, 2 * worst_dev, rtol=0.01)


# ------------------------------------------------------------------ 4. rotation-only bridge
def test_rotation_only_bridge(oracle):
    """C = S rotated about its own centre: the five-point pose of (S, C) against the truth, and the link pose of (S, C)
    on the structure of (S, A): the right rotation with |t| ~ 0, inside the band of test 3"""
    frames, K, Rs, ts = lc.rotation_only_frames()
    pairs, link = [(0, 1), (0, 2)], (0, 1, 0)
    run, p1, p2 = lc.oracle_run_with_points(oracle, frames, pairs, K)
    x1, x2, f = lp.observations(p1, p2, K)
    Rt, tt = lc.truth_link_poses(Rs, ts, pairs, [link])
    assert np.allclose(tt[0], 0, atol=1e-12)
    r = lp.link_pose(run, x1, x2, f, link, oracle.ransac_subsets, iters=lc.ITERS, threshold_px=lc.GATE_PX)
    own = lp.rot_angle_deg(run.R[1], Rt[0]) if run.status[1] == 0 else float("nan")
    rot = lp.rot_angle_deg(r["R"], Rt[0]); nt = float(np.linalg.norm(r["t"]))
    print("rotation-only (S, C): status %d, matches %d, five-point inliers %d -> pose inliers %d, rotation error %.4f deg" %
          (run.status[1], run.n_matches[1], run.ransac_mask[1].sum(), run.pose_mask[1].sum(), own))
    print("link pose: n %d, inliers %d, rotation error %.4f deg, |t| %.4f (truth 0)" % (r["counts"][0], r["counts"][1], rot, nt))
    assert r["code"] == lp.LINKPOSE_OK
    assert rot <= lp.LINK_POSE_ROT_BAND_DEG and nt <= lp.LINK_POSE_SCALE_BAND
