"""The float64 model of the link bundles (tests/link_bundle_model.py) against itself and against plain linear algebra, no
GPU: its analytic Jacobians equal central differences, its Schur step equals the dense LM step, exact data does not
move, the noisy hand-built runs give the codes, counts and point sets they were built for and never a larger rms, the
forward / reversed ties of the chosen seeds stay under the cap, and the accuracy table of DESIGN section 8 with the bands
the GPU tests use."""
import numpy as np
import pytest

from tests import link_bundle_cases as bc
from tests import link_bundle_model as bm
from tests import link_pose_cases as lc
from tests import link_pose_model as lp

EPS = float(np.finfo(np.float64).eps)


def _params_applied(P, X, d, dp):
    poses, Xn = bm.apply_step(P, X, d, dp)
    Q = dict(P); Q.update(poses)
    return Q, Xn


# ------------------------------------------------------------------ 1. derivatives
@pytest.mark.parametrize("n,n_c", [(6, 6), (64, 40)])
def test_jacobians_equal_central_differences(n, n_c):
    """every column of (JC | JX) against (e(+h) - e(-h)) / 2h through the model's own update (rotation increment, tangent
    step with renormalisation, plain increments).  Central differences of step h carry a truncation error ~ h^2 |e'''| and
    a rounding error ~ eps |e| / h; with residuals of a few hundred pixels per unit parameter and h = 1e-6 both stay below
    1e-4 px per unit: the bound is relative, 1e-6 of the largest entry of the column."""
    P = bc.stage_problem(n, n_c)
    X = P["X0"]
    e, JX, JC = bm.rows(P, X)
    h = 1e-6
    worst = 0.0
    for k in range(bm.NCAM):
        d = np.zeros(bm.NCAM); d[k] = h
        Qp, _ = _params_applied(P, X, d, 0.0); Qm, _ = _params_applied(P, X, -d, 0.0)
        num = (bm.residuals_only(Qp, {}, X) - bm.residuals_only(Qm, {}, X)) / (2 * h)
        scale = max(np.abs(JC[:, :, k]).max(), 1.0)
        worst = max(worst, np.abs(num - JC[:, :, k]).max() / scale)
    for k in range(3):
        dp = np.zeros_like(X); dp[:, k] = h
        num = (bm.residuals_only(P, {}, X + dp) - bm.residuals_only(P, {}, X - dp)) / (2 * h)
        scale = max(np.abs(JX[:, :, k]).max(), 1.0)
        worst = max(worst, np.abs(num - JX[:, :, k]).max() / scale)
    print("n %d: worst relative difference analytic / central %.3e" % (n, worst))
    assert worst <= 1e-6
    assert not JC[~P["hc"], 4:6].any() and not JX[~P["hc"], 4:6].any() and not JC[:, 0:2].any()


# ------------------------------------------------------------------ 2. the Schur step
# measured worst (this file, both n, lambda 1e-3 and 10): camera step 1.1e-13 and point step 8.6e-13 relative to the
# step's largest entry, at condition numbers of the dense system up to 6.7e8.  float64 allows cond * eps ~ 1.5e-7 there (the
# dense solve's own error bound); the bounds are ten times the measured worst, for another libm or BLAS.
SCHUR_CAM_WORST, SCHUR_POINT_WORST = 1.1e-13, 8.6e-13


@pytest.mark.parametrize("n", [6, 64])
def test_schur_step_equals_dense_step(n):
    worst_c = worst_p = cond = 0.0
    for n_c in (n, max(6, n // 2)):
        P = bc.stage_problem(n, n_c)
        e, JX, JC = bm.rows(P, P["X0"])
        U, gc, _ = bm.normal_sums(e, JC, lp.SUMS["forward"])
        for lam in (1e-3, 10.0):
            d, dp = bm.schur_step(e, JX, JC, U, gc, lam, lp.SUMS["forward"])
            dd, ddp, c = bm.dense_step(e, JX, JC, lam)
            worst_c = max(worst_c, np.abs(d - dd).max() / np.abs(dd).max())
            worst_p = max(worst_p, np.abs(dp - ddp).max() / np.abs(ddp).max())
            cond = max(cond, c)
    print("n %d: Schur against dense: camera step %.3e, point step %.3e (relative), condition number %.3e, cond * eps %.3e" %
          (n, worst_c, worst_p, cond, cond * EPS))
    assert worst_c <= 10 * SCHUR_CAM_WORST and worst_p <= 10 * SCHUR_POINT_WORST
    assert 10 * max(SCHUR_CAM_WORST, SCHUR_POINT_WORST) <= cond * EPS        # the bound asks more than float64 promises the dense solve


# ------------------------------------------------------------------ 3. exact data
@pytest.mark.parametrize("n", [6, 257])
def test_exact_data_does_not_move(n):
    """no noise, no outliers, the true state as the start: rms is zero to rounding (observations are quotients rounded
    once: residuals of a few eps * f pixels) and the state stays within that of the truth"""
    P = bc.stage_problem(n, n, noise=0.0)
    r = bm.bundle(P, max_iters=10)
    print("exact n %d: code %d rms %s" % (n, r["code"], r["rms"]))
    tol = 64 * EPS * P["fa"]
    assert r["rms"][0] <= tol and r["rms"][1] <= r["rms"][0]
    assert np.abs(r["RA"] - P["RA"]).max() <= 1e-12 and np.abs(r["RC"] - P["RC"]).max() <= 1e-12
    assert np.abs(r["tA"] - P["tA"]).max() <= 1e-12 and np.abs(r["tC"] - P["tC"]).max() <= 1e-11 and np.abs(r["X"] - P["X0"]).max() <= 1e-9


# ------------------------------------------------------------------ 4. noisy hand runs, ties, accuracy
@pytest.fixture(scope="module")
def hand_results(oracle, K_vga):
    """every count from 6 up x every side: the link pose model's minimal and polished pose, then the bundle fed with the
    polished one, forward and reversed"""
    out = []
    for n in bc.COUNTS:
        for side in range(4):
            run, p1, p2, truth_a, truth_b, n_exp, outl = bc.hand_run(n, side, K_vga)
            x1, x2, f = lp.observations(p1, p2, K_vga)
            kw = dict(iters=lc.ITERS, threshold_px=lc.GATE_PX, min_shared=6)
            lp0 = lp.link_pose(run, x1, x2, f, (0, 1, side), oracle.ransac_subsets, refine_iters=0, **kw)
            lp1 = lp.link_pose(run, x1, x2, f, (0, 1, side), oracle.ransac_subsets, refine_iters=10, **kw)
            args = (run, x1, x2, f, (0, 1, side), lp1["R"], lp1["t"])
            fwd = bm.link_bundle(*args, threshold_px=lc.GATE_PX, min_shared=6)
            rev = bm.link_bundle(*args, threshold_px=lc.GATE_PX, min_shared=6, order="reversed")
            out.append(dict(n=n, side=side, run=run, truth_a=truth_a, truth_b=truth_b, n_exp=n_exp, outl=outl, lp0=lp0, lp1=lp1, fwd=fwd, rev=rev))
    return out


def test_noisy_hand_runs(hand_results):
    codes = {}
    for h in hand_results:
        f = h["fwd"]
        codes[f["code"]] = codes.get(f["code"], 0) + 1
        assert h["lp1"]["code"] == lp.LINKPOSE_OK
        assert f["counts"][0] == h["n_exp"] and f["counts"][1] <= h["n_exp"]
        if f["counts"][1] < 6:                                # 6 and 7 points less their outliers on C
            assert f["code"] == bm.BUNDLE_TOO_FEW and h["n"] < 10 and not f["views"].any() and not f["points"].any() and f["rms"] == (0.0, 0.0)
            continue
        assert f["code"] in (bm.BUNDLE_OK, bm.BUNDLE_REJECTED), (h["n"], h["side"], f["code"])
        assert f["counts"][0] == int((f["views"] != 0).sum()) and f["counts"][1] == int((f["views"] == 3).sum())
        # the gross outliers on C are not observations, most of the others are
        assert f["counts"][1] <= h["n_exp"] - int(round(bc.OUTLIER_FRAC * h["n"])) + 2
        assert f["rms"][1] <= f["rms"][0], (h["n"], h["side"], f["rms"])
        if f["code"] == bm.BUNDLE_OK:
            assert abs(np.linalg.norm(f["t_a"]) - 1.0) <= 1e-12
    print("hand runs: codes", codes)
    assert codes.get(bm.BUNDLE_TOO_FEW, 0) == 8 and codes.get(bm.BUNDLE_OK, 0) * 4 >= 3 * (len(hand_results) - 8)


def test_duplicates_and_unusable(K_vga, oracle):
    for side in range(4):
        base = bc.hand_run(64, side, K_vga)
        x1, x2, f = lp.observations(base[1], base[2], K_vga)
        pose = lp.link_pose(base[0], x1, x2, f, (0, 1, side), oracle.ransac_subsets, iters=lc.ITERS, threshold_px=lc.GATE_PX, min_shared=6)
        ref = bm.link_bundle(base[0], x1, x2, f, (0, 1, side), pose["R"], pose["t"], min_shared=6)
        dup = bc.hand_run(64, side, K_vga, dup_a=5, dup_b=7)
        y1, y2, g = lp.observations(dup[1], dup[2], K_vga)
        got = bm.link_bundle(dup[0], y1, y2, g, (0, 1, side), pose["R"], pose["t"], min_shared=6)
        assert got["counts"] == ref["counts"] and got["info"] == ref["info"]
        assert np.array_equal(got["views"][:64], ref["views"]) and not got["views"][64:].any() and not got["points"][64:].any()
        assert np.array_equal(got["points"][:64], ref["points"]) and np.array_equal(got["R_b"], ref["R_b"])
        un = bc.hand_run(64, side, K_vga, a_unusable=9)
        z1, z2, k = lp.observations(un[1], un[2], K_vga)
        got = bm.link_bundle(un[0], z1, z2, k, (0, 1, side), pose["R"], pose["t"], min_shared=6)
        assert got["counts"][0] == 55 and not got["views"][55:].any() and (got["views"][:55] != 0).all()
        # codes as constructed
        assert bm.link_bundle(un[0], z1, z2, k, (0, 1, side), np.zeros((3, 3)), np.zeros(3))["info"] == (bm.BUNDLE_SKIPPED, 0, 0, 0)
        assert bm.link_bundle(un[0], z1, z2, k, (0, 1, side), np.zeros((3, 3)), np.zeros(3))["counts"] == (55, 0)
        assert bm.link_bundle(un[0], z1, z2, k, (0, 1, side), pose["R"], pose["t"], min_shared=65)["code"] == bm.BUNDLE_TOO_FEW
        un[0].status[0] = 3
        assert bm.link_bundle(un[0], z1, z2, k, (0, 1, side), pose["R"], pose["t"])["code"] == bm.BUNDLE_PAIR_FAILED


def test_tie_cap(hand_results):
    """the forward and the reversed model may disagree on an accept / reject decision; at most one scene in 16 may"""
    ties, d = bm.reduction_margin([h["fwd"] for h in hand_results], [h["rev"] for h in hand_results])
    print("ties %s of %d scenes; forward / reversed differences: rms %.3e px, R %.3e deg, t %.3e, point %.3e, rms_before %.3e px" %
          (ties, len(hand_results), *d))
    assert len(ties) * 16 <= len(hand_results) and (d > 0).all()


def test_accuracy_table(hand_results):
    """rotation error of pose a and of pose b (degrees) and | |t_b| - 1.5 | against hand_run's truth for the input state
    (pair a's own pose, the minimal link pose), the link-pose-polished state and the bundled state: the figures of DESIGN
    section 8, and the bands of link_bundle_model (twice the bundled worst)"""
    rows = {"input": [], "polished": [], "bundled": []}
    for h in hand_results:
        if h["fwd"]["code"] == bm.BUNDLE_TOO_FEW:
            continue
        Ra_t, Rb_t = h["truth_a"][0], h["truth_b"][0]
        a_in = lp.rot_angle_deg(h["run"].R[0], Ra_t)
        for name, Ra, Rb, tb in (("input", None, h["lp0"]["R"], h["lp0"]["t"]), ("polished", None, h["lp1"]["R"], h["lp1"]["t"]),
                                 ("bundled", h["fwd"]["R_a"], h["fwd"]["R_b"], h["fwd"]["t_b"])):
            rows[name].append((a_in if Ra is None else lp.rot_angle_deg(Ra, Ra_t), lp.rot_angle_deg(Rb, Rb_t),
                               abs(np.linalg.norm(tb) - lc.BASE_C / lc.BASE_A)))
    print("state      rot a deg (median, worst)   rot b deg (median, worst)   ||t_b| - 1.5| (median, worst)")
    for name, v in rows.items():
        v = np.array(v)
        print("%-9s  %.4f  %.4f              %.4f  %.4f              %.4f  %.4f" %
              (name, np.median(v[:, 0]), v[:, 0].max(), np.median(v[:, 1]), v[:, 1].max(), np.median(v[:, 2]), v[:, 2].max()))
    w = np.array(rows["bundled"]).max(0)
    assert np.allclose(w, [bm.BUNDLE_ROT_A_WORST_DEG, bm.BUNDLE_ROT_B_WORST_DEG, bm.BUNDLE_SCALE_WORST], rtol=0.02), w
