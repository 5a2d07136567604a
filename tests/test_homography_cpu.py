"""Homography RANSAC and rotation-only detection, the parts that need no GPU: the float64 model of the rule in
include/rpe_amd.h (tests/homography_model.py) on synthetic scenes with known inliers, the model's own properties,
geometry.classify_pair on the rendered rotation-only and general pairs through the CPU oracle's pipeline, and the new
names in the header and in _capi.EXPORTS."""
import os
import re

import numpy as np
import pytest

from tests import guided_model as gm
from tests import homography_cases as hc
from tests import homography_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def thr2_px(K, px=hc.GATE_PX):
    return gm.thr2_of(px, gm.focal_K(K))


# ------------------------------------------------------------------ synthetic scenes
@pytest.mark.parametrize("M", hc.SIZES)
@pytest.mark.parametrize("scene", ["plane", "rotation", "general"])
def test_scene(oracle, K_vga, scene, M):
    """0.3 px noise, 25 % outliers, 1 px gate, 256 samples.  Measured with the seeds of homography_cases.SCENE_SEEDS
    (n_H / true correspondences): plane 4/4, 5/5, 45/48, 212/225; rotation 4/4, 5/5, 48/48, 220/225 with n_rot 4, 5, 48,
    224 and R_rot 0.024 deg from the truth at worst (M = 64); general 4, 4, 5, 10 of M = 6, 7, 64, 300."""
    p1, p2, true, R = hc.scene_points(scene, M, K_vga, hc.SCENE_SEEDS[(scene, M)])
    r, a, b = hc.model_on_pixels(p1, p2, K_vga, oracle.ransac_subsets(M, hc.ITERS))
    n_true = int(true.sum())
    assert r["code"] == hm.HOMOGRAPHY_OK and r["n_H"] == int(r["mask"].sum())
    if scene in ("plane", "rotation"):
        assert r["n_H"] >= 0.9 * n_true, (r["n_H"], n_true)
    elif M >= 64:
        assert r["n_H"] <= 0.25 * M, (r["n_H"], M)
    if scene == "rotation":
        assert r["n_rot"] >= 0.9 * n_true, (r["n_rot"], n_true)
        assert hm.rotation_angle_deg(r["R_rot"], R) <= 0.05
        assert np.allclose(r["R_rot"].T @ r["R_rot"], np.eye(3), atol=1e-12) and abs(np.linalg.det(r["R_rot"]) - 1) < 1e-12
        assert r["n_rot"] == hm.rotation_count(r["R_rot"], a, b, thr2_px(K_vga))[0]


def test_homography_is_unit_norm_in_the_gauge_and_maps_the_plane(oracle, K_vga):
    p1, p2, true, R = hc.scene_points("plane", 300, K_vga, 1)
    r, a, b = hc.model_on_pixels(p1, p2, K_vga, oracle.ransac_subsets(300, hc.ITERS))
    H = r["H"]
    assert abs(np.sqrt((H * H).sum()) - 1) < 1e-15
    ha = np.concatenate([a, np.ones((300, 1))], 1) @ H.T
    assert (ha[r["mask"], 2] > 0).all()
    err = np.linalg.norm(ha[:, :2] / ha[:, 2:3] - b, axis=1) * gm.focal_K(K_vga)
    assert (err[r["mask"]] <= 1.0 + 1e-9).all() and np.median(err[true]) < 0.6
    # pixel form: K2 H K1^-1 maps pixels as H maps normalised points
    from relative_pose_estimation_amd import geometry
    Hp = geometry.pixel_homography(H, K_vga, K_vga)
    q = np.concatenate([p1.astype(np.float64), np.ones((300, 1))], 1) @ Hp.T
    assert np.allclose((q[:, :2] / q[:, 2:3])[r["mask"]], (ha[:, :2] / ha[:, 2:3] * [K_vga[0, 0], K_vga[1, 1]] + [K_vga[0, 2], K_vga[1, 2]])[r["mask"]], atol=1e-6)


# ------------------------------------------------------------------ model properties
def test_the_winners_sample_is_in_its_mask(oracle, K_vga):
    for scene in ("plane", "rotation", "general"):
        for M in (7, 64, 300):
            sub = oracle.ransac_subsets(M, hc.ITERS)
            p1, p2, _, _ = hc.scene_points(scene, M, K_vga, 1)
            r, _, _ = hc.model_on_pixels(p1, p2, K_vga, sub)
            assert r["mask"][sub[r["it"], :4]].all(), (scene, M)


def test_duplicated_points_are_invalid_models_and_counted_out(oracle, K_vga):
    M = 64
    sub = oracle.ransac_subsets(M, hc.ITERS)
    p1, p2, _, _ = hc.scene_points("plane", M, K_vga, 1)
    p1 = p1.copy(); p2 = p2.copy()
    p1[1] = p1[0]; p2[1] = p2[0]; p1[3] = p1[2]                 # match 1 repeats match 0; image 1 of match 3 repeats match 2
    r, a, b = hc.model_on_pixels(p1, p2, K_vga, sub)
    s4 = sub[:, :4]
    degenerate = np.array([({0, 1} <= set(s)) or ({2, 3} <= set(s)) for s in s4.tolist()])
    assert degenerate.any() and not degenerate.all()
    H, G, valid = hm.four_point(a[s4], b[s4])
    assert not valid[degenerate].any()
    assert r["n_valid"] == int(valid.sum()) <= hc.ITERS - int(degenerate.sum())
    assert r["code"] == hm.HOMOGRAPHY_OK and not degenerate[r["it"]]


def test_collinear_input_gives_none(oracle, K_vga):
    M = 40
    x = np.arange(-20, 20) / 64.0                                 # dyadic coordinates: every product below is exact,
    a = np.stack([x, 0.5 * x + 0.125], 1)                         # so every lambda and mu is exactly 0
    b = np.stack([x, 0.25 * x - 0.0625], 1)
    r = hm.find_homography(a, b, oracle.ransac_subsets(M, hc.ITERS), thr2_px(K_vga))
    assert r["code"] == hm.HOMOGRAPHY_NONE and r["n_valid"] == 0 and r["n_H"] == 0 and r["n_rot"] == 0
    assert not r["mask"].any() and not r["H"].any() and not r["R_rot"].any()


def test_fewer_than_six_matches_are_skipped(oracle, K_vga):
    p1, p2, _, _ = hc.scene_points("plane", 7, K_vga, 1)
    for M in (0, 5):
        r = hm.find_homography(gm.normalise_K(p1[:M], K_vga), gm.normalise_K(p2[:M], K_vga), np.zeros((hc.ITERS, 5), int), thr2_px(K_vga))
        assert r["code"] == hm.HOMOGRAPHY_SKIPPED and r["n_H"] == 0 and r["mask"].shape == (M,)


def test_ties_go_to_the_lowest_iteration(oracle, K_vga):
    """An exact homography without noise: every sample of four inliers explains all the inliers, the first of them wins;
    and the winner is the first maximum of the per-iteration counts."""
    M = 64
    sub = oracle.ransac_subsets(M, hc.ITERS)
    rng = np.random.default_rng(5)
    a = np.stack([rng.uniform(-0.5, 0.5, M), rng.uniform(-0.4, 0.4, M)], 1)
    Ht = np.array([[1.0, 0.05, 0.02], [-0.04, 0.98, -0.01], [0.1, -0.05, 1.0]])
    hb = np.concatenate([a, np.ones((M, 1))], 1) @ Ht.T
    b = hb[:, :2] / hb[:, 2:3]
    out = np.arange(0, M, 3)                                      # a third of the matches are outliers
    b[out] = rng.uniform(-0.5, 0.5, (len(out), 2))
    thr2 = thr2_px(K_vga)
    r = hm.find_homography(a, b, sub, thr2)
    H, G, valid = hm.four_point(a[sub[:, :4]], b[sub[:, :4]])
    cnt = np.where(valid, hm.inliers(H, G, a, b, thr2).sum(1), -1)
    clean = np.array([not (set(s) & set(out.tolist())) for s in sub[:, :4].tolist()])
    assert clean.sum() > 5 and (cnt[clean] == cnt.max()).sum() > 1          # a tie at the top
    assert r["it"] == int(np.flatnonzero(cnt == cnt.max())[0]) and r["n_H"] == cnt.max() == M - len(out)


# ------------------------------------------------------------------ classify_pair
def test_classify_pair_rule():
    from relative_pose_estimation_amd.geometry import classify_pair
    assert classify_pair(500, 482, 329, 362, 0.7, 0.8) == "rotation"
    assert classify_pair(500, 300, 280, 100, 0.7, 0.8) == "planar"
    assert classify_pair(500, 319, 98, 1, 0.7, 0.8) == "general"
    assert classify_pair(500, 300, 0, 0, 0.7, 0.8) == "general"               # max(n_H, 1): no homography is not a rotation
    assert classify_pair(10, 0, 1, 0, 0.7, 0.8) == "planar"                   # max(n_E, 1)
    assert classify_pair(500, 300, 100, 70, 0.7, 0.8) == "rotation" and classify_pair(500, 300, 100, 69, 0.7, 0.8) == "general"
    assert classify_pair(500, 100, 80, 0, 0.7, 0.8) == "planar" and classify_pair(500, 100, 79, 0, 0.7, 0.8) == "general"
    assert classify_pair(500, 319, 98, 1) == "general"                          # the defaults are those ratios


@pytest.fixture(scope="module")
def rows(oracle, K_vga):
    return hc.rendered_rows(oracle, K_vga)


def test_rendered_pairs_classify(rows):
    """Oracle pipeline (ORB-1000, 500 matches) + model, seeds 11 - 13.  Measured (matches, recoverPose inliers, n_E, n_H,
    n_rot): baseline 0.0: (500, 0, 482, 329, 362), (498, 15, 429, 267, 296), (498, 13, 435, 267, 290); baseline 0.4:
    (411, 386, 319, 98, 1), (444, 343, 339, 118, 40), (426, 410, 362, 46, 2)."""
    from relative_pose_estimation_amd.geometry import classify_pair
    for (seed, baseline), r in zip(hc.RENDERED, rows):
        m, M = r["model"], r["n_matches"]
        assert r["status"] == 0
        kind = classify_pair(M, r["n_E"], m["n_H"], m["n_rot"], hc.ROTATION_RATIO, hc.PLANAR_RATIO)
        if baseline == 0.0:
            assert kind == "rotation", (seed, kind)
            assert m["n_H"] >= 0.5 * M and r["oracle_inliers"] <= 0.1 * M, (seed, m["n_H"], r["oracle_inliers"], M)
        else:
            assert kind == "general", (seed, kind)
            assert m["n_H"] <= 0.5 * r["n_E"], (seed, m["n_H"], r["n_E"])


def test_rotation_fit_beats_the_five_point_rotation_on_rotation_only_pairs(rows):
    from relative_pose_estimation_amd import geometry
    for (seed, baseline), r in zip(hc.RENDERED, rows):
        if baseline == 0.0:
            e_rot = hm.rotation_angle_deg(r["model"]["R_rot"], r["R_gt"])
            assert e_rot < 0.05 and e_rot <= geometry.rotation_error(r["R_oracle"], r["R_gt"]), (seed, e_rot)


# ------------------------------------------------------------------ exports
def test_new_names_are_exported_and_declared():
    from relative_pose_estimation_amd import _capi
    header = open(os.path.join(ROOT, "include", "rpe_amd.h")).read()
    for name in ("rpe_pair_homographies", "rpe_find_homography"):
        assert name in _capi.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for code, value in (("RPE_HOMOGRAPHY_OK", 0), ("RPE_HOMOGRAPHY_SKIPPED", 1), ("RPE_HOMOGRAPHY_NONE", 2)):
        assert re.search(code + r"\s*=\s*%d\b" % value, header), code
    assert (_capi.HOMOGRAPHY_OK, _capi.HOMOGRAPHY_SKIPPED, _capi.HOMOGRAPHY_NONE) == (0, 1, 2)
    assert (hm.HOMOGRAPHY_OK, hm.HOMOGRAPHY_SKIPPED, hm.HOMOGRAPHY_NONE) == (0, 1, 2)
    for method in ("pair_homographies", "find_homography"):
        assert callable(getattr(_capi.Engine, method))
    from relative_pose_estimation_amd.pose_estimator import PoseEstimator
    assert callable(PoseEstimator.last_homographies) and callable(PoseEstimator.estimate_with_geometry)
