"""recover_pose_kernel triangulates once per rotation and takes the verdict of (R, -t) from the mirror of (R, t)'s
(csrc/pose_triangulate.h).  Through the stage call Engine.recover_pose against the CPU oracle's recoverPose, which
triangulates all four hypotheses directly: match counts at the tails of the 256-stride match loop and of the wave sums,
essential matrices presented so that each of the four hypotheses (R1, t), (R2, t), (R1, -t), (R2, -t) wins somewhere
(E and -E, which exchanges R1 and R2; the second camera at t and at -t, the scene behind both cameras of the other; the two
views swapped) -- a condition the test checks on the CPU from the oracle alone.  And one image batch followed by fetch_structure: pose_structure_kernel triangulates the
RETURNED pose directly, so its mask sums to the inlier count only if the mirrored count of a -t winner is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_RT = 1e-4                  # R / t against the oracle, Frobenius: tests/test_gpu_parity.py
COUNTS = [5, 63, 64, 65, 255, 256, 257, 500]
PAIRS = 16
BATCH_CFG = 8                  # synthetic.make_batch(4, K, cfg=8): the batch of tests/test_gpu_structure.py; pairs 1, 3 swapped


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _scene(seed, M, K):
    """M matches of a seeded two-view scene (a fifth of them random outliers, a quarter pixel of noise on the rest) and an
    essential matrix of it.  Four pairs share one (R, t, X), seed >> 2, and present it in the four ways that make the four
    hypotheses win: E or -E (bit 0: decomposeEssentialMat hands back the same t and R1, R2 exchanged), and the second
    camera at t or at -t (bit 1: E(R, -t) = -E(R, t) decomposes to the same t as E(R, t), so the scene at -t -- the one
    whose points lie behind both cameras under (R, t) -- takes the other sign).  Odd groups have the two views swapped
    (the inverse motion, E^T)."""
    rng = np.random.default_rng(1000 * M + (seed >> 2))
    R = _rodrigues(rng.uniform(-1, 1, 3) * np.deg2rad(rng.uniform(2, 12)))
    t = rng.normal(size=3); t /= np.linalg.norm(t)
    if seed & 2:
        t = -t
    X = np.stack([rng.uniform(-3, 3, M), rng.uniform(-2, 2, M), rng.uniform(5, 20, M)], 1)
    Y = X @ R.T + t
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    p1 = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1) + rng.normal(0, 0.25, (M, 2))
    p2 = np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1) + rng.normal(0, 0.25, (M, 2))
    out = rng.random(M) < 0.2
    p2[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    if (seed >> 2) & 1:
        p1, p2, E = p2, p1, E.T
    if seed & 1:
        E = -E
    return E, p1.astype(np.float32), p2.astype(np.float32)


def _winner(oracle, E, R_o, t_o):
    """which of (R1, t), (R2, t), (R1, -t), (R2, -t) the oracle returned: 0..3"""
    R1, R2, tt = oracle.decompose_essential(E)
    hyp = [(R1, tt), (R2, tt), (R1, -tt), (R2, -tt)]
    hit = [k for k, (R, t) in enumerate(hyp) if np.array_equal(R, R_o) and np.array_equal(t, t_o.reshape(3))]
    assert len(hit) == 1, hit
    return hit[0]


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def eng(capi):
    e = capi.Engine(640, 480, max_batch=PAIRS, nfeatures=500, max_matches=500)
    yield e
    e.close()


@pytest.mark.parametrize("M", COUNTS)
def test_recover_pose_all_four_hypotheses(eng, oracle, K_vga, M):
    scenes = [_scene(s, M, K_vga) for s in range(PAIRS)]
    ref = [oracle.recover_pose(E, p1, p2, K_vga) for E, p1, p2 in scenes]
    winners = [_winner(oracle, sc[0], r[1], r[2]) for sc, r in zip(scenes, ref)]
    print("M", M, "winners", winners, "inliers", [r[0] for r in ref])
    assert set(winners) == {0, 1, 2, 3}, winners                           # a condition of the test, from the oracle alone
    R, t, inl = eng.recover_pose(np.stack([sc[0] for sc in scenes]), [sc[1] for sc in scenes], [sc[2] for sc in scenes], K_vga)
    for i, (n_o, R_o, t_o) in enumerate(ref):
        assert inl[i] == n_o, (M, i, winners[i], inl[i], n_o)
        assert np.linalg.norm(R[i] - R_o) <= TOL_RT and np.linalg.norm(t[i] - t_o) <= TOL_RT, (M, i, winners[i])
        assert np.array_equal(R[i], R_o) and np.array_equal(t[i], t_o), f"M {M} pair {i}: R/t not bit-identical"


def _image_batch(K):
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(4, K, cfg=BATCH_CFG)
    a, b = i1.copy(), i2.copy()
    a[[1, 3]], b[[1, 3]] = i2[[1, 3]], i1[[1, 3]]                          # two pairs run backwards
    return a, b


def test_structure_mask_sums_to_inliers_for_minus_t_winners(capi, oracle, K_vga):
    i1, i2 = _image_batch(K_vga)
    out, pts = oracle.estimate_pose_batch(i1, i2, K_vga, 1000, 500, return_points=True)
    winners = []
    for p in range(4):
        assert out[p]["status"] == 0
        n = int(out[p]["n_matches"])
        E, _, _ = oracle.find_essential(pts[p, 0, :n], pts[p, 1, :n], K_vga)
        winners.append(_winner(oracle, E, np.array(out[p]["R"]).reshape(3, 3), np.array(out[p]["t"]).reshape(3)))
    print("winners", winners)
    assert any(w >= 2 for w in winners), winners                           # at least one returned t is a -t hypothesis
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    try:
        R, t, inl, nm, st = e.estimate_batch(i1, i2, K_vga)
        rm, pm, _ = e.fetch_structure(4)
    finally:
        e.close()
    for p in range(4):
        assert st[p] == 0 and nm[p] == out[p]["n_matches"] and inl[p] == out[p]["inliers"], (p, st[p], nm[p], inl[p])
        assert np.linalg.norm(R[p].ravel() - out[p]["R"]) <= TOL_RT and np.linalg.norm(t[p].ravel() - out[p]["t"]) <= TOL_RT, p
        assert int(pm[p].sum()) == int(inl[p]), (p, winners[p], int(pm[p].sum()), int(inl[p]))
