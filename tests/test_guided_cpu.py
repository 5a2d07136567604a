"""Guided matching on the CPU: the float64 model (tests/guided_model.py) against a plain-loop restatement of the rule,
against the oracle's crossCheck when the gate is open, the containment property on real frames, max_distance, and the
two bindings."""
import numpy as np

from tests import guided_model as gm
from tests import scale_model as sc


def _pose(rng):
    from tests import refine_model as rm
    R = rm.rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 1, 3)
    return R, t / np.linalg.norm(t)


def test_vectorised_model_equals_the_loops():
    """tiny inputs, descriptors from a pool of 4 patterns: distance ties dominate; gate widths from shut to open"""
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    seen_partial = 0
    for trial in range(60):
        n1, n2 = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        d1 = pool[rng.integers(0, 4, n1)].reshape(n1, 32); d2 = pool[rng.integers(0, 4, n2)].reshape(n2, 32)
        x1 = rng.uniform(-0.5, 0.5, (n1, 2)); x2 = rng.uniform(-0.5, 0.5, (n2, 2))
        R, t = _pose(rng)
        thr2 = gm.thr2_of(float(rng.choice([1.0, 20.0, 80.0, 1e9])), 500.0)
        md = int(rng.choice([0, 100, 256]))
        mm = None if trial % 3 else 3
        a = gm.guided_match(d1, x1, d2, x2, R, t, thr2, md, mm)
        b = gm.guided_match_slow(d1, x1, d2, x2, R, t, thr2, md, mm)
        for u, v in zip(a, b):
            assert np.array_equal(u, v), (trial, a, b)
        if n1 and n2:
            g = gm.gate_block(gm.essential(R, t), x1, x2, thr2)
            seen_partial += bool(g.any() and not g.all())
    assert seen_partial >= 10          # the gate cut through the population in many trials


def test_open_gate_equals_the_oracle_crosscheck():
    from oracle import oracle
    from relative_pose_estimation_amd import geometry, synthetic
    K = geometry.default_camera_matrix(640, 480)
    i1, i2, _, _ = synthetic.make_batch(1, K, cfg=9)
    (k1, d1), (k2, d2) = oracle.orb_detect_and_compute(i1[0], 1000), oracle.orb_detect_and_compute(i2[0], 1000)
    x1 = gm.normalise_K(np.stack([k1["x"], k1["y"]], 1), K); x2 = gm.normalise_K(np.stack([k2["x"], k2["y"]], 1), K)
    q, t, d = gm.guided_match(d1, x1, d2, x2, np.eye(3), [1., 0., 0.], gm.thr2_of(1e9, gm.focal_K(K)), 256, 500)
    oq, ot, od = oracle.match_hamming(d1, d2, 500)
    assert len(oq) > 100
    assert np.array_equal(q, oq) and np.array_equal(t, ot) and np.array_equal(d, np.asarray(od).astype(np.int64))


def test_admissible_crosscheck_matches_are_guided_matches():
    """PHYSICS frames at the oracle's poses: every crossCheck match the gate admits is in the untruncated guided set"""
    from oracle import oracle
    frames, K = sc.physics_frames()
    pairs = [(0, 1), (1, 2), (0, 2)]
    run = sc.oracle_run(oracle, frames[:3], pairs, K)
    feats = [oracle.orb_detect_and_compute(f, sc.PHYSICS_NFEATURES) for f in frames[:3]]
    thr2 = gm.thr2_of(1.0, gm.focal_K(K))
    for p, (a, b) in enumerate(pairs):
        assert run.status[p] == 0
        (k1, d1), (k2, d2) = feats[a], feats[b]
        x1 = gm.normalise_K(np.stack([k1["x"], k1["y"]], 1), K); x2 = gm.normalise_K(np.stack([k2["x"], k2["y"]], 1), K)
        cq, ct, _ = oracle.match_hamming(d1, d2, len(d1))                     # untruncated crossCheck
        gate = gm.gate_block(gm.essential(run.R[p], run.t[p]), x1, x2, thr2)
        adm = gate[cq, ct]
        q, t, _ = gm.guided_match(d1, x1, d2, x2, run.R[p], run.t[p], thr2)
        guided = set(zip(q.tolist(), t.tolist()))
        kept = [(i, j) for i, j, ok in zip(cq.tolist(), ct.tolist(), adm) if ok]
        print(f"pair {pairs[p]}: crossCheck {len(cq)}, admitted {len(kept)}, guided {len(q)}, RANSAC inliers {int(run.ransac_mask[p].sum())}")
        assert 0 < len(kept) < len(cq)
        assert all(m in guided for m in kept)
        assert all(gate[i, j] for i, j in guided)


def test_max_distance_zero_keeps_identical_descriptors_only():
    rng = np.random.default_rng(5)
    n = 40
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2 = d1.copy()
    d2[::2, 0] ^= 1                                     # every second train differs from its query by one bit
    x = rng.uniform(-0.3, 0.3, (n, 2))
    q, t, d = gm.guided_match(d1, x, d2, x, np.eye(3), [1., 0., 0.], gm.thr2_of(1e9, 500.0), 0)
    assert np.array_equal(q, np.arange(1, n, 2)) and np.array_equal(t, q) and not d.any()
    q1, _, d1_ = gm.guided_match(d1, x, d2, x, np.eye(3), [1., 0., 0.], gm.thr2_of(1e9, 500.0), 1)
    assert len(q1) == n and sorted(d1_.tolist()) == [0] * (n // 2) + [1] * (n // 2)


def test_bindings_are_listed():
    from relative_pose_estimation_amd import _capi
    assert "rpe_guided_matches" in _capi.EXPORTS and "rpe_match_hamming_guided" in _capi.EXPORTS


def test_library_exports_the_guided_calls():
    from relative_pose_estimation_amd import _capi
    lib = _capi.load()
    assert hasattr(lib, "rpe_guided_matches") and hasattr(lib, "rpe_match_hamming_guided")
