"""Non-linear pose refinement on the GPU (rpe_refine_poses / rpe_refine_pose_points, through the C-ABI): the kernel
against the float64 numpy model of the same algorithm (tests/refine_model.py), its invariants on real batches and
streams, and the refusals.

MARGIN.  The model run twice on the 16 noisy scenes of refine_model.noisy_scenes (10 iterations), with the residual sums
in forward and in reversed order, differs by at most 1.887e-15 px in rms_after, 8.866e-15 degrees in R and 1.252e-13
degrees in t (and 1.776e-15 px in rms_before, up to 12 px on these scenes), with no accept / reject decision differing (measured on
CPU).  Ten times those figures is the margin for
reduction-order effects between the kernel's tree and numpy's: 1.9e-14 px, 8.9e-14 degrees, 1.3e-12 degrees.  The tests
recompute the margin from the model instead of hard-coding it."""
import numpy as np
import pytest

from tests import refine_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def noisy(K_vga):
    """the 16 scenes, the model's forward results, its ties and the margin (rms px, R degrees, t degrees)"""
    scenes = rm.noisy_scenes(K_vga)
    fwd, ties, d_rms, d_R, d_t, d_rms0 = rm.reduction_margin(scenes, K_vga, 10)
    assert d_rms > 0 and d_R > 0 and d_t > 0 and d_rms0 > 0 and len(ties) <= 1
    return scenes, fwd, ties, (10 * d_rms, 10 * d_R, 10 * d_t, 10 * d_rms0)


def _blobs(seed, n, lo, hi, W=640, H=480):
    """a few bright rectangles on a dark background: a handful of FAST corners per image"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 40, np.uint8)
    for _ in range(n):
        w, h = rng.integers(lo, hi, 2)
        x = rng.integers(70, W - 70 - w); y = rng.integers(70, H - 70 - h)
        img[y:y + h, x:x + w] = rng.integers(150, 255)
    return img


def _bits(out):
    return [np.ascontiguousarray(a).view(np.uint64).copy() if a.dtype == np.float64 else a.copy() for a in out]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _against_model(gpu, models, margin, skip=()):
    """per pair: same code / iteration counts, rms_after and the pose within the margin, and the GPU cost not above the
    model's by more than the margin"""
    R, t, inl, info, rms = gpu
    m_rms, m_R, m_t, m_rms0 = margin
    worst = [0.0, 0.0, 0.0]
    for p, mo in enumerate(models):
        if p in skip:
            continue
        assert tuple(info[p]) == mo["info"], (p, info[p], mo["info"])
        assert inl[p] == mo["inliers"], (p, inl[p], mo["inliers"])
        d = (abs(rms[p, 1] - mo["rms"][1]), rm.rot_angle_deg(R[p], mo["R"]), rm.vec_angle_deg(t[p], mo["t"]))
        worst = [max(a, b) for a, b in zip(worst, d)]
        print("pair", p, "info", tuple(info[p]), "rms", rms[p], "model", mo["rms"], "d_rms %.3e d_R %.3e d_t %.3e" % d)
        assert abs(rms[p, 0] - mo["rms"][0]) <= m_rms0, (p, rms[p, 0], mo["rms"][0], m_rms0)
        assert rms[p, 1] <= mo["rms"][1] + m_rms, (p, rms[p, 1], mo["rms"][1])         # no slower than its specification
        assert d[0] <= m_rms and d[1] <= m_R and d[2] <= m_t, (p, d, margin)
    print("worst d_rms %.3e d_R %.3e d_t %.3e  margin %.3e %.3e %.3e (rms_before %.3e)" % (*worst, *margin))


def _invariants(capi, batch, struct, ref):
    """rms never up, pass-through bit-exact where not refined, rotations proper, inliers never down, residual count"""
    R0, t0, inl0, nm, st = batch
    R, t, inl, info, rms = ref
    B = len(st)
    assert (rms[:, 1] <= rms[:, 0]).all()
    assert np.array_equal(info[:, 2], struct[0].sum(1))
    for p in range(B):
        if info[p, 0] != capi.REFINE_OK:
            assert np.array_equal(R[p].view(np.uint64), R0[p].view(np.uint64)) and np.array_equal(t[p].view(np.uint64), t0[p].view(np.uint64))
            assert inl[p] == inl0[p] and rms[p, 0] == rms[p, 1]
        else:
            assert st[p] == 0 and inl[p] >= inl0[p] and info[p, 2] >= 6 and 1 <= info[p, 1] <= 10
            assert np.abs(R[p] @ R[p].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R[p]) - 1) <= 1e-12
            assert abs(np.linalg.norm(t[p]) - 1) <= 1e-12
        assert info[p, 3] <= info[p, 1]


# ------------------------------------------------------------------ 1. stage form vs the model
def test_stage_form_equals_model(capi, K_vga, noisy):
    """16 noisy exact-geometry scenes (sigma 0.5 px, f32 points, 300 matches, 60 outliers masked out, starts turned by
    0.5 ... 2 degrees) in one call, 10 iterations: per pair rms_after and the pose agree with the model within the
    margin of the module docstring (10 x the model's own forward / reversed difference: 1.9e-14 px, 8.9e-14 degrees in
    R, 1.3e-12 degrees in t), and the GPU cost is not above the model's by more than that margin."""
    scenes, fwd, ties, margin = noisy
    e = capi.Engine(640, 480, max_batch=16, nfeatures=1000, max_matches=500)
    gpu = e.refine_pose_points([s["R0"] for s in scenes], [s["t0"] for s in scenes], [s["pts1"] for s in scenes],
                               [s["pts2"] for s in scenes], [s["mask"] for s in scenes], K_vga, 10)
    again = e.refine_pose_points([s["R0"] for s in scenes], [s["t0"] for s in scenes], [s["pts1"] for s in scenes],
                                 [s["pts2"] for s in scenes], [s["mask"] for s in scenes], K_vga, 10)
    e.close()
    assert _same(gpu, again)
    assert (gpu[3][:, 0] == capi.REFINE_OK).sum() >= 12 and (gpu[4][:, 1] <= gpu[4][:, 0]).all()
    _against_model(gpu, fwd, margin, skip=ties)


# ------------------------------------------------------------------ 2. invariants on real batches
@pytest.mark.parametrize("B", [4, 8])
def test_batch_invariants(capi, K_vga, B):
    """device-resident ORB + Hamming batches (B = 4 is hipGraph-replayed): the invariants, the batch's own results and
    structure bit-identical before and after refine_poses in both call orders, and two calls bit-identical"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(8, K_vga, cfg=8)
    e = capi.Engine(640, 480, max_batch=8, nfeatures=1000, max_matches=500)
    da, db = e.upload(i1[:B]), e.upload(i2[:B])
    res = e.estimate_batch_device(da, db, B, K_vga)
    assert (res[4] == 0).all()
    s0 = e.fetch_structure(B)                     # structure first, then refine
    r1 = e.refine_poses(B, 10)
    r2 = e.refine_poses(B, 10)
    assert _same(r1, r2)
    assert _same(e.fetch_results(B), res) and _same(e.fetch_structure(B), s0)
    _invariants(capi, res, s0, r1)
    assert (r1[3][:, 0] == capi.REFINE_OK).any() and (r1[4][r1[3][:, 0] == capi.REFINE_OK, 1] < r1[4][r1[3][:, 0] == capi.REFINE_OK, 0]).all()
    res_b = e.estimate_batch_device(da, db, B, K_vga)         # refine first, then structure
    r3 = e.refine_poses(B, 10)
    assert _same(res_b, res) and _same(r3, r1)
    assert _same(e.fetch_structure(B), s0) and _same(e.fetch_results(B), res)
    assert not _same(e.refine_poses(B, 1)[:2], r1[:2])
    e.close()


# ------------------------------------------------------------------ 3. batch form vs stage form
def test_batch_equals_stage_form(capi, K_vga):
    """refine_poses after a batch equals refine_pose_points fed with that batch's matched points, RANSAC mask and pose,
    bit for bit (same kernel, same inputs)"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(8, K_vga, cfg=8)
    e = capi.Engine(640, 480, max_batch=8, nfeatures=1000, max_matches=500)
    R, t, inl, nm, st = e.estimate_batch_device(e.upload(i1), e.upload(i2), 8, K_vga)
    ref = e.refine_poses(8, 10)
    p1, p2 = e.fetch_matched_points(8)
    rmask = e.fetch_structure(8)[0]
    stage = e.refine_pose_points(R, t, [p1[p, :nm[p]] for p in range(8)], [p2[p, :nm[p]] for p in range(8)],
                                 [rmask[p, :nm[p]] for p in range(8)], K_vga, 10)
    e.close()
    assert _same(ref, stage)


# ------------------------------------------------------------------ 4. accuracy against ground truth
def test_accuracy_scenes_equal_model(capi, K_vga, noisy):
    """the 48 pairs of test_refine_cpu.test_model_accuracy_against_ground_truth: per pair the GPU's refined pose agrees
    with the model's (run on the batch's own matched points, mask and pose) within test 1's margin, hence so do the
    medians (model, CPU: 0.4805 -> 0.3050 degrees)"""
    from relative_pose_estimation_amd import synthetic, geometry
    margin = noisy[3]
    n = rm.ACCURACY_PAIRS
    i1, i2, Rgt, _ = synthetic.make_batch(n, K_vga, cfg=rm.ACCURACY_CFG, workers=4)
    e = capi.Engine(640, 480, max_batch=n, nfeatures=1000, max_matches=500)
    R, t, inl, nm, st = e.estimate_batch_device(e.upload(i1), e.upload(i2), n, K_vga)
    assert (st == 0).all()
    gpu = e.refine_poses(n, 10)
    p1, p2 = e.fetch_matched_points(n)
    rmask = e.fetch_structure(n)[0]
    e.close()
    models, ties = [], []
    for p in range(n):
        a = [rm.refine(R[p], t[p], p1[p, :nm[p]], p2[p, :nm[p]], rmask[p, :nm[p]], K_vga, 10, order=o) for o in ("forward", "reversed")]
        if a[0]["decisions"] != a[1]["decisions"] or a[0]["info"] != a[1]["info"]:
            ties.append(p)
        models.append(a[0])
    assert len(ties) * 16 <= n, ties
    _against_model(gpu, models, margin, skip=ties)
    e0 = np.array([geometry.rotation_error(R[p], Rgt[p]) for p in range(n)])
    e1 = np.array([geometry.rotation_error(gpu[0][p], Rgt[p]) for p in range(n)])
    print("median rotation error", np.median(e0), "->", np.median(e1))
    assert np.median(e1) < 0.75 * np.median(e0)


# ------------------------------------------------------------------ 5. stream and the other modes
def test_stream_refine_equals_pairwise(capi, K_vga):
    """refine_poses after estimate_stream equals the pairwise batch of the same frames bit for bit; the drop-in's
    last_refined / estimate_refined return the same numbers"""
    from relative_pose_estimation_amd import PoseEstimator, synthetic
    i1, i2, _, _ = synthetic.make_batch(3, K_vga, cfg=8)
    frames = np.stack([i1[0], i2[0], i1[1], i2[1], i1[2]])
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    rs = e.estimate_stream(frames, K_vga)
    fs = e.refine_poses(4, 10)
    _invariants(capi, rs, e.fetch_structure(4), fs)
    rp = e.estimate_batch(frames[:-1], frames[1:], K_vga)
    fp = e.refine_poses(4, 10)
    assert _same(rs, rp) and _same(fs, fp)
    e.close()
    pe = PoseEstimator(K_vga, nfeatures=1000, max_batch=4)
    R, t, inl, st = pe.estimate_sequence(frames)
    lr = pe.last_refined()
    assert len(lr) == 6 and np.array_equal(lr[3], st) and _same((lr[0], lr[1], lr[2], lr[4], lr[5]), fs)
    d = pe.estimate_refined(frames[0], frames[1])
    dbg = pe.estimate_with_debug(frames[0], frames[1])
    assert set(d) == set(dbg) | {'R_refined', 't_refined', 'inliers_refined', 'refine_code', 'refine_iters', 'rms_before', 'rms_after'}
    assert np.array_equal(d['R'], dbg['R']) and np.array_equal(d['R'], R[0])
    assert np.array_equal(d['R_refined'], fs[0][0]) and np.array_equal(d['t_refined'], fs[1][0])
    assert (d['inliers_refined'], d['refine_code'], d['refine_iters']) == (fs[2][0], fs[3][0, 0], fs[3][0, 1])
    assert (d['rms_before'], d['rms_after']) == (fs[4][0, 0], fs[4][0, 1])
    pe.close()


@pytest.mark.parametrize("mode", ["sift_l2", "orb_l2", "orb_ratio"])
def test_refine_other_modes(capi, K_vga, mode):
    from relative_pose_estimation_amd import synthetic, geometry
    if mode == "sift_l2":
        K = geometry.default_camera_matrix(320, 240)
        i1, i2, _, _ = synthetic.make_batch(2, K, 320, 240, cfg=6)
        e = capi.Engine(320, 240, max_batch=2, nfeatures=600, max_matches=300, feature_method=capi.FEATURE_SIFT,
                        norm_type=capi.NORM_L2)
    else:
        K = K_vga
        i1, i2, _, _ = synthetic.make_batch(2, K, cfg=2)
        kw = dict(norm_type=capi.NORM_L2) if mode == "orb_l2" else dict(match_mode=capi.MATCH_RATIO, match_ratio=0.8)
        e = capi.Engine(640, 480, max_batch=2, nfeatures=1000, max_matches=500, **kw)
    res = e.estimate_batch(i1, i2, K)
    assert (res[4] == 0).all()
    ref = e.refine_poses(2, 10)
    s = e.fetch_structure(2)
    assert _same(e.refine_poses(2, 10), ref) and _same(e.fetch_results(2), res)
    _invariants(capi, res, s, ref)
    e.close()


# ------------------------------------------------------------------ 6. ragged batch
def test_refine_of_failing_pairs(capi, K_vga):
    """fewer than 5 matches, exactly 5 (stacked models), a blank image and a good pair: the failed pairs come back
    skipped with identity R, zero t and zero inliers, exactly as the batch reported them; the good pair is refined"""
    from relative_pose_estimation_amd import synthetic
    ok1, ok2, _, _ = synthetic.make_batch(1, K_vga, cfg=2)
    flat = np.full((480, 640), 128, np.uint8)
    a = np.stack([_blobs(7, 1, 14, 40), _blobs(23, 1, 14, 40), flat, ok1[0]])
    b = np.stack([_blobs(1007, 1, 14, 40), _blobs(1023, 1, 14, 40), ok2[0], ok2[0]])
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    res = e.estimate_batch(a, b, K_vga)
    assert list(res[4]) == [capi.PAIR_INSUFFICIENT_MATCHES, capi.PAIR_AMBIGUOUS_ESSENTIAL, capi.PAIR_NO_DESCRIPTORS, capi.PAIR_OK]
    R, t, inl, info, rms = ref = e.refine_poses(4, 10)
    for p in range(3):
        assert tuple(info[p]) == (capi.REFINE_SKIPPED, 0, 0, 0) and inl[p] == 0 and not rms[p].any()
        assert np.array_equal(R[p], np.eye(3)) and not t[p].any()
    assert info[3, 0] == capi.REFINE_OK and info[3, 3] >= 1 and rms[3, 1] < rms[3, 0] and inl[3] >= res[2][3] > 0
    _invariants(capi, res, e.fetch_structure(4), ref)
    e.close()


# ------------------------------------------------------------------ 7. refusals
def test_refine_refusals(capi, K_vga):
    """refused before any batch, after a chunked host batch, after a stage-API call, for more pairs than the last batch
    had and for max_iters outside 1 ... 100, each with its text; a new device-resident batch makes it available again"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(3, K_vga, cfg=2)
    B = 512
    a = np.ascontiguousarray(np.concatenate([i1] * (B // 3 + 1))[:B]); b = np.ascontiguousarray(np.concatenate([i2] * (B // 3 + 1))[:B])
    e = capi.Engine(640, 480, max_batch=B, nfeatures=1000, max_matches=500)
    with pytest.raises(capi.RpeError, match="rpe_refine_poses: no batch or stream"):
        e.refine_poses(1)                                            # nothing run yet
    e.estimate_batch(a, b, K_vga)                                    # >= 512 pairs, 150 MiB per set: chunked
    with pytest.raises(capi.RpeError, match="rpe_refine_poses: the last host batch ran in chunks"):
        e.refine_poses(B)
    da, db = e.upload(a), e.upload(b)
    dev = e.estimate_batch_device(da, db, B, K_vga)
    ref = e.refine_poses(B, 10)
    for p in range(3, B):                                            # every copy of a pair is refined identically
        assert _same([x[p] for x in ref], [x[p % 3] for x in ref])
    for bad in (0, 101, -1):
        with pytest.raises(capi.RpeError, match="rpe_refine_poses: max_iters must be 1 ... 100"):
            e.refine_poses(1, bad)
    p1, p2 = e.fetch_matched_points(1)
    n = int(dev[3][0])
    e.find_essential([p1[0, :n]], [p2[0, :n]], K_vga)                # stage API overwrites the per-match buffers
    with pytest.raises(capi.RpeError, match="rpe_refine_poses: no batch or stream since the last stage-API call"):
        e.refine_poses(1)
    e.estimate_batch_device(da, db, 2, K_vga)
    assert _same(e.refine_poses(2, 10), [x[:2] for x in ref])
    with pytest.raises(capi.RpeError, match="rpe_refine_poses: more pairs than the last batch"):
        e.refine_poses(3)
    e.refine_pose_points(dev[0][:1], dev[1][:1], [p1[0, :n]], [p2[0, :n]], [np.ones(n, bool)], K_vga, 5)
    with pytest.raises(capi.RpeError, match="rpe_refine_poses: no batch or stream since the last stage-API call"):
        e.refine_poses(1)
    e.close()


# ------------------------------------------------------------------ 8. the streaming (non-LDS) branch
def test_streaming_branch_equals_model(capi, K_vga, noisy):
    """max_matches = 8064 (ORB nfeatures 8000) takes the branch that reads the points from HBM through the compacted
    index list: the 16 scenes of test 1 agree with the model within test 1's margin, and -- the list is walked in the
    same order -- with the LDS branch bit for bit.  A real 4-pair batch at that capacity (more than 1024 matches and 512
    inliers per pair, several residuals per lane) agrees with the model within the same margin and with its own stage form
    bit for bit; so do the scenes and a real batch on the LDS branch at its cut, max_matches = 2048."""
    from relative_pose_estimation_amd import synthetic
    scenes, fwd, ties, margin = noisy
    args = ([s["R0"] for s in scenes], [s["t0"] for s in scenes], [s["pts1"] for s in scenes], [s["pts2"] for s in scenes],
            [s["mask"] for s in scenes], K_vga, 10)
    small = capi.Engine(640, 480, max_batch=16, nfeatures=1000, max_matches=500)
    lds = small.refine_pose_points(*args)
    small.close()
    e = capi.Engine(640, 480, max_batch=16, nfeatures=8000, max_matches=8064)
    gpu = e.refine_pose_points(*args)
    _against_model(gpu, fwd, margin, skip=ties)
    assert _same(gpu, lds)
    # a real batch at that capacity: thousands of inliers per pair, several residuals per lane
    i1, i2, _, _ = synthetic.make_batch(4, K_vga, cfg=8)
    res = e.estimate_batch(i1, i2, K_vga)
    assert (res[4] == 0).all() and (res[3] > 1024).all()
    ref = e.refine_poses(4, 10)
    s = e.fetch_structure(4)
    assert (s[0].sum(1) > 512).all()
    _invariants(capi, res, s, ref)
    p1, p2 = e.fetch_matched_points(4)
    models, real_ties = [], []
    for p in range(4):
        n = res[3][p]
        a = [rm.refine(res[0][p], res[1][p], p1[p, :n], p2[p, :n], s[0][p, :n], K_vga, 10, order=o) for o in ("forward", "reversed")]
        if a[0]["decisions"] != a[1]["decisions"] or a[0]["info"] != a[1]["info"]:
            real_ties.append(p)
        models.append(a[0])
    assert not real_ties, real_ties                                   # cap: 1 pair in 16
    _against_model(ref, models, margin)
    stage = e.refine_pose_points(res[0], res[1], [p1[p, :res[3][p]] for p in range(4)], [p2[p, :res[3][p]] for p in range(4)],
                                 [s[0][p, :res[3][p]] for p in range(4)], K_vga, 10)
    assert _same(stage, ref)
    e.close()
    # the LDS branch at its cut (max_matches 2048: 64 KB of staged points): the same scenes, the same bits
    cut = capi.Engine(640, 480, max_batch=16, nfeatures=4000, max_matches=2048)
    assert _same(cut.refine_pose_points(*args), lds)
    res = cut.estimate_batch(i1, i2, K_vga)
    assert (res[4] == 0).all() and (res[3] > 1024).all()
    ref = cut.refine_poses(4, 10)
    s = cut.fetch_structure(4)
    _invariants(capi, res, s, ref)
    p1, p2 = cut.fetch_matched_points(4)
    models = []
    for p in range(4):
        n = res[3][p]
        a = [rm.refine(res[0][p], res[1][p], p1[p, :n], p2[p, :n], s[0][p, :n], K_vga, 10, order=o) for o in ("forward", "reversed")]
        assert a[0]["decisions"] == a[1]["decisions"] and a[0]["info"] == a[1]["info"], p
        models.append(a[0])
    _against_model(ref, models, margin)
    cut.close()


# ------------------------------------------------------------------ 9. the sequence front-end
def test_batch_processor_refine_columns(capi, K_vga):
    """BatchProcessor.process_frames(refine=True): the default columns are those of refine=False bit for bit, and the
    refined columns are Engine.refine_poses of the same stream composed with the ground-truth rotation of the previous
    frame, as the unrefined ones are"""
    from relative_pose_estimation_amd import BatchProcessor, PoseEstimator, synthetic
    from relative_pose_estimation_amd.geometry import euler_to_rotation, rotation_to_euler
    i1, i2, _, _ = synthetic.make_batch(3, K_vga, cfg=8)
    frames = np.stack([i1[0], i2[0], i1[1], i2[1], i1[2]])
    idx = [10, 11, 12, 13, 14]

    class GT:
        def get_pose(self, f):
            return {"roll": 0.5 * (f - 10), "pitch": -1.0 + 0.25 * f, "yaw": 3.0 * (f - 12)}
    pe = PoseEstimator(K_vga, nfeatures=1000, max_batch=4)
    bp = BatchProcessor(None, pe, GT())
    plain = bp.process_frames(idx, frames)
    out = bp.process_frames(idx, frames, refine=True)
    R, t, inl, info, rms = pe._engine(480, 640, 4).refine_poses(4)      # the engine process_frames ran the stream on
    pe.close()
    assert set(out) == set(plain) | {"R_refined", "t_refined", "roll_refined", "pitch_refined", "yaw_refined", "refine_code",
                                     "rms_before", "rms_after"}
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(out[k])), k
    assert np.array_equal(out["refine_code"], info[:, 0]) and (info[:, 0] == capi.REFINE_OK).any()
    assert np.array_equal(out["rms_before"], rms[:, 0]) and np.array_equal(out["rms_after"], rms[:, 1])
    for i in range(4):
        g = GT().get_pose(idx[i])
        Rw = euler_to_rotation(g["yaw"], g["pitch"], g["roll"], convention=bp.euler_convention) @ R[i]
        yaw, pitch, roll = rotation_to_euler(Rw, convention=bp.euler_convention)
        assert np.array_equal(out["R_refined"][i], Rw) and np.array_equal(out["t_refined"][i], t[i])
        assert (out["yaw_refined"][i], out["pitch_refined"][i], out["roll_refined"][i]) == (yaw, pitch, roll)
        if info[i, 0] == capi.REFINE_OK and info[i, 3] > 0:
            assert not np.array_equal(out["R_refined"][i], out["R"][i])
        else:
            assert np.array_equal(out["R_refined"][i], out["R"][i])
