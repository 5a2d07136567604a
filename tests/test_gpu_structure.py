"""Per-match structure of batch and stream runs (rpe_fetch_structure, through the C-ABI): findEssentialMat's inlier
mask equals the CPU oracle's bit for bit, recoverPose's cheirality mask sums to the inlier count and equals the float64
model's (tests/structure_model.py), the triangulated points match the model, and the call is refused where the
per-match buffers no longer describe the last batch."""
import numpy as np
import pytest

from tests import structure_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


def _blobs(seed, n, lo, hi, W=640, H=480):
    """a few bright rectangles on a dark background: a handful of FAST corners per image"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 40, np.uint8)
    for _ in range(n):
        w, h = rng.integers(lo, hi, 2)
        x = rng.integers(70, W - 70 - w); y = rng.integers(70, H - 70 - h)
        img[y:y + h, x:x + w] = rng.integers(150, 255)
    return img


def _check_structure(oracle, e, K, res, struct, model=True):
    """every pair of a batch: RANSAC mask == oracle.find_essential's on the batch's matched points, pose mask sums to
    the inlier count (and equals the model's), points match the model, zeros past n_matches and for failed pairs"""
    R, t, inl, nm, st = res
    rm, pm, pts = struct
    B = len(st)
    p1s, p2s = e.fetch_matched_points(B)
    assert rm.dtype == bool and pm.dtype == bool and pts.dtype == np.float64
    assert rm.shape == pm.shape == (B, e.max_matches) and pts.shape == (B, e.max_matches, 3)
    for p in range(B):
        n = int(nm[p])
        assert not rm[p, n:].any() and not pm[p, n:].any() and not pts[p, n:].any(), p
        if st[p] != 0:
            assert not rm[p].any() and not pm[p].any() and not pts[p].any(), p
            continue
        p1, p2 = p1s[p, :n], p2s[p, :n]
        E, omask, _ = oracle.find_essential(p1, p2, K)
        assert np.array_equal(rm[p, :n], omask.astype(bool)), p
        assert int(pm[p].sum()) == int(inl[p]), (p, pm[p].sum(), inl[p])
        if not model:
            continue
        mask, P, near = sm.triangulate(R[p], t[p], p1, p2, K)
        assert not ((pm[p, :n] != mask) & ~near).any(), (p, np.nonzero(pm[p, :n] != mask))
        sel = pm[p, :n] & mask
        err = np.linalg.norm(pts[p, :n][sel] - P[sel], axis=1)
        assert np.all(err <= 1e-7 * np.maximum(1.0, np.linalg.norm(P[sel], axis=1))), (p, err.max())


def _bits(struct):
    rm, pm, pts = struct
    return rm.copy(), pm.copy(), pts.view(np.uint64).copy()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# ------------------------------------------------------------------ 1. batch, ORB + Hamming, VGA
def test_batch_structure_orb_hamming(capi, oracle, K_vga):
    """device-resident (hipGraph-replayed at B = 4) and unchunked host batches of 4 VGA pairs"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(4, K_vga, cfg=8)
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    da, db = e.upload(i1), e.upload(i2)
    dev = e.estimate_batch_device(da, db, 4, K_vga)
    sd = e.fetch_structure(4)
    assert (dev[4] == 0).all() and (dev[2] > 100).all()
    _check_structure(oracle, e, K_vga, dev, sd)
    host = e.estimate_batch(i1, i2, K_vga)
    sh = e.fetch_structure(4)
    for x, y in zip(host, dev):
        assert np.array_equal(x, y)
    assert _same(sh, sd)
    _check_structure(oracle, e, K_vga, host, sh)
    e.close()


def test_estimate_with_structure(capi, oracle, K_vga):
    """the drop-in's per-pair call: estimate_with_debug's pose, matches and inliers plus the trimmed structure"""
    from relative_pose_estimation_amd import PoseEstimator, synthetic
    i1, i2, _, _ = synthetic.make_batch(1, K_vga, cfg=8)
    pe = PoseEstimator(K_vga, nfeatures=1000, use_vp_refinement=True)
    d = pe.estimate_with_structure(i1[0], i2[0])
    dbg = pe.estimate_with_debug(i1[0], i2[0])
    n = dbg['num_matches']
    assert set(d) == {'R', 't', 'num_matches', 'pts1', 'pts2', 'inliers', 'ransac_mask', 'pose_mask', 'points3d'}
    for k in ('R', 't', 'num_matches', 'pts1', 'pts2', 'inliers'):
        assert np.array_equal(d[k], dbg[k]), k
    assert d['ransac_mask'].shape == d['pose_mask'].shape == (n,) and d['points3d'].shape == (n, 3)
    assert int(d['pose_mask'].sum()) == d['inliers']
    mask, P, near = sm.triangulate(d['R'], d['t'], d['pts1'], d['pts2'], K_vga)
    assert not ((mask != d['pose_mask']) & ~near).any()
    E, omask, _ = oracle.find_essential(d['pts1'], d['pts2'], K_vga)
    assert np.array_equal(d['ransac_mask'], omask.astype(bool))
    with pytest.raises(RuntimeError, match="Could not compute descriptors"):
        pe.estimate_with_structure(np.full((480, 640), 128, np.uint8), i2[0])
    pe.close()


# ------------------------------------------------------------------ 2. physics
def test_structure_depths_cluster_at_plane_depths(capi, K_vga):
    """make_pair's planes at depths 4, 7, 12 with baseline 0.4: pose inliers triangulate at 10, 17.5, 30 on the
    |t| = 1 scale (band fixed from the CPU oracle in test_structure_cpu.py)"""
    from relative_pose_estimation_amd import synthetic
    pairs = [synthetic.make_pair(s, K_vga, baseline=sm.PHYSICS_BASELINE) for s in sm.PHYSICS_SEEDS]
    i1 = np.stack([p[0] for p in pairs]); i2 = np.stack([p[1] for p in pairs])
    B = len(pairs)
    e = capi.Engine(640, 480, max_batch=B, nfeatures=1000, max_matches=500)
    R, t, inl, nm, st = e.estimate_batch(i1, i2, K_vga)
    rm, pm, pts = e.fetch_structure(B)
    Zs = []
    for p in range(B):
        assert st[p] == 0 and pm[p].sum() == inl[p]
        frac, _ = sm.depth_clusters(pts[p][pm[p], 2], synthetic.DEPTHS)
        assert frac >= sm.DEPTH_BAND, (p, frac)
        Zs.append(pts[p][pm[p], 2])
    frac, per_plane = sm.depth_clusters(np.concatenate(Zs), synthetic.DEPTHS)
    assert frac >= sm.DEPTH_BAND and min(per_plane) >= 50, (frac, per_plane)
    e.close()


# ------------------------------------------------------------------ 3. stream
def test_stream_structure_equals_pairwise(capi, oracle, K_vga):
    """estimate_sequence's structure is bit-identical to pairwise batches of the same frames"""
    from relative_pose_estimation_amd import PoseEstimator, synthetic
    i1, i2, _, _ = synthetic.make_batch(3, K_vga, cfg=8)
    frames = np.stack([i1[0], i2[0], i1[1], i2[1], i1[2]])
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    rs = e.estimate_stream(frames, K_vga)
    ss = e.fetch_structure(4)
    _check_structure(oracle, e, K_vga, rs, ss)
    rp = e.estimate_batch(frames[:-1], frames[1:], K_vga)
    sp = e.fetch_structure(4)
    for x, y in zip(rs, rp):
        assert np.array_equal(x, y)
    assert _same(ss, sp)
    e.close()
    pe = PoseEstimator(K_vga, nfeatures=1000, max_batch=4)
    R, t, inl, st = pe.estimate_sequence(frames)
    ls = pe.last_structure()
    assert len(ls) == 4
    for p in range(4):
        n = int(rs[3][p])
        assert np.array_equal(ls[p]['ransac_mask'], ss[0][p, :n]) and np.array_equal(ls[p]['pose_mask'], ss[1][p, :n])
        assert np.array_equal(ls[p]['points3d'].view(np.uint64), ss[2][p, :n].view(np.uint64))
        assert int(ls[p]['pose_mask'].sum()) == inl[p]
    pe.close()


# ------------------------------------------------------------------ 4. the other feature / matcher modes
@pytest.mark.parametrize("mode", ["sift_l2", "orb_l2", "orb_ratio"])
def test_structure_other_modes(capi, oracle, K_vga, mode):
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
    _check_structure(oracle, e, K, res, e.fetch_structure(2), model=False)
    e.close()


# ------------------------------------------------------------------ 5. failing pairs
def test_structure_of_failing_pairs(capi, oracle, K_vga):
    """a ragged batch: fewer than 5 matches, exactly 5 (stacked models), a blank image and a good pair -- the failed
    pairs' masks and points are zero, and every pair is zero past its match count"""
    from relative_pose_estimation_amd import synthetic
    ok1, ok2, _, _ = synthetic.make_batch(1, K_vga, cfg=2)
    flat = np.full((480, 640), 128, np.uint8)
    a = np.stack([_blobs(7, 1, 14, 40), _blobs(23, 1, 14, 40), flat, ok1[0]])
    b = np.stack([_blobs(1007, 1, 14, 40), _blobs(1023, 1, 14, 40), ok2[0], ok2[0]])
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    res = e.estimate_batch(a, b, K_vga)
    st = res[4]
    assert list(st) == [capi.PAIR_INSUFFICIENT_MATCHES, capi.PAIR_AMBIGUOUS_ESSENTIAL, capi.PAIR_NO_DESCRIPTORS, capi.PAIR_OK]
    s = e.fetch_structure(4)
    _check_structure(oracle, e, K_vga, res, s)
    assert res[3][0] > 0 and res[3][1] == 5 and s[1][3].sum() == res[2][3] > 0
    e.close()


# ------------------------------------------------------------------ 6. refusals
def test_structure_refusals(capi, K_vga):
    """refused after a chunked host batch, after a stage-API call and for more pairs than the last batch had; a new
    device-resident batch makes it available again"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(3, K_vga, cfg=2)
    B = 512
    a = np.ascontiguousarray(np.concatenate([i1] * (B // 3 + 1))[:B]); b = np.ascontiguousarray(np.concatenate([i2] * (B // 3 + 1))[:B])
    e = capi.Engine(640, 480, max_batch=B, nfeatures=1000, max_matches=500)
    with pytest.raises(capi.RpeError, match="rpe_fetch_structure"):
        e.fetch_structure(1)                                         # nothing run yet
    host = e.estimate_batch(a, b, K_vga)                             # >= 512 pairs, 150 MiB per set: chunked
    with pytest.raises(capi.RpeError, match="ran in chunks"):
        e.fetch_structure(B)
    da, db = e.upload(a), e.upload(b)
    dev = e.estimate_batch_device(da, db, B, K_vga)
    for x, y in zip(host, dev):
        assert np.array_equal(x, y)
    rm, pm, pts = e.fetch_structure(B)
    assert np.array_equal(pm.sum(1), dev[2])
    for p in range(3, B):                                            # every copy of a pair describes it identically
        assert np.array_equal(pm[p], pm[p % 3]) and np.array_equal(pts[p].view(np.uint64), pts[p % 3].view(np.uint64))
    p1, p2 = e.fetch_matched_points(1)
    n = int(dev[3][0])
    e.find_essential([p1[0, :n]], [p2[0, :n]], K_vga)                # stage API overwrites the per-match buffers
    with pytest.raises(capi.RpeError, match="stage-API"):
        e.fetch_structure(1)
    e.estimate_batch_device(da, db, 2, K_vga)
    s2 = e.fetch_structure(2)
    assert np.array_equal(s2[1], pm[:2]) and np.array_equal(s2[2].view(np.uint64), pts[:2].view(np.uint64))
    with pytest.raises(capi.RpeError, match="more pairs than the last batch"):
        e.fetch_structure(3)
    e.close()


# ------------------------------------------------------------------ 7. no side effects
def test_structure_fetch_has_no_side_effects(capi, oracle, K_vga):
    """two different pairs back to back at B = 1 (the hipGraph-replayed path): results are bit-identical with and
    without a fetch in between, and the second fetch describes the second pair"""
    from relative_pose_estimation_amd import synthetic
    i1, i2, _, _ = synthetic.make_batch(2, K_vga, cfg=8)
    with_fetch = capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=500)
    plain = capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=500)
    ra = with_fetch.estimate_batch(i1[:1], i2[:1], K_vga)
    sa = with_fetch.fetch_structure(1)
    rb = with_fetch.estimate_batch(i1[1:], i2[1:], K_vga)
    sb = with_fetch.fetch_structure(1)
    qa = plain.estimate_batch(i1[:1], i2[:1], K_vga)
    qb = plain.estimate_batch(i1[1:], i2[1:], K_vga)
    for x, y in zip(ra + rb, qa + qb):
        assert np.array_equal(x, y)
    assert _same(plain.fetch_structure(1), sb)
    assert not _same(sa, sb)
    _check_structure(oracle, with_fetch, K_vga, rb, sb)
    # and a fetch between two batches leaves the next batch's results alone on the same handle
    rc = with_fetch.estimate_batch(i1[:1], i2[:1], K_vga)
    for x, y in zip(rc, ra):
        assert np.array_equal(x, y)
    assert _same(with_fetch.fetch_structure(1), sa)
    with_fetch.close(); plain.close()
