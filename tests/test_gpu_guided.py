"""Guided matching on the GPU (rpe_guided_matches / rpe_match_hamming_guided, through the C-ABI) against the float64 model
(tests/guided_model.py).  Equality is exact: the indices and distances with array_equal, the points with array_equal.
Covered: tile edges and empty sides, distance ties, both election forms (words in HBM with the split grid and with
kcap = 8064; words in LDS for batches beyond the split limit), truncation, streams, pair lists, failed pairs, supplied
poses, cameras, the refusals, and that the call changes nothing of the run it reads."""
import numpy as np
import pytest

from tests import camera_model as cm
from tests import guided_model as gm
from tests import scale_model as sc

pytestmark = pytest.mark.gpu

SHAPES = [(70, 33), (32, 64), (1, 1000), (0, 50)]


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


def synthetic_pairs(shapes, K, seed=3):
    """Per (n1, n2): keypoint k of either image is the projection of 3-D point k through a known (R, t) plus 0 .. 3 px of
    noise, so a 1 px gate cuts through the population; its descriptor is one of 8 patterns with two bits flipped by k
    and up to one more by chance: the true correspondence is the nearest, and distance ties are everywhere."""
    from tests import refine_model as rm
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    R = rm.rodrigues(np.array([0.02, -0.05, 0.01])); t = np.array([0.9, 0.1, -0.2]); t /= np.linalg.norm(t)
    K = np.asarray(K, np.float64)
    out = []
    for n1, n2 in shapes:
        N = max(n1, n2, 1)
        X = np.stack([rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 10, N)], 1)
        Y = X @ R.T + t

        def image(P, n):
            uv = P[:, :2] / P[:, 2:3]
            px = np.stack([uv[:, 0] * K[0, 0] + K[0, 2], uv[:, 1] * K[1, 1] + K[1, 2]], 1)
            ang = rng.uniform(0, 2 * np.pi, N); mag = rng.uniform(0, 3, N)
            px += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
            d = pool[np.arange(N) % 8].copy()
            for k in range(N):
                for bit in ((k * 7) % 256, (k * 13 + 5) % 256):
                    d[k, bit >> 3] ^= 1 << (bit & 7)
                if rng.random() < 0.5:
                    bit = int(rng.integers(0, 256)); d[k, bit >> 3] ^= 1 << (bit & 7)
            return d[:n], px[:n].astype(np.float32)
        d1, p1 = image(X, n1); d2, p2 = image(Y, n2)
        out.append((d1, p1, d2, p2))
    return out, R, t


def model_stage(data, K, R, t, gate_px, max_distance, mm):
    res = []
    for d1, p1, d2, p2 in data:
        res.append(gm.guided_match(d1, gm.normalise_K(p1, K), d2, gm.normalise_K(p2, K), R, t,
                                   gm.thr2_of(gate_px, gm.focal_K(K)), max_distance, mm))
    return res


def run_stage(e, data, K, R, t, gate_px, max_distance):
    B = len(data)
    return e.match_hamming_guided([d[0] for d in data], [d[1] for d in data], [len(d[0]) for d in data],
                                  [d[2] for d in data], [d[3] for d in data], [len(d[2]) for d in data], K,
                                  np.tile(R, (B, 1, 1)), np.tile(t, (B, 1)), gate_px, max_distance)


def assert_equal_lists(got, want, mm):
    q, ti, d, nm = got
    for p, (mq, mt, md) in enumerate(want):
        n = len(mq)
        assert nm[p] == n, (p, int(nm[p]), n)
        assert np.array_equal(q[p, :n], mq) and np.array_equal(ti[p, :n], mt) and np.array_equal(d[p, :n], md), p
        assert (q[p, n:] == -1).all() and (ti[p, n:] == -1).all() and (d[p, n:] == -1).all(), p


@pytest.fixture(scope="module")
def stage_case(K_vga):
    data, R, t = synthetic_pairs(SHAPES, K_vga)
    return data, R, t


# ------------------------------------------------------------------ 1 - 3. stage form
def test_stage_form_smallest_shapes(capi, K_vga, stage_case):
    data, R, t = stage_case
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    want = model_stage(data, K_vga, R, t, 1.0, 40, 500)
    # the inputs exercise the gate: some pair has crossCheck matches the gate admits and crossCheck matches it rejects
    both = False
    for (d1, p1, d2, p2), (mq, mt, _) in zip(data, want):
        cq, ct, _ = gm.guided_match(d1, gm.normalise_K(p1, K_vga), d2, gm.normalise_K(p2, K_vga), R, t, gm.thr2_of(1e9, gm.focal_K(K_vga)))
        if len(cq):
            g = gm.gate_block(gm.essential(R, t), gm.normalise_K(p1, K_vga), gm.normalise_K(p2, K_vga), gm.thr2_of(1.0, gm.focal_K(K_vga)))[cq, ct]
            both = both or (g.any() and not g.all())
    assert both
    assert sum(len(w[0]) for w in want) > 20
    assert_equal_lists(run_stage(e, data, K_vga, R, t, 1.0, 40), want, 500)
    e.close()


def test_open_gate_equals_crosscheck(capi, K_vga, stage_case):
    data, R, t = stage_case
    e = capi.Engine(640, 480, max_batch=4, nfeatures=1000, max_matches=500)
    g = run_stage(e, data, K_vga, R, t, 1e9, 256)
    c = e.match_hamming([d[0] for d in data], [len(d[0]) for d in data], [d[2] for d in data], [len(d[2]) for d in data])
    assert c[3].sum() > 50
    for p in range(len(data)):
        n = int(c[3][p])
        assert g[3][p] == n
        for a, b in zip(g[:3], c[:3]):
            assert np.array_equal(a[p, :n], b[p, :n]), p
    e.close()


def test_truncation_keeps_the_head_of_the_sorted_list(capi, K_vga):
    data, R, t = synthetic_pairs([(200, 200)], K_vga, seed=4)
    full = model_stage(data, K_vga, R, t, 2.0, 256, None)
    assert len(full[0][0]) > 16
    e = capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=16)
    got = run_stage(e, data, K_vga, R, t, 2.0, 256)
    assert_equal_lists(got, [tuple(a[:16] for a in full[0])], 16)
    e.close()


# ------------------------------------------------------------------ 4. election forms
def test_election_words_in_hbm_at_full_capacity(capi, K_vga):
    """kcap = 8064: 8 bytes of election words per keypoint no longer fit LDS beside the staging"""
    e = capi.Engine(640, 480, max_batch=1, nfeatures=8000, max_matches=500)
    assert e.kcap == 8064
    data, R, t = synthetic_pairs([(8064, 8064)], K_vga, seed=5)
    assert_equal_lists(run_stage(e, data, K_vga, R, t, 1.0, 40), model_stage(data, K_vga, R, t, 1.0, 40, 500), 500)
    e.close()


def test_single_pair_takes_the_split_grid(capi, K_vga):
    e = capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=500)
    data, R, t = synthetic_pairs([(1064, 1001)], K_vga, seed=6)
    assert_equal_lists(run_stage(e, data, K_vga, R, t, 1.0, 40), model_stage(data, K_vga, R, t, 1.0, 40, 500), 500)
    e.close()


def test_election_words_in_lds_beyond_the_split_limit(capi, K_vga):
    """more than 64 pairs: one workgroup per pair, election words in LDS, fused select.  kcap = 364: two rounds of 8 tiles"""
    B = 65
    e = capi.Engine(640, 480, max_batch=B, nfeatures=300, max_matches=100)
    rng = np.random.default_rng(8)
    shapes = [(int(rng.integers(0, 365)), int(rng.integers(0, 365))) for _ in range(B - 4)] + [(364, 364), (33, 300), (0, 10), (5, 0)]
    data, R, t = synthetic_pairs(shapes, K_vga, seed=7)
    want = model_stage(data, K_vga, R, t, 1.5, 60, 100)
    assert max(len(w[0]) for w in want) == 100 and min(len(w[0]) for w in want) == 0
    assert_equal_lists(run_stage(e, data, K_vga, R, t, 1.5, 60), want, 100)
    e.close()


# ------------------------------------------------------------------ 5 - 7. run form
def model_run(kps, desc, cnt, pairs, R, t, st, thr2, mm, norm1, norm2, max_distance=256, own_poses=True):
    """the model over a run: pair p = (image a, image b) of the fetched features"""
    out = []
    for p, (a, b) in enumerate(pairs):
        if own_poses and st[p] != 0:
            out.append((np.zeros(0, np.int64),) * 3)
            continue
        pa = np.stack([kps[a]["x"][:cnt[a]], kps[a]["y"][:cnt[a]]], 1); pb = np.stack([kps[b]["x"][:cnt[b]], kps[b]["y"][:cnt[b]]], 1)
        out.append(gm.guided_match(desc[a][:cnt[a]], norm1(p, pa), desc[b][:cnt[b]], norm2(p, pb), R[p], t[p],
                                   thr2(p), max_distance, mm))
    return out


def check_run(e, kps, desc, cnt, pairs, K, R=None, t=None, gate_px=None, max_distance=256, st=None, cams=None):
    """guided_matches over the last run == the model; the points are the keypoints the indices name"""
    P = len(pairs)
    res = e.fetch_results(P)
    own = R is None
    Rm, tm = (res[0], res[1].reshape(P, 3)) if own else (np.asarray(R), np.asarray(t).reshape(P, 3))
    g = 1.0 if gate_px is None else gate_px
    if cams is None:
        norm1 = norm2 = lambda p, px: gm.normalise_K(px, K)
        thr2 = lambda p: gm.thr2_of(g, gm.focal_K(K))
    else:
        norm1 = lambda p, px: cm.normalise(px, cams[pairs[p][0]])
        norm2 = lambda p, px: cm.normalise(px, cams[pairs[p][1]])
        thr2 = lambda p: gm.thr2_of(g, cm.pair_focal(cams[pairs[p][0]], cams[pairs[p][1]]))
    want = model_run(kps, desc, cnt, pairs, Rm, tm, res[4], thr2, e.max_matches, norm1, norm2, max_distance, own)
    q, ti, d, p1, p2, nm = e.guided_matches(P, R, t, gate_px, max_distance)
    assert_equal_lists((q, ti, d, nm), want, e.max_matches)
    for p, (a, b) in enumerate(pairs):
        n = int(nm[p])
        assert np.array_equal(p1[p, :n, 0], kps[a]["x"][q[p, :n]]) and np.array_equal(p1[p, :n, 1], kps[a]["y"][q[p, :n]]), p
        assert np.array_equal(p2[p, :n, 0], kps[b]["x"][ti[p, :n]]) and np.array_equal(p2[p, :n, 1], kps[b]["y"][ti[p, :n]]), p
        assert not p1[p, n:].any() and not p2[p, n:].any(), p
    return nm, res


def snapshot(e, P, links=None):
    out = list(e.fetch_results(P)) + list(e.fetch_match_indices(P)) + list(e.fetch_structure(P)) + list(e.fetch_matched_points(P))
    if links is not None:
        out += list(e.scale_links(*np.asarray(links, np.int32).T))
    return out


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_stream_and_pair_list(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=6, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    kps, desc, cnt = e.orb_detect_and_compute(frames[:4])
    # stream
    e.estimate_stream(frames[:4], K)
    links = [(0, 1, 1), (1, 2, 1)]
    before = snapshot(e, 3, links)
    nm, res = check_run(e, kps, desc, cnt, [(0, 1), (1, 2), (2, 3)], K)
    assert_same(before, snapshot(e, 3, links))
    print("stream: guided", nm.tolist(), "RANSAC inliers", before[7].sum(1).tolist(), "matches", res[3].tolist())
    assert (nm >= 5).all()
    # pair list: a reversed pair and a self pair
    pairs = [(0, 1), (0, 2), (1, 2), (2, 1), (3, 3), (2, 3)]
    e.frames_reserve(4)
    e.frames_put(frames[:4], [0, 1, 2, 3])
    s1, s2 = np.array(pairs, np.int32).T
    e.estimate_pairs(s1, s2, K)
    links = [(0, 1, 0), (2, 3, 2)]
    before = snapshot(e, 6, links)
    nm, res = check_run(e, kps, desc, cnt, pairs, K)
    assert_same(before, snapshot(e, 6, links))
    print("pair list: guided", nm.tolist(), "RANSAC inliers", before[7].sum(1).tolist(), "matches", res[3].tolist(), "status", res[4].tolist())
    # a wider gate and a distance bound, on the poses of the list given back as a prior
    ok = res[4] == 0
    Rs = np.where(ok[:, None, None], res[0], np.eye(3)); ts = np.where(ok[:, None], res[1].reshape(-1, 3), [1., 0., 0.])
    check_run(e, kps, desc, cnt, pairs, K, R=Rs, t=ts, gate_px=3.0, max_distance=48)
    e.close()


def test_failed_pairs_and_supplied_poses(capi, physics):
    frames, K = physics
    imgs1 = np.stack([frames[0], np.zeros_like(frames[0]), frames[1]]); imgs2 = np.stack([frames[1], np.zeros_like(frames[0]), frames[3]])
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500)
    kps, desc, cnt = e.orb_detect_and_compute(np.concatenate([imgs1, imgs2]))
    R, t, inl, nm0, st = e.estimate_batch(imgs1, imgs2, K)
    assert st[0] == 0 and st[1] != 0 and st[2] == 0
    pairs = [(0, 3), (1, 4), (2, 5)]
    nm, _ = check_run(e, kps, desc, cnt, pairs, K)
    assert nm[1] == 0 and nm[0] > 0 and nm[2] > 0
    # supplied poses: every pair is matched, whatever its status (pair 1 has no keypoints; pair 0 under pair 2's pose)
    Rs = np.stack([R[2], R[0], R[2]]); ts = np.stack([t[2], t[0], t[2]])
    nm2, _ = check_run(e, kps, desc, cnt, pairs, K, R=Rs, t=ts, gate_px=2.0)
    assert nm2[1] == 0 and nm2[2] > 0
    e.close()


def test_cameras(capi, physics):
    frames, K = physics
    pairs = [(0, 1), (1, 2), (2, 0)]
    s1, s2 = np.array(pairs, np.int32).T
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500)
    kps, desc, cnt = e.orb_detect_and_compute(frames[:3])
    e.frames_reserve(3)
    e.frames_put(frames[:3], [0, 1, 2])
    # single K, then pinhole cameras: the same bits
    e.estimate_pairs(s1, s2, K)
    gk = e.guided_matches(3)
    e.frames_set_cameras([0, 1, 2], capi.Camera(K))
    e.estimate_pairs_cameras(s1, s2)
    assert_same(gk, e.guided_matches(3))
    # a lens on slot 1 and another focal length on slot 2
    K2 = K.copy(); K2[0, 0] *= 1.02; K2[1, 1] *= 1.02
    dist = [-0.08, 0.02, 0.001, -0.0005]
    e.frames_set_cameras([0, 1, 2], [capi.Camera(K), capi.Camera(K, dist), capi.Camera(K2)])
    e.estimate_pairs_cameras(s1, s2)
    cams = [cm.Cam(K), cm.Cam(K, dist), cm.Cam(K2)]
    nm, _ = check_run(e, kps, desc, cnt, pairs, K, cams=cams)
    print("cameras: guided", nm.tolist())
    e.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500)
    e.frames_reserve(2)
    e.estimate_stream(frames[:3], K)
    good = e.guided_matches(2)
    assert good[5].min() > 0
    R, t = e.fetch_results(2)[:2]
    Rn = R.copy(); Rn[1, 2, 2] = np.nan
    lib, h = e.lib, e.h
    Rc = np.ascontiguousarray(R.reshape(2, 9)); tc = np.ascontiguousarray(t.reshape(2, 3)); Rnc = np.ascontiguousarray(Rn.reshape(2, 9))
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    raw = lambda B, R_, t_, gate, md: lib.rpe_guided_matches(h, B, R_, t_, gate, md, None, None, None, None, None, None)
    assert raw(2, None, None, 1.0, 256) == 0
    for args in ((3, None, None, 1.0, 256),                     # more pairs than the run
                 (2, None, None, 0.0, 256), (2, None, None, -1.0, 256), (2, None, None, float("nan"), 256), (2, None, None, float("inf"), 256),
                 (2, None, None, 1.0, 257), (2, None, None, 1.0, -1),
                 (2, p(Rnc), p(tc), 1.0, 256),                  # a NaN in R
                 (2, p(Rc), None, 1.0, 256), (2, None, p(tc), 1.0, 256)):
        assert raw(*args) == -1, args
        assert_same(good, e.guided_matches(2))
    # after a put the workspace holds other features
    e.frames_put(frames[3:4], [0])
    assert raw(2, None, None, 1.0, 256) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.guided_matches(2))
    # after a stage call
    e.match_hamming([np.zeros((1, 32), np.uint8)], [1], [np.zeros((1, 32), np.uint8)], [1])
    assert raw(2, None, None, 1.0, 256) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.guided_matches(2))
    # once the store was resized under a pair list
    e.frames_put(frames[:2], [0, 1])
    e.estimate_pairs([0], [1], K)
    assert raw(1, None, None, 1.0, 256) == 0
    e.frames_reserve(3)
    assert raw(1, None, None, 1.0, 256) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.guided_matches(2))
    e.close()
    # an L2 handle
    e2 = capi.Engine(640, 480, max_batch=1, nfeatures=500, max_matches=200, norm_type=capi.NORM_L2)
    r0 = e2.estimate_batch(frames[:1], frames[1:2], K)
    with pytest.raises(capi.RpeError, match="Hamming handles only"):
        e2.guided_matches(1)
    assert_same(r0, e2.fetch_results(1))
    e2.close()


# ------------------------------------------------------------------ 9. the drop-in
def test_estimate_guided(physics):
    from relative_pose_estimation_amd import PoseEstimator
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=1000, max_matches=500)
    a = pe.estimate_guided(frames[0], frames[1])
    assert np.isfinite(a['R']).all() and np.isfinite(a['t']).all()
    assert abs(np.linalg.norm(a['t']) - 1) <= 1e-12 and abs(np.linalg.det(a['R']) - 1) <= 1e-12
    assert a['num_guided'] >= 5 and len(a['pts1']) == a['num_guided']
    b = pe.estimate_guided(frames[0], frames[1])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    print("estimate_guided: guided", a['num_guided'], "code", a['refine_code'], "rms", a['rms_before'], a['rms_after'])
    pe.close()
