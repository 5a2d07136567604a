"""Guided matching for NORM_L2 handles on the GPU (rpe_guided_matches_l2 / rpe_match_l2_guided, through the C-ABI) against
the model (tests/guided_l2_model.py).  Equality is exact: indices with array_equal, distances on their bits, -1 and
all-ones bits past each pair's count.  The stage form runs the L2 descriptor cases of tests/match_cases.py with the
keypoints, pose and 1 px gate of the model module, on engines of the sizes that reach each launch form of the tile kernel
(match_l2_guided_mfma_kernel<4 | 1>); the run form covers a SIFT stream, a pair list (the table instances), ORB bytes
under L2, cameras with a lens, a ratio-mode handle, failed pairs, supplied poses and the refusals, and checks that the
call changes nothing of the run it reads."""
import math

import numpy as np
import pytest

from tests import camera_model as cm
from tests import guided_l2_model as g2
from tests import guided_model as gm
from tests import match_cases as mc
from tests import scale_model as sc

pytestmark = pytest.mark.gpu

ONES = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_lists(got, want):
    """got: (qidx, tidx, dist, n_matches) of a call; want: per pair the model's (qidx, tidx, dist)"""
    q, ti, d, nm = got
    for p, (mq, mt, md) in enumerate(want):
        n = len(mq)
        assert nm[p] == n, (p, int(nm[p]), n)
        assert np.array_equal(q[p, :n], mq) and np.array_equal(ti[p, :n], mt), p
        assert np.array_equal(bits(d[p, :n]), bits(md)), p
        assert (q[p, n:] == -1).all() and (ti[p, n:] == -1).all() and (bits(d[p, n:]) == ONES).all(), p


# ------------------------------------------------------------------ the stage form on the descriptor cases
def l2_form(kcap, B):
    """the tile kernels' grid: (gridDim.x, gridDim.y)"""
    chunks = (kcap + 127) // 128
    return chunks, min(8, max(1, (1024 + chunks * 2 * B - 1) // (chunks * 2 * B)))


def engine(capi, list_name, nfeatures, max_batch, **kw):
    spec = mc.SPECS[list_name]
    if spec.dim == 128:
        kw["feature_method"] = capi.FEATURE_SIFT
    kw.setdefault("max_matches", spec.max_matches)
    e = capi.Engine(96, 96, max_batch=max_batch, nfeatures=nfeatures, norm_type=capi.NORM_L2, **kw)
    assert e.desc_dim == spec.dim and e.kcap == (nfeatures or 16320) + 64
    return e


def run_stage(e, list_name, group, gate_px=g2.GATE_PX, max_distance=None):
    R, t = g2.pose()
    B = len(group)
    pts = [g2.keypoints(c.name, list_name) for c in group]
    return e.match_l2_guided([c.desc1.astype(np.float32) for c in group], [p[0] for p in pts], [len(c.desc1) for c in group],
                             [c.desc2.astype(np.float32) for c in group], [p[1] for p in pts], [len(c.desc2) for c in group],
                             g2.camera_K(), np.tile(R, (B, 1, 1)), np.tile(t, (B, 1)), gate_px, max_distance)


# list -> (nfeatures, max_batch of the engine, pairs per call, the grid that call must take)
STAGE = {
    "l2_sift_448": (448, 4, 1, (4, 8)), "l2_orb_448": (448, 4, 1, (4, 8)),
    "l2_sift_1984_ring": (1984, 32, 32, (16, 1)), "l2_orb_1984_ring": (1984, 32, 32, (16, 1)),
    "l2_sift_1984_full": (1984, 1, 1, (16, 8)),
    "l2_sift_uncapped": (0, 1, 1, (128, 4)),
}


@pytest.mark.parametrize("list_name", g2.LISTS)
def test_stage_form(capi, list_name):
    """1. every case of the six lists: owners 127 / 128 / 129, scanned tiles dealt over 8 workgroups (448), 1 .. 6 tiles
    through the 3-deep ring, empty sides and 1 x 1 in a batch of 32 (ring), 8 chunks of 8 tiles (full), the 128 KB select
    and indices beyond 8191 (uncapped); squared distances beyond 2^22 in the far cases"""
    nf, mb, per_call, form = STAGE[list_name]
    e = engine(capi, list_name, nf, mb)
    try:
        assert l2_form(e.kcap, per_call) == form
        cs = list(mc.cases(list_name))
        if per_call == 32:
            cs = (cs + cs[::-1])[:32]
        for s in range(0, len(cs), per_call):
            group = cs[s:s + per_call]
            assert_lists(run_stage(e, list_name, group), [g2.expected(c.name, list_name) for c in group])
    finally:
        e.close()


@pytest.fixture(scope="module", params=["l2_sift_448", "l2_orb_448"])
def eng448(capi, request):
    e = engine(capi, request.param, 448, 4)
    yield e, request.param
    e.close()


def test_open_gate_equals_match_l2(eng448):
    """2. gate_px = 1e9 and no bound: the crossCheck result of rpe_match_l2 on the same handle, bit for bit"""
    e, name = eng448
    total = 0
    for c in mc.cases(name):
        g = run_stage(e, name, [c], 1e9, None)
        m = e.match_l2([c.desc1.astype(np.float32)], [len(c.desc1)], [c.desc2.astype(np.float32)], [len(c.desc2)])
        n = int(m[3][0])
        total += n
        assert g[3][0] == n, c.name
        assert np.array_equal(g[0][0, :n], m[0][0, :n]) and np.array_equal(g[1][0, :n], m[1][0, :n]), c.name
        assert np.array_equal(bits(g[2][0, :n]), bits(m[2][0, :n])), c.name
    assert total > 100


@pytest.mark.parametrize("n1,n2,kind", [(512, 512, "mixed"), (288, 288, "far")])
def test_distance_bound(eng448, n1, n2, kind):
    """3. max_distance = the median of the case's unbounded guided distances, and 0: only equal rows survive"""
    e, name = eng448
    c = mc.case(name, n1, n2, kind)
    full = g2.expected(c.name, name, math.inf, None)
    assert len(full[0]) > 10
    med = float(np.median(full[2]))
    want = g2.expected(c.name, name, med)
    assert 0 < len(want[0]) and (want[2] <= med).all()
    assert_lists(run_stage(e, name, [c], max_distance=med), [want])
    zero = g2.expected(c.name, name, 0.0)
    assert (len(zero[0]) > 0) == (kind == "mixed") and not zero[2].any()
    assert_lists(run_stage(e, name, [c], max_distance=0.0), [zero])


@pytest.mark.parametrize("list_name", ["l2_sift_448", "l2_orb_448"])
def test_truncation_keeps_the_head_of_the_sorted_list(capi, list_name):
    """4. max_matches = 7, far below the guided count"""
    c = mc.case(list_name, 512, 512)
    full = g2.expected(c.name, list_name, math.inf, None)
    assert len(full[0]) > 100
    e = engine(capi, list_name, 448, 1, max_matches=7)
    try:
        assert_lists(run_stage(e, list_name, [c]), [tuple(a[:7] for a in full)])
    finally:
        e.close()


# ------------------------------------------------------------------ 5. the run form
def patch_frame(img, size):
    """a flat image that keeps a size x size window of img: a handful of keypoints, too few matches for a pose"""
    out = np.full_like(img, 128)
    out[200:200 + size, 300:300 + size] = img[200:200 + size, 300:300 + size]
    return out


def model_run(px, desc, cnt, pairs, R, t, st, thr2, mm, norm1, norm2, bound, own_poses):
    out = []
    for p, (a, b) in enumerate(pairs):
        if own_poses and st[p] != 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)))
            continue
        out.append(g2.guided_match(desc[a][:cnt[a]], norm1(p, px[a][:cnt[a]]), desc[b][:cnt[b]], norm2(p, px[b][:cnt[b]]),
                                   R[p], t[p], thr2(p), bound, mm))
    return out


def check_run(e, kps, desc, cnt, pairs, K, R=None, t=None, gate_px=None, max_distance=None, cams=None):
    """guided_matches_l2 over the last run == the model; the points are the keypoints the indices name; every fetch of
    the run returns the same bits afterwards.  Returns the counts, the run's results and the distances"""
    P = len(pairs)
    before = snapshot(e, P)
    res = before[:5]
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
    px = [np.stack([k["x"], k["y"]], 1) for k in kps]
    bound = math.inf if max_distance is None else max_distance
    want = model_run(px, desc, cnt, pairs, Rm, tm, res[4], thr2, e.max_matches, norm1, norm2, bound, own)
    q, ti, d, p1, p2, nm = e.guided_matches_l2(P, R, t, gate_px, max_distance)
    assert d.dtype == np.float32
    assert_lists((q, ti, d, nm), want)
    for p, (a, b) in enumerate(pairs):
        n = int(nm[p])
        assert np.array_equal(p1[p, :n], px[a][q[p, :n]]) and np.array_equal(p2[p, :n], px[b][ti[p, :n]]), p
        assert not p1[p, n:].any() and not p2[p, n:].any(), p
    assert_same(before, snapshot(e, P))
    return nm, res, d


def snapshot(e, P):
    return list(e.fetch_results(P)) + list(e.fetch_structure(P)) + list(e.fetch_match_indices(P)) + list(e.fetch_matched_points(P))


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def own_then_supplied(e, kps, desc, cnt, pairs, K, good, failed, cams=None):
    """the run's own poses (the failed pair gets nothing although both its images have keypoints), then the good pair's
    pose supplied for every pair under a 10 px gate and a distance bound: the failed pair is matched too"""
    a, b = pairs[failed]
    assert cnt[a] > 0 and cnt[b] > 0
    nm, res, _ = check_run(e, kps, desc, cnt, pairs, K, cams=cams)
    st = res[4]
    assert st[good] == 0 and st[failed] != 0 and nm[good] > 0 and nm[failed] == 0, (st, nm)
    P = len(pairs)
    Rs = np.tile(res[0][good], (P, 1, 1)); ts = np.tile(res[1][good].reshape(3), (P, 1))
    nm2, _, d = check_run(e, kps, desc, cnt, pairs, K, R=Rs, t=ts, gate_px=10.0, cams=cams)
    assert nm2[failed] > 0 and nm2[good] > 0, (nm, nm2)
    check_run(e, kps, desc, cnt, pairs, K, R=Rs, t=ts, gate_px=10.0, max_distance=float(np.median(d[good, :nm2[good]])), cams=cams)
    return nm, nm2


@pytest.fixture(scope="module")
def sift_run(capi, physics):
    """a SIFT engine, four frames -- two of the stream and two patch frames -- and their features"""
    frames, K = physics
    four = np.stack([frames[0], frames[1], patch_frame(frames[1], 24), patch_frame(frames[2], 24)])
    e = capi.Engine(640, 480, max_batch=3, nfeatures=600, max_matches=300, feature_method=capi.FEATURE_SIFT, norm_type=capi.NORM_L2)
    kps, desc, cnt = e.sift_detect_and_compute(four)
    yield e, four, K, kps, desc, cnt
    e.close()


def test_sift_stream(sift_run):
    e, four, K, kps, desc, cnt = sift_run
    e.estimate_stream(four, K)
    nm, nm2 = own_then_supplied(e, kps, desc, cnt, [(0, 1), (1, 2), (2, 3)], K, good=0, failed=2)
    print("SIFT stream: guided", nm.tolist(), "under pair 0's pose at 10 px", nm2.tolist())


def test_sift_pair_list_from_the_frame_store(sift_run):
    """the table instances (TAB): a reversed pair and the failed pair in the middle of the list"""
    e, four, K, kps, desc, cnt = sift_run
    pairs = [(1, 0), (2, 3), (0, 1)]
    e.frames_reserve(4)
    e.frames_put(four, [0, 1, 2, 3])
    s1, s2 = np.array(pairs, np.int32).T
    e.estimate_pairs(s1, s2, K)
    nm, nm2 = own_then_supplied(e, kps, desc, cnt, pairs, K, good=2, failed=1)
    print("SIFT pair list: guided", nm.tolist(), "under pair 2's pose at 10 px", nm2.tolist())


def test_sift_cameras_with_a_lens(capi, sift_run):
    """the CAM records: a lens on slots 1 and 3 and another focal length on slot 2"""
    e, four, K, kps, desc, cnt = sift_run
    pairs = [(0, 1), (2, 3), (1, 0)]
    K2 = K.copy(); K2[0, 0] *= 1.02; K2[1, 1] *= 1.02
    dist = [-0.08, 0.02, 0.001, -0.0005]
    e.frames_reserve(4)
    e.frames_put(four, [0, 1, 2, 3])
    e.frames_set_cameras([0, 1, 2, 3], [capi.Camera(K), capi.Camera(K, dist), capi.Camera(K2), capi.Camera(K, dist)])
    s1, s2 = np.array(pairs, np.int32).T
    e.estimate_pairs_cameras(s1, s2)
    cams = [cm.Cam(K), cm.Cam(K, dist), cm.Cam(K2), cm.Cam(K, dist)]
    nm, nm2 = own_then_supplied(e, kps, desc, cnt, pairs, K, good=0, failed=1, cams=cams)
    print("SIFT cameras: guided", nm.tolist(), "under pair 0's pose at 10 px", nm2.tolist())


def test_orb_bytes_under_l2(capi, physics):
    """KS = 1: a batch of an ORB + NORM_L2 handle"""
    frames, K = physics
    imgs1 = np.stack([frames[0], patch_frame(frames[1], 6), frames[1]]); imgs2 = np.stack([frames[1], patch_frame(frames[2], 6), frames[3]])
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500, norm_type=capi.NORM_L2)
    try:
        kps, desc, cnt = e.orb_detect_and_compute(np.concatenate([imgs1, imgs2]))
        e.estimate_batch(imgs1, imgs2, K)
        nm, nm2 = own_then_supplied(e, kps, desc, cnt, [(0, 3), (1, 4), (2, 5)], K, good=0, failed=1)
        print("ORB + L2 batch: guided", nm.tolist(), "under pair 0's pose at 10 px", nm2.tolist())
    finally:
        e.close()


# ------------------------------------------------------------------ 6. a ratio-mode handle
def test_ratio_mode_handle(capi, physics):
    """the run's matcher was the Lowe-ratio kernel, which writes no norm words: the guided launch computes its own"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=2, nfeatures=1000, max_matches=500, norm_type=capi.NORM_L2,
                    match_mode=capi.MATCH_RATIO, match_ratio=0.8)
    try:
        kps, desc, cnt = e.orb_detect_and_compute(frames[:3])
        # a stage call first: whatever norm words an earlier run left belong to other descriptors
        e.match_l2([np.full((3, 32), 7, np.float32)], [3], [np.full((2, 32), 9, np.float32)], [2])
        res = e.estimate_stream(frames[:3], K)
        assert (res[4] == 0).all()
        nm, _, _ = check_run(e, kps, desc, cnt, [(0, 1), (1, 2)], K)
        assert (nm > 5).all()
        print("ratio-mode ORB + L2 stream: guided", nm.tolist(), "ratio matches", res[3].tolist())
    finally:
        e.close()


def test_ratio_mode_pair_list_from_the_frame_store(capi, physics):
    """the table instances on a ratio-mode handle: the slots' norm words come from the put, although the handle's own
    matcher never reads them.  A reversed pair; the run's own poses, then pair 0's pose for both pairs"""
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=2, nfeatures=1000, max_matches=500, norm_type=capi.NORM_L2,
                    match_mode=capi.MATCH_RATIO, match_ratio=0.8)
    try:
        kps, desc, cnt = e.orb_detect_and_compute(frames[:3])
        e.frames_reserve(2)
        e.frames_put(frames[:2], [0, 1])
        e.frames_reserve(3)                                        # growing keeps the slots' words
        e.frames_put(frames[2:3], [2])
        pairs = [(1, 0), (0, 2)]
        s1, s2 = np.array(pairs, np.int32).T
        res = e.estimate_pairs(s1, s2, K)
        assert (res[4] == 0).all()
        nm, _, _ = check_run(e, kps, desc, cnt, pairs, K)
        assert (nm > 5).all()
        Rs = np.tile(res[0][0], (2, 1, 1)); ts = np.tile(res[1][0].reshape(3), (2, 1))
        nm2, _, _ = check_run(e, kps, desc, cnt, pairs, K, R=Rs, t=ts, gate_px=10.0)
        assert (nm2 > 0).all()
        print("ratio-mode ORB + L2 pair list: guided", nm.tolist(), "under pair 0's pose at 10 px", nm2.tolist(), "ratio matches", res[3].tolist())
    finally:
        e.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable(capi, physics):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=1000, max_matches=500, norm_type=capi.NORM_L2)
    e.frames_reserve(2)
    e.estimate_stream(frames[:3], K)
    good = e.guided_matches_l2(2)
    results = snapshot(e, 2)
    assert good[5].min() > 0
    R, t = e.fetch_results(2)[:2]
    Rn = R.copy(); Rn[1, 2, 2] = np.nan
    ti = t.copy().reshape(2, 3); ti[0, 1] = np.inf
    lib, h = e.lib, e.h
    Rc = np.ascontiguousarray(R.reshape(2, 9)); tc = np.ascontiguousarray(t.reshape(2, 3)); Rnc = np.ascontiguousarray(Rn.reshape(2, 9))
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    raw = lambda B, R_, t_, gate, md: lib.rpe_guided_matches_l2(h, B, R_, t_, gate, md, None, None, None, None, None, None)
    inf = float("inf")
    assert raw(2, None, None, 1.0, inf) == 0 and raw(2, None, None, 1.0, 0.0) == 0
    for args in ((3, None, None, 1.0, inf),                     # more pairs than the run
                 (2, None, None, 0.0, inf), (2, None, None, -1.0, inf), (2, None, None, float("nan"), inf), (2, None, None, inf, inf),
                 (2, None, None, 1.0, -1.0), (2, None, None, 1.0, float("nan")), (2, None, None, 1.0, -inf),
                 (2, p(Rnc), p(tc), 1.0, inf), (2, p(Rc), p(ti), 1.0, inf),     # a NaN in R, an infinity in t
                 (2, p(Rc), None, 1.0, inf), (2, None, p(tc), 1.0, inf)):
        assert raw(*args) == -1, args
        assert_same(good, e.guided_matches_l2(2))
    assert_same(results, snapshot(e, 2))
    # the stage form refuses the same arguments before it touches the workspace: the run is still there
    d = [np.zeros((1, 32), np.float32)]; x = [np.zeros((1, 2), np.float32)]
    for kw in (dict(gate_px=0.0), dict(max_distance=-1.0), dict(max_distance=float("nan"))):
        with pytest.raises(capi.RpeError, match="rpe_match_l2_guided"):
            e.match_l2_guided(d, x, [1], d, x, [1], K, R[:1], t[:1], **kw)
    with pytest.raises(capi.RpeError, match="non-finite"):
        e.match_l2_guided(d, x, [1], d, x, [1], K, Rn[1:], t[:1])
    with pytest.raises(capi.RpeError, match="byte-valued"):
        e.match_l2_guided([np.full((1, 32), 0.5, np.float32)], x, [1], d, x, [1], K, R[:1], t[:1])
    assert_same(good, e.guided_matches_l2(2))
    # after a put the workspace holds other features
    e.frames_put(frames[3:4], [0])
    assert raw(2, None, None, 1.0, inf) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.guided_matches_l2(2))
    # after a stage call, the guided one included
    e.match_l2(d, [1], d, [1])
    assert raw(2, None, None, 1.0, inf) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.guided_matches_l2(2))
    e.match_l2_guided(d, x, [1], d, x, [1], K, R[:1], t[:1])
    assert raw(2, None, None, 1.0, inf) == -1
    e.estimate_stream(frames[:3], K)
    assert_same(good, e.guided_matches_l2(2))
    assert_same(results, snapshot(e, 2))
    e.close()


def test_refused_for_hamming_handles_and_chunked_batches(capi, K_vga):
    from relative_pose_estimation_amd import geometry, synthetic
    # a Hamming handle through the new calls
    i1, i2, _, _ = synthetic.make_batch(1, K_vga, cfg=2)
    e = capi.Engine(640, 480, max_batch=1, nfeatures=500, max_matches=200)
    r0 = e.estimate_batch(i1, i2, K_vga)
    with pytest.raises(capi.RpeError, match="L2 handles only"):
        e.guided_matches_l2(1)
    with pytest.raises(capi.RpeError, match="L2 handles only"):
        e.match_l2_guided([np.zeros((1, 32), np.float32)], [np.zeros((1, 2), np.float32)], [1], [np.zeros((1, 32), np.float32)],
                          [np.zeros((1, 2), np.float32)], [1], K_vga, r0[0], r0[1])
    assert_same(r0, e.fetch_results(1))
    assert e.guided_matches(1)[5][0] > 0
    e.close()
    # a host batch that ran in chunks (512 pairs, 64 MiB per image set) leaves no per-match data
    W, H, B = 512, 256, 512
    K = geometry.default_camera_matrix(W, H)
    i1, i2, _, _ = synthetic.make_batch(2, K, W, H, cfg=2)
    a = np.ascontiguousarray(np.concatenate([i1] * (B // 2))); b = np.ascontiguousarray(np.concatenate([i2] * (B // 2)))
    e = capi.Engine(W, H, max_batch=B, nfeatures=300, max_matches=100, norm_type=capi.NORM_L2)
    host = e.estimate_batch(a, b, K)
    with pytest.raises(capi.RpeError, match="ran in chunks"):
        e.guided_matches_l2(2)
    dev = e.estimate_batch_device(e.upload(a[:2]), e.upload(b[:2]), 2, K)
    assert_same([x[:2] for x in host], dev)
    nm = e.guided_matches_l2(2)[5]
    assert ((nm > 0) | (dev[4] != 0)).all()
    e.close()


# ------------------------------------------------------------------ 8. the drop-in
def test_estimate_guided_sift(capi, physics):
    from relative_pose_estimation_amd import PoseEstimator
    frames, K = physics
    pe = PoseEstimator(K, feature_method="SIFT", norm_type="L2", nfeatures=600, max_matches=300)
    a = pe.estimate_guided(frames[0], frames[1])
    assert a['num_guided'] > 0 and len(a['pts1']) == len(a['pts2']) == a['num_guided']
    assert a['refine_code'] in (capi.REFINE_OK, capi.REFINE_SKIPPED, capi.REFINE_REJECTED)
    assert np.isfinite(a['R']).all() and np.isfinite(a['t']).all()
    R0, t0 = pe.estimate(frames[0], frames[1])
    assert np.array_equal(R0, a['R_initial']) and np.array_equal(t0, a['t_initial'])
    g = pe.last_guided()[0]
    assert g['dist'].dtype == np.float32 and (np.diff(g['dist']) >= 0).all()
    assert np.array_equal(g['pts1'], a['pts1']) and np.array_equal(g['pts2'], a['pts2'])
    bounded = pe.last_guided(max_distance=float(np.median(g['dist'])))[0]
    assert len(bounded['qidx']) > 0 and (bounded['dist'] <= np.median(g['dist'])).all()
    print("estimate_guided SIFT: guided", a['num_guided'], "code", a['refine_code'], "rms", a['rms_before'], a['rms_after'])
    pe.close()
    # ORB + NORM_L2 dispatches the same way
    pe = PoseEstimator(K, norm_type="L2", nfeatures=1000, max_matches=500)
    b = pe.estimate_guided(frames[0], frames[1])
    pe.estimate(frames[0], frames[1])                          # the refinement was a stage call: a run again
    g = pe.last_guided()[0]
    assert b['num_guided'] > 0 and g['dist'].dtype == np.float32 and np.array_equal(g['pts1'], b['pts1'])
    pe.close()
