"""Frame store and pair lists (rpe_frames_* / rpe_enqueue_pairs, through the C-ABI): the result of pair (a, b) is bit
for bit what rpe_estimate_batch_device returns for the frame put into slot a against the frame put into slot b --
whatever the position in the list, the list length, the slot numbers and whatever ran on the handle in between.
Every comparison is np.array_equal on the raw bits (doubles viewed as uint64); nothing here has a tolerance except
the comparison with the CPU oracle, which is the one tests/test_gpu_parity.py makes for batches."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_RT = 1e-4   # oracle comparison only: tests/test_gpu_parity.py test_end_to_end_parity

# the 21 pairs: (i, i + d) for d = 1, 2, 3, two reversed pairs and a self pair
WINDOW = [(i, i + d) for d in (1, 2, 3) for i in range(8 - d)] + [(3, 0), (7, 4), (2, 2)]


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def frames(K_vga):
    from relative_pose_estimation_amd import synthetic
    return synthetic.make_stream(8, K_vga)[0]


@pytest.fixture(scope="module")
def eng(capi):
    e = capi.Engine(640, 480, max_batch=24, nfeatures=1000, max_matches=500)
    yield e
    e.close()


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b, what=""):
    """two (R, t, inliers, n_matches, status) tuples, bit for bit"""
    for k, (x, y) in enumerate(zip(a, b)):
        if x.dtype == np.float64:
            x, y = _u64(x), _u64(y)
        assert np.array_equal(x, y), (what, "field", k, np.nonzero(np.asarray(x != y).reshape(len(x), -1).any(axis=1))[0])


def _batch(e, imgs, pairs, K, after=None):
    """rpe_estimate_batch_device on the gathered image pairs (the images resident in HBM); after(e, B) runs before the
    image buffers are released"""
    pairs = np.asarray(pairs)
    d1 = e.upload(imgs[pairs[:, 0]]); d2 = e.upload(imgs[pairs[:, 1]])
    try:
        res = e.estimate_batch_device(d1, d2, len(pairs), K)
        extra = after(e, len(pairs)) if after else None
    finally:
        e.synchronize()
        e.device_free(d1); e.device_free(d2)
    return (res, extra) if after else res


def _pairs(e, pairs, K):
    pairs = np.asarray(pairs)
    return e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)


@pytest.fixture(scope="module")
def ref(eng, frames, K_vga):
    """the batch path on the 21 gathered pairs"""
    return _batch(eng, frames, WINDOW, K_vga)


@pytest.fixture()
def store8(eng, frames):
    """frames 0..7 in slots 0..7 of an 8-slot store, put once"""
    eng.frames_reserve(0)
    eng.frames_reserve(8)
    eng.frames_put(frames, np.arange(8))
    return eng


def test_window_list_equals_batches_and_oracle(store8, frames, ref, oracle, K_vga):
    res = _pairs(store8, WINDOW, K_vga)
    R, t, inl, nm, st = res
    print("status", st.tolist(), "n_matches", nm.tolist(), "inliers", inl.tolist())
    assert list(st) == [0] * 21 and (nm >= 490).all(), (st, nm)      # not an empty comparison
    _same(res, ref, "pair list vs batch")
    w = np.asarray(WINDOW)
    o = oracle.estimate_pose_batch(frames[w[:, 0]], frames[w[:, 1]], K_vga, 1000, 500, nthreads=8)
    for p in range(21):
        assert st[p] == o["status"][p] and nm[p] == o["n_matches"][p] and inl[p] == o["inliers"][p], (p, st[p], nm[p], inl[p], o["status"][p], o["n_matches"][p], o["inliers"][p])
        dR = np.linalg.norm(R[p] - o["R"][p].reshape(3, 3)); dt = np.linalg.norm(t[p] - o["t"][p].reshape(3, 1))
        print(p, WINDOW[p], "dR", dR, "dt", dt)
        assert dR <= TOL_RT and dt <= TOL_RT, (p, dR, dt)
    cnt, fl = store8.frames_info(np.arange(8))
    assert (cnt > 0).all() and not fl.any()


def test_stream_equivalence(store8, frames, K_vga):
    res = _pairs(store8, [(i, i + 1) for i in range(7)], K_vga)
    _same(res, store8.estimate_stream(frames, K_vga), "pair list vs stream")


def test_persistence_and_replacement(store8, frames, ref, K_vga):
    from relative_pose_estimation_amd import synthetic
    e = store8
    i1, i2, _, _ = synthetic.make_batch(3, K_vga, cfg=2)
    e.estimate_batch(i1, i2, K_vga)                       # an unrelated batch
    e.orb_detect_and_compute(np.concatenate([i1, i2]))    # a stage call over six workspace slots
    e.estimate_batch(i1, i2, K_vga)
    e.refine_poses(3, 10)
    _same(_pairs(e, WINDOW, K_vga), ref, "after unrelated calls")
    # another frame into slot 5: pairs touching the slot become that frame's batch result, all others keep their bits
    e.frames_put(i1[:1], [5])
    res = _pairs(e, WINDOW, K_vga)
    changed = frames.copy(); changed[5] = i1[0]
    want = _batch(e, changed, WINDOW, K_vga)
    _same(res, want, "after replacing slot 5")
    keep = np.array([5 not in p for p in WINDOW])
    assert keep.sum() == 16
    _same([x[keep] for x in res], [x[keep] for x in ref], "pairs that do not touch slot 5")


def test_slot_numbers_do_not_matter(eng, frames, ref, K_vga):
    e = eng
    e.frames_reserve(0)
    e.frames_reserve(64)
    assert e.frames_capacity() == 64
    slots = np.array([13, 2, 9, 0, 15, 7, 11, 4])            # frame f lives in slots[f]; all below 16
    d = e.upload(frames)
    try:
        # two puts of unequal size, frames resident in HBM, in an order that is not the frame order
        e.frames_put_device(C.c_void_p(d.value + 3 * 480 * 640), 5, slots[3:])
        e.frames_put_device(d, 3, slots[:3])
        e.synchronize()
    finally:
        e.device_free(d)
    w = slots[np.asarray(WINDOW)]
    _same(_pairs(e, w, K_vga), ref, "scattered slots")
    cnt64, _ = e.frames_info(np.arange(64))
    assert (cnt64[slots] > 0).all() and (np.delete(cnt64, slots) == -1).all()
    e.frames_reserve(128)
    assert e.frames_capacity() == 128
    cnt, _ = e.frames_info(np.arange(128))
    assert np.array_equal(cnt[:64], cnt64) and (cnt[64:] == -1).all()
    _same(_pairs(e, w, K_vga), ref, "after growing to 128")
    e.frames_reserve(16)
    assert e.frames_capacity() == 16
    cnt, _ = e.frames_info(np.arange(16))
    assert np.array_equal(cnt, cnt64[:16])
    _same(_pairs(e, w, K_vga), ref, "after shrinking to 16")


def _last_batch_views(e, B):
    p1, p2 = e.fetch_matched_points(B)
    rm, pm, pts = e.fetch_structure(B)
    rR, rt, rinl, rinfo, rrms = e.refine_poses(B, 10)
    ov = e.fetch_overflow(B)
    return [p1.view(np.uint32), p2.view(np.uint32), rm, pm, _u64(pts), _u64(rR), _u64(rt), rinl, rinfo, _u64(rrms), ov]


def test_everything_behind_the_last_batch(store8, frames, K_vga):
    e = store8
    _, want = _batch(e, frames, WINDOW, K_vga, after=_last_batch_views)
    w = np.asarray(WINDOW)
    e.enqueue_pairs(w[:, 0], w[:, 1], K_vga)
    got = _last_batch_views(e, 21)
    names = ["pts1", "pts2", "ransac_mask", "pose_mask", "points", "refined R", "refined t", "refined inliers", "refine info",
             "refine rms", "overflow"]
    for n, a, b in zip(names, got, want):
        assert np.array_equal(a, b), n
    assert got[2].any() and got[3].any() and (got[8][:, 0] == 0).any()     # masks are set, some pair was refined


SHORT = [(0, 1), (0, 2), (1, 3), (2, 1), (3, 3), (0, 3)]


@pytest.mark.parametrize("name,W,H,kw", [
    ("orb_l2", 640, 480, dict(nfeatures=1000, norm_type=1)),
    ("sift_512", 320, 240, dict(nfeatures=512, feature_method=1, norm_type=1)),
    ("sift_uncapped", 320, 240, dict(nfeatures=0, feature_method=1, norm_type=1)),
    ("orb_ratio", 640, 480, dict(nfeatures=1000, match_mode=1)),
    ("orb_l2_ratio", 640, 480, dict(nfeatures=1000, norm_type=1, match_mode=1)),
    ("sift_ratio", 320, 240, dict(nfeatures=512, feature_method=1, norm_type=1, match_mode=1)),
    ("orb_msvc", 640, 480, dict(nfeatures=1000, stl_runtime=1)),
    ("orb_848x478", 848, 478, dict(nfeatures=1000)),
    ("orb_odd_capacity", 640, 480, dict(nfeatures=777)),
])
def test_other_configurations(capi, name, W, H, kw):
    from relative_pose_estimation_amd import synthetic, geometry
    K = geometry.default_camera_matrix(W, H)
    fr = synthetic.make_stream(4, K, W, H)[0]
    e = capi.Engine(W, H, max_batch=8, max_matches=500, **kw)
    try:
        e.frames_reserve(6)
        e.frames_put(fr, [4, 0, 5, 2])
        w = np.array([4, 0, 5, 2])[np.asarray(SHORT)]
        res = _pairs(e, w, K)
        print(name, "status", res[4].tolist(), "n_matches", res[3].tolist(), "inliers", res[2].tolist())
        assert (res[3] > 0).all(), "the configuration matched nothing: empty comparison"
        _same(res, _batch(e, fr, SHORT, K), name)
        _same(_pairs(e, w, K), res, name + " again, after a batch")
    finally:
        e.close()


def test_fused_matcher_with_a_table(capi, frames, ref, K_vga):
    """more than RPE_MATCH_SPLIT_PAIRS (64) pairs in one list: the fused Hamming matcher (election words in LDS, in-kernel
    sort and point gather) instead of the split form every shorter list takes -- scattered slots, an 80-pair engine"""
    e = capi.Engine(640, 480, max_batch=80, nfeatures=1000, max_matches=500)
    try:
        slots = np.array([13, 2, 9, 0, 15, 7, 11, 4])
        e.frames_reserve(16)
        e.frames_put(frames, slots)
        lst = (WINDOW * 4)[:80]                              # 80 pairs: the window list three times and 17 more
        lst = lst[5:] + lst[:5]                              # not aligned with the repetition
        assert len(lst) == 80 > 64
        res = _pairs(e, slots[np.asarray(lst)], K_vga)
        assert (res[4] == 0).all() and (res[3] >= 490).all()
        _same(res, _batch(e, frames, lst, K_vga), "80-pair list vs 80-pair batch")
        idx = [WINDOW.index(p) for p in lst]
        _same(res, [x[idx] for x in ref], "80-pair list vs the 21-pair batch of the 24-pair engine")
        # 65 pairs: the shortest list that takes the fused form
        res65 = _pairs(e, slots[np.asarray(lst[:65])], K_vga)
        _same(res65, [x[:65] for x in res], "65-pair list")
    finally:
        e.close()


def test_resizing_the_store_ends_the_overflow_claim(capi, frames, K_vga):
    """rpe_fetch_overflow after a pair list reads the flags of the slots the list named: once rpe_frames_reserve has
    resized or freed the store it is refused (a host check), and the next list restores it"""
    e = capi.Engine(640, 480, max_batch=24, nfeatures=1000, max_matches=500)
    lib = e.lib
    fl = np.zeros(2, np.uint32)
    try:
        e.frames_reserve(64)
        e.frames_put(frames[:2], [60, 3])
        _pairs(e, [(60, 3), (3, 60)], K_vga)
        assert list(e.fetch_overflow(2)) == [0, 0]
        e.frames_reserve(16)                                  # slot 60 is gone
        assert lib.rpe_fetch_overflow(e.h, 2, fl.ctypes.data_as(C.c_void_p)) == -1 and lib.rpe_last_error(e.h).decode() != ""
        e.frames_put(frames[:1], [5])
        _pairs(e, [(5, 3)], K_vga)
        assert list(e.fetch_overflow(1)) == [0]
        e.frames_reserve(0)                                   # no store at all
        assert lib.rpe_fetch_overflow(e.h, 1, fl.ctypes.data_as(C.c_void_p)) == -1
        e.frames_reserve(32)                                  # growing: refused as well, the rule has no exceptions
        e.frames_put(frames[:2], [1, 2])
        _pairs(e, [(1, 2)], K_vga)
        e.frames_reserve(48)
        assert lib.rpe_fetch_overflow(e.h, 1, fl.ctypes.data_as(C.c_void_p)) == -1
        _same(_pairs(e, [(1, 2)], K_vga), _batch(e, frames, [(0, 1)], K_vga), "after the resizes")
        # frames_info names a range, wherever it lies in the store
        cnt, _ = e.frames_info([47, 1, 30, 2])
        assert cnt[0] == -1 and cnt[1] > 0 and cnt[2] == -1 and cnt[3] > 0
    finally:
        e.close()


def test_list_lengths(store8, frames, ref, K_vga):
    e = store8
    for n in (1, 2):                                          # the small-batch Hamming path (election words in HBM)
        _same(_pairs(e, WINDOW[4:4 + n], K_vga), _batch(e, frames, WINDOW[4:4 + n], K_vga), f"{n} pairs")
    full = (WINDOW + WINDOW[:3])[:24]                         # max_batch pairs
    assert len(full) == e.max_batch
    res = _pairs(e, full, K_vga)
    _same([x[:21] for x in res], ref, "max_batch pairs, first 21")
    _same([x[21:] for x in res], [x[:3] for x in ref], "max_batch pairs, repeats")


def _blobs(seed, n, lo, hi, W=640, H=480):
    """a few bright rectangles on a dark background: a handful of FAST corners per image (tests/test_gpu_structure.py)"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 40, np.uint8)
    for _ in range(n):
        w, h = rng.integers(lo, hi, 2)
        x = rng.integers(70, W - 70 - w); y = rng.integers(70, H - 70 - h)
        img[y:y + h, x:x + w] = rng.integers(150, 255)
    return img


def test_statuses(capi, eng, frames, ref, K_vga):
    e = eng
    e.frames_reserve(0)
    e.frames_reserve(12)
    blank = np.full((480, 640), 128, np.uint8)
    few = _blobs(7, 1, 14, 40)                                        # 42 keypoints; 3 matches against a stream frame (CPU oracle)
    imgs = np.concatenate([frames, blank[None], few[None]])          # frame 8 = blank, 9 = one rectangle
    e.frames_put(imgs, np.arange(10))
    cnt, _ = e.frames_info([8, 9, 10, 11])
    print("counts", cnt.tolist())
    assert cnt[0] == 0 and 0 < cnt[1] < 100 and cnt[2] == -1 and cnt[3] == -1
    lst = [(0, 8), (0, 1), (8, 1), (9, 0), (2, 5), (8, 8), (1, 9), (8, 9)]
    res = _pairs(e, lst, K_vga)
    st = res[4]
    ND, IM = capi.PAIR_NO_DESCRIPTORS, capi.PAIR_INSUFFICIENT_MATCHES
    assert list(st) == [ND, 0, ND, IM, 0, ND, IM, ND], st
    _same(res, _batch(e, imgs, lst, K_vga), "statuses vs batch")
    i01, i25 = WINDOW.index((0, 1)), WINDOW.index((2, 5))
    _same([x[[1, 4]] for x in res], [x[[i01, i25]] for x in ref], "good pairs of a list with failing ones")


def test_refusals(capi, frames, ref, K_vga):
    e = capi.Engine(640, 480, max_batch=24, nfeatures=1000, max_matches=500)
    lib, p = e.lib, (lambda a: a.ctypes.data_as(C.c_void_p))
    K = np.ascontiguousarray(K_vga, np.float64)
    w = np.ascontiguousarray(np.asarray(WINDOW, np.int32).T)
    INVALID, HIP, CAPACITY = -1, -2, -3

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert lib.rpe_last_error(e.h).decode() != ""

    def i32(*v):
        return np.array(v, np.int32)
    try:
        # no store yet
        refused(lib.rpe_enqueue_pairs(e.h, p(w[0]), p(w[1]), 21, p(K)), INVALID)
        refused(lib.rpe_frames_put(e.h, p(frames), 8, p(np.arange(8, dtype=np.int32))), INVALID)
        refused(lib.rpe_frames_info(e.h, 1, p(i32(0)), None, None), INVALID)
        e.frames_reserve(8)
        e.frames_put(frames[:7], np.arange(7))                  # slot 7 stays empty
        good = _pairs(e, [(0, 1), (2, 5)], K_vga)
        before = e.fetch_results(2)
        refused(lib.rpe_enqueue_pairs(e.h, p(i32(0, 8)), p(i32(1, 1)), 2, p(K)), INVALID)          # slot outside the store
        refused(lib.rpe_enqueue_pairs(e.h, p(i32(0, -1)), p(i32(1, 1)), 2, p(K)), INVALID)
        refused(lib.rpe_enqueue_pairs(e.h, p(i32(0, 1)), p(i32(7, 2)), 2, p(K)), INVALID)          # empty slot in a pair
        refused(lib.rpe_frames_put(e.h, p(frames), 2, p(i32(3, 3))), INVALID)                      # a slot twice in one put
        refused(lib.rpe_frames_put(e.h, p(frames), 2, p(i32(3, 8))), INVALID)                      # slot outside the store
        many = np.zeros(25, np.int32)
        refused(lib.rpe_enqueue_pairs(e.h, p(many), p(many), 25, p(K)), CAPACITY)                   # P > max_batch
        refused(lib.rpe_frames_put(e.h, p(frames), 49, p(np.arange(49, dtype=np.int32))), CAPACITY)  # n > 2*max_batch
        # a store the device cannot hold: 16 M slots of 42 KB ask for 571 GB of descriptors in one hipMalloc, twice the
        # 288 GB of an MI355X (an assumption about the machine: a device with more memory than that would grant it).
        # An allocation error, the old store is kept
        refused(lib.rpe_frames_reserve(e.h, 1 << 24), HIP)
        assert e.frames_capacity() == 8
        refused(lib.rpe_frames_reserve(e.h, -1), INVALID)
        # nothing ran: the results of the last valid list are still what a fetch returns, and slot 3 holds frame 3
        _same(e.fetch_results(2), before, "results after refused calls")
        cnt, _ = e.frames_info(np.arange(8))
        assert (cnt[:7] > 0).all() and cnt[7] == -1
        e.frames_put(frames[7:], [7])
        _same(_pairs(e, WINDOW, K_vga), ref, "first valid list after the refusals")
        i01, i25 = WINDOW.index((0, 1)), WINDOW.index((2, 5))
        _same(good, [x[[i01, i25]] for x in ref], "the list before the refusals")
    finally:
        e.close()


def test_profiling_reports_the_pair_stages(store8, K_vga):
    e = store8
    e.set_profiling(True)
    try:
        _pairs(e, WINDOW, K_vga)
        ms = e.stage_ms()
    finally:
        e.set_profiling(False)
    print(ms)
    assert ms["match"] > 0 and ms["ransac"] > 0 and ms["pose"] > 0
    assert all(v == 0 for k, v in ms.items() if k not in ("match", "ransac", "pose"))


def test_python_front_end(frames, K_vga):
    """PoseEstimator.estimate_pairs with more pairs than max_batch and more frames than 2*max_batch, and a FrameStore
    used as a ring that keeps the last three frames next to the new one (four slots)"""
    from relative_pose_estimation_amd import PoseEstimator, _capi, synthetic
    fr10 = synthetic.make_stream(10, K_vga)[0]
    lst = np.array([(i, i + d) for d in (1, 2, 3) for i in range(10 - d)] + [(9, 0), (4, 4)])
    big = PoseEstimator(K_vga, nfeatures=1000, max_matches=500, max_batch=len(lst))
    small = PoseEstimator(K_vga, nfeatures=1000, max_matches=500, max_batch=4)
    try:
        R0, t0, inl0, st0 = big.estimate_batch(fr10[lst[:, 0]], fr10[lst[:, 1]])
        nm0 = big._last_n_matches.copy()
        assert len(lst) > 4 and len(fr10) > 8
        R, t, inl, nm, st = small.estimate_pairs(fr10, lst)
        assert small._engines[(480, 640)].max_batch == 4
        _same((R, t, inl, nm, st), (R0, t0, inl0, nm0, st0), "estimate_pairs vs estimate_batch")
        assert (st == 0).all() and (nm > 400).all()
        assert len(small.last_structure()) == len(lst) % 4 or len(small.last_structure()) == 4      # the last chunk
        assert not small.last_overflow().any()
        eng = small._engines[(480, 640)]
        assert eng.frames_capacity() == 10
        again = small.estimate_pairs(fr10[:6], lst[:3])          # a shorter sequence reuses the store
        assert eng.frames_capacity() == 10
        _same(again, [x[:3] for x in (R, t, inl, nm, st)], "second estimate_pairs on the same engine")
        eng.frames_reserve(0)
        # online: frame i goes into slot i % 4 and is paired with the frames still in the ring
        w = np.asarray(WINDOW)
        Rw, tw, inlw, stw = big.estimate_batch(frames[w[:, 0]], frames[w[:, 1]])
        nmw = big._last_n_matches.copy()
        ring = small.frame_store(4)
        seen = {}
        for i in range(8):
            ring.put(i % 4, frames[i])
            mine = [k for k, (a, b) in enumerate(WINDOW) if max(a, b) == i]
            if not mine:
                continue
            assert all(i - min(WINDOW[k]) <= 3 for k in mine)
            got = ring.estimate([(WINDOW[k][0] % 4, WINDOW[k][1] % 4) for k in mine])
            for j, k in enumerate(mine):
                seen[k] = [x[j] for x in got]
        assert sorted(seen) == list(range(21))
        got = [np.stack([seen[k][f] for k in range(21)]) for f in range(5)]
        _same(got, (Rw, tw, inlw, nmw, stw), "ring of four slots vs the window list")
        cnt, _ = ring.info([0, 1, 2, 3])
        assert (cnt > 0).all()
        ring.close()
        with pytest.raises(_capi.RpeError):                     # the store is gone: refused, not read
            small.last_overflow()
    finally:
        big.close(); small.close()
