"""The pair-proposal kernels against the NumPy model (tests/similarity_model.py), through the C-ABI calls
rpe_similarity_hamming (stage form) and rpe_frames_similar (frame store).  Scores, candidates and counts are integers and
are compared exactly; nothing here has a tolerance.

The stage-form engines are 96 x 96 (the smallest legal image; only the keypoint capacity kcap = nfeatures + 64 matters to
these kernels).  The tests recompute the launcher's arithmetic (rpe_launch_similar, csrc/similar_kernels.hip) and assert the
form they mean to reach: the kept owner registers (a target sample of at most 8 tiles), the rounds of 8 owner tiles above
that, more than one query per workgroup, the triangle of identical lists."""
import numpy as np
import pytest

from tests import scale_model as scm
from tests import similarity_cases as sc
from tests import similarity_model as sm

pytestmark = pytest.mark.gpu

STEPS, DISTANCES = (1, 2, 3, 5), (0, 40, 256)


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module", params=[64, 320])
def stage(request, capi):
    e = capi.Engine(96, 96, max_batch=8, nfeatures=request.param, max_matches=64)
    assert e.kcap == request.param + 64
    yield e
    e.close()


@pytest.fixture(scope="module")
def small(capi):
    e = capi.Engine(96, 96, max_batch=8, nfeatures=64, max_matches=64)
    yield e
    e.close()


# ---------------------------------------------------------------- the launcher's arithmetic
def chunk_of(nq, nt, same):
    """query positions per workgroup (similar_chunk)"""
    pairs = nq * (nq + 1) // 2 if same else nq * nt
    return min(4, max(1, (pairs + 1023) // 1024))


def owner_kept(n, step):
    """the target's sample is at most 8 tiles: its owner registers are loaded once per workgroup"""
    return (-(-n // step) + 31) // 32 <= 8


def counts_for(kcap):
    """the tile edges, the edge of a round of 8 tiles, and one frame at the capacity"""
    return [c for c in (0, 1, 31, 32, 33, 64, 65, 256, 257) if c < kcap] + [kcap, 40]


def _call(e, descs, q, t, **kw):
    return e.similarity_hamming(descs, None, q, t, **kw)


def _check_scores(e, descs, steps=STEPS, distances=DISTANCES):
    F = len(descs)
    idx = np.arange(F, dtype=np.int32)
    perm = np.roll(idx, 3)                                            # a rectangular list over the same frames
    assert chunk_of(F, F, True) == 1
    for step in steps:
        for md in distances:
            want = sm.score_matrix(descs, idx, idx, step, md)
            tri = _call(e, descs, idx, idx, step=step, max_distance=md)["scores"]          # identical lists: the triangle
            assert np.array_equal(tri, want), (step, md, np.argwhere(tri != want)[:8].tolist())
            rect = _call(e, descs, idx, perm, step=step, max_distance=md)["scores"]
            assert np.array_equal(rect, want[:, perm]), (step, md)
            assert np.array_equal(rect[:, np.argsort(perm)], tri)


def test_stage_scores_equal_the_model(stage):
    counts = counts_for(stage.kcap)
    assert len(counts) <= 12 and len(counts) <= 2 * stage.max_batch
    if stage.kcap > 257:                                              # both owner forms are reached at step 1
        assert owner_kept(256, 1) and not owner_kept(257, 1) and not owner_kept(stage.kcap, 1) and owner_kept(stage.kcap, 2)
    _check_scores(stage, sc.random_frames(100 + stage.kcap, counts))


def test_stage_scores_with_ties_equal_the_model(stage):
    counts = counts_for(stage.kcap)
    descs = sc.tie_frames(200 + stage.kcap, counts)
    idx = np.arange(len(descs))
    assert not np.array_equal(sm.score_matrix(descs, idx, idx), sm.score_matrix(descs, idx, idx, last=True)), "the ties must matter"
    _check_scores(stage, descs, steps=(1, 3), distances=(0, 40, 256))
    for name in sc.HAND_CASES:
        frames, step, expected, _ = sc.hand_case(name)
        idx = np.arange(len(frames), dtype=np.int32)
        for md, want in expected.items():
            assert np.array_equal(_call(stage, frames, idx, idx, step=step, max_distance=md)["scores"], want), (name, md)


def test_repeats_and_single_rows(small):
    descs = sc.random_frames(7, [33, 0, 64, 128, 1, 65])
    q = np.array([3, 3, 0, 5, 1, 3], np.int32); t = np.array([2, 0, 0, 4, 2], np.int32)      # repeats within each list
    got = _call(small, descs, q, t, step=2, max_distance=40)["scores"]
    assert np.array_equal(got, sm.score_matrix(descs, q, t, 2, 40))
    got = _call(small, descs, q, q, step=1, max_distance=256)["scores"]                      # identical lists with repeats
    assert np.array_equal(got, sm.score_matrix(descs, q, q, 1, 256))
    for one in ([2], [1]):                                                                     # nq = 1, nt = 1; an empty frame
        assert np.array_equal(_call(small, descs, one, t)["scores"], sm.score_matrix(descs, one, t, 1, 48))
        assert np.array_equal(_call(small, descs, q, one)["scores"], sm.score_matrix(descs, q, one, 1, 48))
        assert np.array_equal(_call(small, descs, one, one)["scores"], sm.score_matrix(descs, one, one, 1, 48))
    # a stride beyond every frame: descriptor 0 against descriptor 0
    got = _call(small, descs, q, t, step=10 ** 9, max_distance=256)["scores"]
    assert np.array_equal(got, sm.score_matrix(descs, q, t, 10 ** 9, 256))


def test_owner_registers_are_kept_over_a_chunk_of_queries(small):
    """Lists long enough for 4 queries per workgroup (repeats make them so from 12 frames): a target of at most 8 tiles keeps its
    owner registers while the queries change -- among them an empty one and a full one -- and the election words start again
    for every pair."""
    counts = [128, 0, 1, 33, 128, 64, 0, 97, 31, 128, 5, 65]
    assert all(owner_kept(c, 1) for c in counts)
    descs = sc.random_frames(21, counts, pool=48)
    rng = np.random.default_rng(5)
    q = rng.integers(0, len(counts), 90).astype(np.int32)
    q[:8] = [0, 1, 4, 1, 2, 9, 6, 0]                                  # full, empty, full, empty, ... inside the first chunks
    t = rng.integers(0, len(counts), 40).astype(np.int32)
    assert chunk_of(q.size, t.size, False) == 4 and chunk_of(q.size, q.size, True) == 4
    for step, md in ((1, 256), (1, 30), (2, 40)):
        want = sm.score_matrix(descs, q, t, step, md)
        assert np.array_equal(_call(small, descs, q, t, step=step, max_distance=md)["scores"], want), (step, md)
        want = sm.score_matrix(descs, q, q, step, md)
        assert np.array_equal(_call(small, descs, q, q, step=step, max_distance=md)["scores"], want), (step, md, "triangle")
    # one target against a chunk of queries: the list of one column, long enough on the query side
    q = np.tile(np.array([0, 1, 3, 6, 9, 2, 1, 4], np.int32), 520)
    assert chunk_of(q.size, 1, False) == 4
    for tgt in ([7], [1], [0]):
        assert np.array_equal(_call(small, descs, q, tgt, max_distance=256)["scores"], sm.score_matrix(descs, q, tgt, 1, 256)), tgt


def test_owner_rounds_over_a_chunk_of_queries(capi):
    """the same with targets of more than 8 tiles: the owner registers are loaded again for every round of every pair"""
    e = capi.Engine(96, 96, max_batch=8, nfeatures=320, max_matches=64)
    try:
        counts = [384, 0, 257, 33, 300, 256]
        assert [owner_kept(c, 1) for c in counts] == [False, True, False, True, False, True]
        descs = sc.random_frames(22, counts, pool=128)
        rng = np.random.default_rng(6)
        q = rng.integers(0, len(counts), 70).astype(np.int32)
        t = rng.integers(0, len(counts), 50).astype(np.int32)
        assert chunk_of(q.size, t.size, False) == 4
        assert np.array_equal(_call(e, descs, q, t, max_distance=64)["scores"], sm.score_matrix(descs, q, t, 1, 64))
    finally:
        e.close()


def test_selection_equals_the_model(small):
    counts = [40, 64, 0, 128, 33, 90, 64, 17, 128, 100, 50, 1]
    descs = sc.random_frames(31, counts, pool=40)
    F = len(counts)
    idx = np.arange(F, dtype=np.int32)
    S = sm.score_matrix(descs, idx, idx, 1, 64)
    assert len(np.unique(S[S > 0])) < np.count_nonzero(S)            # equal scores in a row: the column breaks them
    for k in (1, 5, 32):                                              # 32 > the 11 eligible columns
        got = _call(small, descs, idx, idx, max_distance=64, k=k)
        cand, cs, n = sm.candidates(S, idx, idx, k)
        assert np.array_equal(got["scores"], S)
        assert np.array_equal(got["cand"], cand) and np.array_equal(got["cand_score"], cs) and np.array_equal(got["n_cand"], n), k
    assert (sm.candidates(S, idx, idx, 32)[2] == F - 1).all()
    # scores only (k = 0, no candidate arrays), candidates only (no score array)
    got = _call(small, descs, idx, idx, max_distance=64)
    assert got["cand"] is None and np.array_equal(got["scores"], S)
    got = _call(small, descs, idx, idx, max_distance=64, k=3, want_scores=False)
    cand, cs, n = sm.candidates(S, idx, idx, 3)
    assert got["scores"] is None and np.array_equal(got["cand"], cand) and np.array_equal(got["cand_score"], cs)
    # exclude without times (time = frame index), with times, min_score; rectangular lists with a repeated column
    q = np.array([0, 3, 5, 8, 3], np.int32); t = np.array([1, 3, 3, 4, 9, 8, 0, 6], np.int32)
    Sr = sm.score_matrix(descs, q, t, 1, 64)
    qt = np.array([100, 103, 105, 108, 250], np.int32); tt = np.array([101, 103, 300, 104, 109, 108, 100, -50], np.int32)
    for kw in (dict(exclude=2), dict(exclude=0), dict(exclude=1, q_time=qt, t_time=tt), dict(exclude=-1, q_time=qt, t_time=tt),
               dict(min_score=int(np.median(Sr))), dict(min_score=10 ** 6), dict(exclude=2 ** 31 - 1, q_time=qt, t_time=tt)):
        got = _call(small, descs, q, t, max_distance=64, k=4, **kw)
        cand, cs, n = sm.candidates(Sr, q, t, 4, **kw)
        assert np.array_equal(got["cand"], cand) and np.array_equal(got["cand_score"], cs) and np.array_equal(got["n_cand"], n), kw


# ---------------------------------------------------------------- the frame store
STORE_SLOTS = np.array([9, 2, 14, 5, 0, 11], np.int32)               # frame f of the PHYSICS stream in slot STORE_SLOTS[f]


@pytest.fixture(scope="module")
def store(capi):
    frames, K = scm.physics_frames()
    e = capi.Engine(640, 480, max_batch=8, nfeatures=scm.PHYSICS_NFEATURES, max_matches=scm.PHYSICS_MAX_MATCHES)
    e.frames_reserve(16)
    e.frames_put(frames, STORE_SLOTS)
    _, desc, counts = e.orb_detect_and_compute(frames)
    descs = {int(s): desc[f, :counts[f]].copy() for f, s in enumerate(STORE_SLOTS)}
    yield e, descs, K
    e.close()


def test_store_scores_equal_the_model_of_the_extracted_descriptors(store):
    e, descs, _ = store
    q = np.array([14, 0, 9, 2, 5, 11, 9], np.int32); t = np.array([2, 5, 0, 11], np.int32)
    for step, md in ((1, 48), (4, 64)):
        want = sm.score_matrix(descs, q, t, step, md)
        got = e.frames_similar(q, t, step=step, max_distance=md, k=2, exclude=3)
        assert np.array_equal(got["scores"], want), (step, md)
        cand, cs, n = sm.candidates(want, q, t, 2, exclude=3)
        assert np.array_equal(got["cand"], cand) and np.array_equal(got["cand_score"], cs) and np.array_equal(got["n_cand"], n)
        again = e.frames_similar(q, t, step=step, max_distance=md, k=2, exclude=3)
        assert all(np.array_equal(got[key], again[key]) for key in got)                 # repeats bit for bit
    allq = np.sort(STORE_SLOTS)
    want = sm.score_matrix(descs, allq, allq, 1, 48)
    assert np.array_equal(e.frames_similar(allq, allq)["scores"], want)
    assert (np.diag(want) > 900).all() and (want[~np.eye(6, dtype=bool)] < np.diag(want).min()).all()


def test_store_call_leaves_the_last_run_untouched(store):
    e, descs, K = store
    s1, s2 = STORE_SLOTS[:-1], STORE_SLOTS[1:]
    P = s1.size
    res = e.estimate_pairs(s1, s2, K)
    assert (res[4] == 0).all()

    def fetched():
        return [np.array(x) for x in e.fetch_results(P)] + [np.array(x) for x in e.fetch_structure(P)] + [np.array(e.fetch_overflow(P))] \
            + [np.array(x) for x in e.fetch_matched_points(P)]

    before = fetched()
    e.frames_similar(STORE_SLOTS, STORE_SLOTS, k=3)
    e.frames_similar(STORE_SLOTS[:2], STORE_SLOTS, step=4, want_scores=False, k=1)
    after = fetched()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert all(np.array(a).tobytes() == np.array(b).tobytes() for a, b in zip(res, e.fetch_results(P)))
    # the stage form goes through the last-run gate like every stage call
    e.similarity_hamming([descs[int(STORE_SLOTS[0])]], None, [0], [0])
    from relative_pose_estimation_amd import _capi
    with pytest.raises(_capi.RpeError):
        e.fetch_structure(P)


# ---------------------------------------------------------------- refusals
def _raw(e, lib_call, q, t, step=1, md=48, k=0, scores=True, cand=True, n_cand=True, head=()):
    from relative_pose_estimation_amd._capi import _p
    q = np.ascontiguousarray(q, np.int32); t = np.ascontiguousarray(t, np.int32)
    S = np.zeros((max(q.size, 1), max(t.size, 1)), np.int32)
    c = np.zeros((max(q.size, 1), max(k, 1)), np.int32); cs = c.copy(); n = np.zeros(max(q.size, 1), np.int32)
    return lib_call(e.h, *head, q.size, _p(q), t.size, _p(t), step, md, None, None, -1, 0, k,
                    _p(S) if scores else None, _p(c) if cand else None, _p(cs) if cand else None, _p(n) if n_cand else None)


def test_refusals_leave_the_handle_usable(capi, store, small):
    e, descs, _ = store
    ERR_INVALID = -1
    f = e.lib.rpe_frames_similar
    ok = [int(STORE_SLOTS[0]), int(STORE_SLOTS[1])]
    assert _raw(e, f, ok, ok) == 0
    bad = [dict(q=[16], t=ok), dict(q=ok, t=[-1]),                   # a slot outside the store
           dict(q=[1], t=ok),                                         # an empty slot
           dict(q=ok, t=ok, step=0), dict(q=ok, t=ok, md=-1), dict(q=ok, t=ok, md=257),
           dict(q=ok, t=ok, k=-1), dict(q=ok, t=ok, k=capi.SIMILAR_MAX_K + 1),
           dict(q=[], t=ok), dict(q=ok, t=[]),                        # nq < 1, nt < 1
           dict(q=ok, t=ok, scores=False, cand=False, n_cand=False),  # no output
           dict(q=ok, t=ok, k=2, n_cand=False)]                       # part of the candidate trio
    for kw in bad:
        assert _raw(e, f, **kw) == ERR_INVALID, kw
        assert e.lib.rpe_last_error(e.h).decode().startswith("rpe_frames_similar: "), kw
        want = sm.score_matrix(descs, ok, ok, 1, 48)
        assert np.array_equal(e.frames_similar(ok, ok)["scores"], want), kw           # the handle works afterwards
    assert _raw(e, f, ok, ok, k=0, cand=False, n_cand=False) == 0                     # k = 0 with the trio NULL is allowed
    assert _raw(e, f, ok, ok, k=capi.SIMILAR_MAX_K, scores=False) == 0
    # no store
    assert small.frames_capacity() == 0 and _raw(small, f, [0], [0]) == ERR_INVALID
    assert "no frame store" in small.lib.rpe_last_error(small.h).decode()
    # the stage form: its own frame range and counts
    g = e.lib.rpe_similarity_hamming
    from relative_pose_estimation_amd._capi import _p
    D = np.zeros((2, small.kcap, 32), np.uint8)
    for n, q, code in (([3, 4], [2], ERR_INVALID), ([3, small.kcap + 1], [0], ERR_INVALID), ([3, -1], [0], ERR_INVALID), ([3, 4], [1], 0)):
        n = np.array(n, np.int32)
        assert _raw(small, g, q, [0], head=(_p(D), _p(n), 2)) == code, (n, q)
    n = np.array([3, 4], np.int32)
    assert _raw(small, g, [0], [0], head=(_p(D), _p(n), 0)) == ERR_INVALID            # F < 1
    assert _raw(small, g, [0], [0], head=(_p(D), _p(n), 2 * small.max_batch + 1)) == -3   # RPE_ERR_CAPACITY
    # L2 and SIFT handles
    for kw in (dict(norm_type=capi.NORM_L2), dict(norm_type=capi.NORM_L2, feature_method=capi.FEATURE_SIFT)):
        l2 = capi.Engine(96, 96, max_batch=1, nfeatures=64, max_matches=64, **kw)
        try:
            l2.frames_reserve(2)
            assert _raw(l2, f, [0], [0]) == ERR_INVALID and "Hamming handles only" in l2.lib.rpe_last_error(l2.h).decode()
            Dl = np.zeros((1, l2.kcap, 32), np.uint8); nl = np.zeros(1, np.int32)
            assert _raw(l2, g, [0], [0], head=(_p(Dl), _p(nl), 1)) == ERR_INVALID
        finally:
            l2.close()


# ---------------------------------------------------------------- end to end
def test_proposed_pairs_close_the_loop(oracle):
    """FrameStore.propose_pairs on the loop scene proposes every revisit pair of the CPU table, and FrameStore.estimate returns
    a pose for each of them."""
    from relative_pose_estimation_amd import PoseEstimator, geometry
    frames, K, twin, distract = sc.loop_scene()
    n = frames.shape[0]
    pe = PoseEstimator(K, nfeatures=sc.LOOP_NFEATURES, max_batch=8)
    try:
        fs = pe.frame_store(n)
        fs.put_many(np.arange(n), frames)
        _, S = sc.loop_table(oracle)
        got = fs.similar(max_distance=sc.LOOP_MAX_DISTANCE)
        assert np.array_equal(got["queries"], np.arange(n)) and np.array_equal(got["scores"], S[(1, sc.LOOP_MAX_DISTANCE)])
        got = fs.similar(max_distance=sc.LOOP_MAX_DISTANCE, step=4)
        assert np.array_equal(got["scores"], S[(4, sc.LOOP_MAX_DISTANCE)])
        pairs, score = fs.propose_pairs(k=2, exclude=3)
        cand, cs, _ = sm.candidates(S[(1, sc.LOOP_MAX_DISTANCE)], np.arange(n), np.arange(n), 2, exclude=3)
        want = geometry.pairs_of_candidates(np.arange(n), np.arange(n), cand, cs)
        assert np.array_equal(pairs, want[0]) and np.array_equal(score, want[1])
        assert pairs.shape[1] == 2 and (pairs[:, 0] < pairs[:, 1]).all() and len({tuple(p) for p in pairs.tolist()}) == len(pairs)
        assert (np.diff(score) <= 0).all()
        revisit = [(int(twin[f]), int(f)) for f in np.nonzero(twin >= 0)[0]]
        for p in revisit:
            assert list(p) in pairs.tolist(), (p, pairs.tolist())
        R, t, inl, nm, st = fs.estimate(np.array(revisit, np.int32))
        assert (st == 0).all(), st
        fs.close()
    finally:
        pe.close()
