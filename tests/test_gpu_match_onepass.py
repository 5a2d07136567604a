"""match_hamming_mfma_kernel elects both crossCheck sides in one pass over the product tiles: the trains' nearest queries
down the columns, the queries' nearest trains along the rows (a lane reduction per tile, joined over waves and rounds by an
atomicMin).  Its matches (qidx, tidx, dist, n_matches) against the NumPy model of tests/match_model.py, bit for bit, on
the hand-made pairs of tests/onepass_cases.py (tests/test_match_onepass_cpu.py shows what ties and rejections they hold),
in the SPLIT form (election words in HBM, match_hamming_select_kernel converts the row keys), the fused form (LDS) and
the pair-table instances."""
import numpy as np
import pytest

from tests import match_model as mm
from tests import onepass_cases as oc
from tests.test_gpu_match_model import hamming_form

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def eng(capi):
    e = capi.Engine(96, 96, max_batch=65, nfeatures=oc.NFEATURES, max_matches=oc.MAX_MATCHES)
    assert e.kcap == 512
    yield e
    e.close()


@pytest.fixture(scope="module")
def pairs():
    """[(name, desc1, desc2, (qidx, tidx, dist))]: the model's matches, computed once"""
    return [(name, d1, d2, oc.expected(d1, d2)) for name, d1, d2 in oc.all_pairs()]


def _check(e, group):
    n1 = [len(p[1]) for p in group]; n2 = [len(p[2]) for p in group]
    q, t, d, nm = e.match_hamming([p[1] for p in group], n1, [p[2] for p in group], n2)
    bad = []
    for i, (name, d1, d2, (wq, wt, wd)) in enumerate(group):
        n = int(nm[i])
        kept, rejected = n, len(d1) - n                        # max_matches >= n1: nothing is truncated
        if (kept, rejected) != (len(wq), len(d1) - len(wq)):
            bad.append((i, name, "kept / rejected", (kept, rejected), "model", (len(wq), len(d1) - len(wq))))
        elif not (np.array_equal(q[i, :n], wq) and np.array_equal(t[i, :n], wt) and np.array_equal(d[i, :n], wd)):
            k = int(np.nonzero((q[i, :n] != wq) | (t[i, :n] != wt) | (d[i, :n] != wd))[0][0])
            bad.append((i, name, "first difference at", k, "got", (int(q[i, k]), int(t[i, k]), int(d[i, k])),
                        "model", (int(wq[k]), int(wt[k]), int(wd[k]))))
    assert not bad, bad


def test_split_one_pair(eng, pairs):
    """a batch of one pair: gridDim = (1, 2), the two rounds of owner tiles in two workgroups, the row keys joined in HBM"""
    assert hamming_form(eng.kcap, 1) == ("split", 2, 2)
    for p in pairs:
        _check(eng, [p])


def test_split_three_pairs(eng, pairs):
    """batches of three unequal pairs: the election words of pair p start at p * kcap"""
    assert hamming_form(eng.kcap, 3) == ("split", 2, 2)
    by = {p[0]: p for p in pairs}
    _check(eng, [by["33x65"], by["300x300"], by["0x40"]])
    _check(eng, [by["40x300"], by["1x1"], by["300x40"]])
    _check(eng, [by["40x0"], by["300x40"], by["33x65"]])


def test_fused_65_pairs(eng, pairs):
    """65 pairs take the fused kernel: one workgroup per pair walks both rounds, the row keys meet in LDS and are converted
    before the sort.  Every size in turn, so the small and empty pairs sit between the large ones."""
    assert hamming_form(eng.kcap, 65) == ("fused", 1, 2)
    _check(eng, [pairs[i % len(pairs)] for i in range(65)])


@pytest.mark.parametrize("P", [3, 65])
def test_pair_table_with_a_repeated_frame(capi, P):
    """the pair-table instances (SPLIT at 3 pairs, fused at 65): a pair list over three stored frames that names frame 0 in
    several pairs, on either side.  The store takes extracted frames only, so these descriptors are ORB's, read back through
    the stage call; the list's match indices and counts equal the model's on them (the distances stay on the device)."""
    from relative_pose_estimation_amd import geometry, synthetic
    W, H = 320, 240
    K = geometry.default_camera_matrix(W, H)
    fr = synthetic.make_stream(3, K, W, H)[0]
    e = capi.Engine(W, H, max_batch=65, nfeatures=300, max_matches=400)
    try:
        assert hamming_form(e.kcap, P)[0] == ("split" if P == 3 else "fused")
        _, desc, cnt = e.orb_detect_and_compute(fr)
        assert (cnt > 32).all(), cnt
        e.frames_reserve(3)
        e.frames_put(fr, [0, 1, 2])
        lst = ([(0, 1), (2, 0), (0, 2), (1, 0), (1, 2)] * 13)[:P]
        s1 = [a for a, _ in lst]; s2 = [b for _, b in lst]
        nm = e.estimate_pairs(s1, s2, K)[3]
        q, t = e.fetch_match_indices(P)
        want = {}
        for p, (a, b) in enumerate(lst):
            if (a, b) not in want:
                want[(a, b)] = mm.match_hamming(desc[a, :cnt[a]], desc[b, :cnt[b]], 400)
            wq, wt, _ = want[(a, b)]
            n = int(nm[p])
            assert n == len(wq) > 0, (p, a, b, n, len(wq))
            assert np.array_equal(q[p, :n], wq) and np.array_equal(t[p, :n], wt), (p, a, b)
    finally:
        e.close()
