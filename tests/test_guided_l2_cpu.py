"""The model of guided matching for NORM_L2 handles (tests/guided_l2_model.py) against its plain-loops twin and against
the crossCheck model, and the conditions that keep the shared inputs of tests/test_gpu_guided_l2.py from passing
vacuously -- all from the models alone, no GPU."""
import math

import numpy as np
import pytest

from tests import guided_l2_model as g2
from tests import guided_model as gm
from tests import match_cases as mc
from tests import match_model as M


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


TINY = [("l2_sift_1984_ring", n1, n2, kind) for n1, n2, kind in
        [(2, 3, "mixed"), (5, 2, "mixed"), (8, 8, "mixed"), (17, 12, "mixed"), (1, 1, "mixed"), (0, 9, "mixed"), (9, 0, "mixed")]] + \
       [("l2_orb_1984_ring", 40, 32, "mixed"), ("l2_orb_1984_ring", 33, 40, "mixed"), ("l2_orb_1984_ring", 40, 161, "far")]


@pytest.mark.parametrize("list_name,n1,n2,kind", TINY)
def test_model_equals_plain_loops(list_name, n1, n2, kind):
    c = mc.case(list_name, n1, n2, kind)
    p1, p2 = g2.keypoints(c.name, list_name)
    K = g2.camera_K(); R, t = g2.pose()
    x1, x2 = gm.normalise_K(p1, K), gm.normalise_K(p2, K)
    D = g2.distances(c.name, list_name)
    bounds = [math.inf, 0.0] + ([float(np.median(D))] if D.size else [])
    for gate_px in (1.0, 25.0, 1e9):
        for bound in bounds:
            for mm in (None, 3):
                fast = g2.guided_match(c.desc1, x1, c.desc2, x2, R, t, g2.thr2(gate_px), bound, mm)
                slow = g2.guided_match_slow(c.desc1, x1, c.desc2, x2, R, t, g2.thr2(gate_px), bound, mm)
                assert _same(fast, slow), (c.name, gate_px, bound, mm)


@pytest.mark.parametrize("list_name", g2.LISTS)
def test_open_gate_equals_crosscheck(list_name):
    K = g2.camera_K(); R, t = g2.pose()
    mm = mc.SPECS[list_name].max_matches
    for c in mc.cases(list_name):
        p1, p2 = g2.keypoints(c.name, list_name)
        got = g2.guided_match(c.desc1, gm.normalise_K(p1, K), c.desc2, gm.normalise_K(p2, K), R, t, g2.thr2(1e9), math.inf, mm)
        assert _same(got, M.match_l2(c.desc1, c.desc2, mm)), c.name
        assert _same(got, mc.expected(list_name, c)), c.name


@pytest.mark.parametrize("list_name", g2.LISTS)
def test_inputs_exercise_the_gate(list_name):
    """Summed over the list: at least 100 guided matches; at least 50 whose query's overall nearest train is inadmissible;
    at least 10 whose query has an inadmissible train of equal float32 distance and lower index.  Every case with both
    sides >= 32 has a guided set other than its crossCheck set.  Some case is truncated by the list's max_matches."""
    total = beyond = tied = 0
    cut = False
    for c in mc.cases(list_name):
        q, j, d = g2.expected(c.name, list_name, math.inf, None)
        D = g2.distances(c.name, list_name); adm = g2.gate(c.name, list_name)
        total += len(q)
        cut = cut or len(q) > mc.SPECS[list_name].max_matches
        if len(q):
            beyond += int((~adm[q, D[q].argmin(1)]).sum())
            for i, jj, dd in zip(q, j, d):
                tied += bool(((D[i, :jj] == dd) & ~adm[i, :jj]).any())
        if min(D.shape) >= 32:
            cross = M.cross_check(D, max(D.shape[0], 1))
            assert not _same((q, j, d), cross), c.name
    print(list_name, "guided", total, "nearest inadmissible", beyond, "tied with a lower inadmissible train", tied)
    assert total >= 100 and beyond >= 50 and tied >= 10, (list_name, total, beyond, tied)
    assert cut, list_name


@pytest.mark.parametrize("list_name", g2.LISTS)
def test_admissible_crosscheck_matches_are_guided_matches(list_name):
    for c in mc.cases(list_name):
        D = g2.distances(c.name, list_name)
        if D.size == 0:
            continue
        adm = g2.gate(c.name, list_name)
        cq, cj, _ = M.cross_check(D, max(D.shape[0], 1))
        q, j, _ = g2.expected(c.name, list_name, math.inf, None)
        guided = set(zip(q.tolist(), j.tolist()))
        for i, jj in zip(cq.tolist(), cj.tolist()):
            if adm[i, jj]:
                assert (i, jj) in guided, (c.name, i, jj)


def test_distance_bound_and_truncation():
    """max_distance filters entries, not matches: a bound can create a match that the unbounded rule does not have; the
    bounded answer is still the model of the bounded matrix.  max_distance = 0 keeps equal rows only."""
    name = "l2_sift_448"
    c = mc.case(name, 512, 512)
    full = g2.expected(c.name, name, math.inf, None)
    med = float(np.median(full[2]))
    bounded = g2.expected(c.name, name, med, None)
    assert 0 < len(bounded[0]) < len(full[0]) and (bounded[2] <= med).all()
    zero = g2.expected(c.name, name, 0.0, None)
    assert len(zero[0]) >= 1 and (zero[2] == 0).all()
    for i, j in zip(zero[0], zero[1]):
        assert np.array_equal(c.desc1[i], c.desc2[j])
    head = g2.expected(c.name, name, math.inf, 7)
    assert _same(head, tuple(a[:7] for a in full))


def test_binding_table_has_the_l2_calls():
    from relative_pose_estimation_amd import _capi
    C = _capi.C
    for name, n_args, doubles in (("rpe_guided_matches_l2", 12, (4, 5)), ("rpe_match_l2_guided", 17, (11, 12))):
        assert name in _capi.EXPORTS
        ret, args = _capi.SIGNATURES[name]
        assert ret is C.c_int and len(args) == n_args
        assert [k for k, a in enumerate(args) if a is C.c_double] == list(doubles)
