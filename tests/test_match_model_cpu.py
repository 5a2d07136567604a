"""The matcher model (tests/match_model.py) against the C oracle on every case of tests/match_cases.py: all four
functions, both descriptor widths, indices and distances equal (L2 distances as uint32 views).  The two were written
apart -- the oracle keeps packed (distance, index) keys as the kernels do, the model takes argmins of the whole distance
matrix -- so their agreement is what lets the GPU tests use the model as referee.  The generator's own conditions
(match_cases.check_list) are asserted here too: no list can pass vacuously."""
import numpy as np
import pytest

from tests import match_cases as mc
from tests import match_model as mm


@pytest.mark.parametrize("list_name", sorted(mc.SPECS))
def test_model_equals_oracle(oracle, list_name):
    spec = mc.SPECS[list_name]
    for c in mc.cases(list_name):
        a, b = (c.desc1, c.desc2) if spec.norm == "hamming" else (c.desc1.astype(np.float32), c.desc2.astype(np.float32))
        for r in spec.ratios or (None,):
            if spec.norm == "hamming":
                got = oracle.match_hamming(a, b, spec.max_matches) if r is None else oracle.match_hamming_ratio(a, b, r, spec.max_matches)
            else:
                got = oracle.match_l2(a, b, spec.max_matches) if r is None else oracle.match_l2_ratio(a, b, r, spec.max_matches)
            q, t, d = mc.expected(list_name, c, r)
            assert len(got[0]) == len(q), (c.name, r, len(got[0]), len(q))
            assert np.array_equal(got[0], q) and np.array_equal(got[1], t), (c.name, r)
            if spec.norm == "hamming":
                assert np.array_equal(got[2], d), (c.name, r)
            else:
                assert d.dtype == np.float32 and np.array_equal(got[2].view(np.uint32), d.view(np.uint32)), (c.name, r)


@pytest.mark.parametrize("list_name", sorted(mc.SPECS))
def test_lists_cannot_pass_vacuously(list_name):
    mc.check_list(list_name)


def test_case_contents():
    """the ingredients are where the generator says: extremes, planted ties, the 1 x 1 extreme pair"""
    c = mc.case("ham_448", 512, 512)
    D = mm.hamming_matrix(c.desc1, c.desc2)
    assert {0, 1, 255, 256} <= set(np.unique(D).tolist())
    for p, q in mc.TIE_PAIRS + ((510, 511),):
        assert np.array_equal(c.desc2[p], c.desc2[q]) and (D[:, p] == 0).any(), (p, q)
        assert np.array_equal(c.desc1[p], c.desc1[q]) and (D[p] == 0).any(), (p, q)
    assert ((D == 0).sum(0) >= 3).any()                          # several queries equal one train row
    for name, dim in (("l2_sift_448", 128), ("l2_orb_448", 32)):
        S = mm.l2_squared_matrix(*mc.case(name, 512, 512)[1:])
        assert S.max() == dim * 65025 and S.min() == 0
    one = mc.case("ham_96", 1, 1)
    assert mm.hamming_matrix(one.desc1, one.desc2)[0, 0] == 256
    # the same case twice is the same bytes: the CPU and the GPU tests see one input
    again = mc.make_case("ham_448", 512, 512, 32, "hamming", "mixed")
    assert np.array_equal(again.desc1, c.desc1) and np.array_equal(again.desc2, c.desc2)
    # far L2 rows: squared distances beyond 2^22, where float32 roots of neighbouring integers collide
    far = mc.case("l2_sift_448", 288, 288, "far")
    S = mm.l2_squared_matrix(far.desc1, far.desc2)
    assert S.min() > 1 << 22 and len(np.unique(np.sqrt(S.astype(np.float32)))) < len(np.unique(S))


def test_ratio_drops_equal_best_and_second():
    """two equal best trains: dropped for every ratio <= 1, ratio = 1.0 included; kept once one of them is gone"""
    c = mc.case("ham_8000_ratio", 257, 1025)
    D = mm.hamming_matrix(c.desc1, c.desc2)
    i = int(np.nonzero(D[:, 3] == 0)[0][0])                      # the query that equals trains 3 and 4
    assert D[i, 4] == 0
    for r in (0.75, 1.0):
        assert i not in mm.ratio_test(D, r, 257)[0]
        assert i in mm.ratio_test(np.delete(D, 4, axis=1), r, 257)[0]
    assert len(mm.ratio_test(D[:, :1], 1.0, 257)[0]) == 0        # fewer than two trains: nothing
