"""The pairs of tests/onepass_cases.py under the NumPy matcher model alone: they must hold the ties and the rejections
that tests/test_gpu_match_onepass.py means to put before the kernel, or that test compares little."""
import numpy as np
import pytest

from tests import match_model as mm
from tests import onepass_cases as oc


def _pairs(d1, d2, last=False):
    q, t, d = mm.match_hamming(d1, d2, oc.MAX_MATCHES, last=last)
    return {(int(a), int(b)): int(c) for a, b, c in zip(q, t, d)}


def test_full_structure():
    d1, d2, fitted = oc.make(300, 300)
    assert set(fitted) == {"cols_3_19_35", "lanes_1_apart", "lanes_2_apart", "lanes_4_apart", "lanes_8_apart", "rounds", "dup_queries",
                           "dup_queries_small", "crowded_train", "crowded_train_small", "two_electors", "two_electors_small", "weights"}
    D = mm.hamming_matrix(d1, d2)
    m = _pairs(d1, d2)
    # equal row entries, the lowest train wins: columns 3 | 19 (lanes 16 apart) | 35 (next tile), lanes 1, 2, 4, 8 apart, three rounds
    for qi, trains, dist in [(7, (3, 19, 35), 3), (8, (40, 41), 2), (9, (44, 46), 2), (10, (48, 52), 2), (11, (50, 58), 2), (12, (10, 266, 299), 1)]:
        assert all(D[qi, j] == dist for j in trains) and D[qi].min() == dist and (D[qi] == dist).sum() == len(trains)
        assert m[(qi, trains[0])] == dist and not any((qi, j) in m for j in trains[1:])
    # equal column entries, the lowest query wins; the other copies choose the same train and are rejected
    assert all(D[i, 150] == 4 for i in (5, 21, 37, 261)) and D[:, 150].min() == 4
    assert m[(5, 150)] == 4 and not any(q in (21, 37, 261) for q, _ in m)
    assert m[(6, 20)] == 4 and not any(q == 22 for q, _ in m)
    # a train three queries choose elects one; a query two trains elect takes the nearer
    assert [int(np.argmin(D[i])) for i in (13, 14, 290)] == [200] * 3 and m[(13, 200)] == 2 and not any(q in (14, 290) for q, _ in m)
    assert [int(np.argmin(D[:, j])) for j in (210, 280)] == [30, 30] and m[(30, 210)] == 2 and not any(t == 280 for _, t in m)
    # popcounts 0 and 256, distance 0, and their repeats
    assert m[(0, 1)] == 0 and m[(1, 0)] == 0 and not any(q == 2 for q, _ in m) and not any(t == 2 for _, t in m)
    assert D[0, 0] == 256


@pytest.mark.parametrize("n1,n2", [s for s in oc.SIZES if min(s) >= 33])
def test_ties_and_rejections_in_every_size(n1, n2):
    """each pair of some size has ties that decide matches (taking the LAST of equal distances gives other matches), queries
    that are rejected, trains that nobody keeps, and row winners that differ from the column winners"""
    d1, d2, fitted = oc.make(n1, n2)
    assert "cols_3_19_35" in fitted and "weights" in fitted
    D = mm.hamming_matrix(d1, d2)
    first, last = _pairs(d1, d2), _pairs(d1, d2, last=True)
    assert first != last
    assert first[(7, 3)] == 3 and (7, 3) not in last
    kept = len(first)
    assert 0 < kept < min(n1, n2) and n1 - kept >= 3
    # a row election that copied the column election would match every train's elected query: more than crossCheck keeps
    elected = {int(np.argmin(D[:, j])) for j in range(n2)}
    assert len(elected) > kept


def test_edges():
    for n1, n2 in [(0, 40), (40, 0)]:
        d1, d2, _ = oc.make(n1, n2)
        assert len(d1) == n1 and len(d2) == n2 and _pairs(d1, d2) == {}
    d1, d2, _ = oc.make(1, 1)
    assert _pairs(d1, d2) == {(0, 0): 256}


def test_second_round_sizes():
    """300 owners are 10 tiles: a second round of 8; 300 scanned rows are 10 tiles: three trips of the 4-tile ring"""
    assert (300 + 31) // 32 > 8 and (oc.NFEATURES + 64 + 31) // 32 == 16
