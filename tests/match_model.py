"""NumPy model of the brute-force matchers, written from cv2's rules and from nothing else: no code shared with oracle/
or the kernels, no packed keys.  It builds the whole n1 x n2 distance matrix and applies the rule to it.

Distances.  Hamming: the number of differing bits of the 256-bit rows.  L2: the float32 square root of the exact integer
sum of squared byte differences, which is what cv2's batchDistance returns for byte-valued rows.  Both matrices come
from |a|^2 + |b|^2 - 2 a.b with the product a.b taken by a floating-point matrix multiplication and cast back to integers.
That product is exact: its terms are byte products (L2, float64: at most 128 x 255^2 = 8 323 200, every partial sum an
integer below 2^53) or 0/1 (Hamming, float32: at most 256 unpacked bits, every partial sum an integer below 2^24), and
the format represents those integers without rounding in whatever order BLAS adds them.  The sum of squares is below 2^24, so its conversion to float32 is exact as well, and NumPy's float32
sqrt is correctly rounded (IEEE 754): the model's L2 distance is THE float32 distance, bit for bit.

crossCheck (cv2.BFMatcher(norm, crossCheck=True).match): j(i) = argmin_j D[i, j] and i(j) = argmin_i D[i, j], both taking
the first (lowest) index among equal distances; query i is matched to j(i) iff i(j(i)) == i.  For L2 the argmins compare
the float32 distances, not the integers under the root: beyond 2^22 neighbouring integers share one root.

Ratio (knnMatch(k=2) + Lowe's test): best and second-best train of a query, lowest index on ties; kept iff
float64(best) < ratio * float64(second); fewer than two trains give nothing.

Order: stable sort by distance, so the query index breaks ties, then the first max_matches.  An empty side gives none.

`last=True` replaces every first-occurrence argmin by the last occurrence.  No matcher does that; the case generator uses
it to prove that a case has ties that matter."""
import numpy as np

ROW_BLOCK = 1024


def _gram(a, b, dtype=np.float64):
    """a @ b.T of two integer matrices, exact (see above), as int32; in row blocks to bound the floating scratch"""
    a = np.asarray(a, dtype); b = np.ascontiguousarray(np.asarray(b, dtype).T)
    out = np.empty((a.shape[0], b.shape[1]), np.int32)
    for r in range(0, a.shape[0], ROW_BLOCK):
        out[r:r + ROW_BLOCK] = a[r:r + ROW_BLOCK] @ b
    return out


def hamming_matrix(d1, d2):
    """(n1, n2) int32: differing bits of the uint8 rows of d1 and d2.  The product of 0/1 rows is at most 256, so float32
    (exact below 2^24) carries it as well as float64 does, at half the memory traffic."""
    a = np.unpackbits(np.asarray(d1, np.uint8), axis=1); b = np.unpackbits(np.asarray(d2, np.uint8), axis=1)
    pa = a.sum(1, dtype=np.int32); pb = b.sum(1, dtype=np.int32)
    D = _gram(a, b, np.float32)
    D *= -2
    D += pa[:, None]; D += pb[None, :]
    return D


def l2_squared_matrix(d1, d2):
    """(n1, n2) int32: sum of squared differences of byte-valued rows (uint8, or floats holding 0..255 integers)"""
    a = np.asarray(d1).astype(np.int32); b = np.asarray(d2).astype(np.int32)
    assert np.array_equal(a, d1) and np.array_equal(b, d2) and min(a.min(initial=0), b.min(initial=0)) >= 0 \
        and max(a.max(initial=0), b.max(initial=0)) <= 255, "byte-valued rows only"
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * _gram(a, b)


def l2_matrix(d1, d2):
    """(n1, n2) float32 distances"""
    s = l2_squared_matrix(d1, d2)
    assert s.size == 0 or (s.min() >= 0 and s.max() < 1 << 24)
    return np.sqrt(s.astype(np.float32))


def _argmin(D, axis, last):
    if not last:
        return np.argmin(D, axis=axis)
    return D.shape[axis] - 1 - np.argmin(np.flip(D, axis=axis), axis=axis)


def _none(D):
    return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, D.dtype)


def _ordered(q, j, d, max_matches):
    o = np.argsort(d, kind="stable")[:max_matches]          # q ascends already: equal distances keep the query order
    return q[o], j[o], d[o]


def cross_check(D, max_matches, last=False):
    """(qidx, tidx, dist) of the mutual nearest neighbours of distance matrix D"""
    if D.shape[0] == 0 or D.shape[1] == 0:
        return _none(D)
    j_of_i = _argmin(D, 1, last)
    i_of_j = _argmin(D, 0, last)
    q = np.nonzero(i_of_j[j_of_i] == np.arange(D.shape[0]))[0]
    return _ordered(q, j_of_i[q], D[q, j_of_i[q]], max_matches)


def ratio_test(D, ratio, max_matches, last=False):
    """(qidx, tidx, dist) of the queries whose best train passes Lowe's test against the second best"""
    if D.shape[0] == 0 or D.shape[1] < 2:
        return _none(D)
    rows = np.arange(D.shape[0])
    j = _argmin(D, 1, last)
    best = D[rows, j]
    rest = D.astype(np.float64)
    rest[rows, j] = np.inf
    second = rest.min(axis=1)
    q = np.nonzero(best.astype(np.float64) < ratio * second)[0]
    return _ordered(q, j[q], best[q], max_matches)


def match_hamming(d1, d2, max_matches, last=False):
    return cross_check(hamming_matrix(d1, d2), max_matches, last)


def match_hamming_ratio(d1, d2, ratio, max_matches, last=False):
    return ratio_test(hamming_matrix(d1, d2), ratio, max_matches, last)


def match_l2(d1, d2, max_matches, last=False):
    return cross_check(l2_matrix(d1, d2), max_matches, last)


def match_l2_ratio(d1, d2, ratio, max_matches, last=False):
    return ratio_test(l2_matrix(d1, d2), ratio, max_matches, last)
