"""Float64 NumPy model of guided matching (include/rpe_amd.h, rpe_guided_matches): the mutual nearest neighbour among the
keypoint pairs that pass the Sampson gate of a pose.  Written from the rule in the header, in its operation order (NumPy
evaluates a * b + c * d as two products and a sum, never fused); Hamming distances from np.unpackbits; every election is
an argmin, whose first index is the lowest index on ties.  The distance and gate matrices are built in row blocks, so
the largest capacities (8064 x 8064) stay within a few hundred megabytes."""
import numpy as np

ROW_BLOCK = 1024
NONE = np.iinfo(np.int64).max          # distance of an inadmissible entry: above every real one


def essential(R, t):
    """E = [t]x R, row by row"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    E = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            E[r, c] = t[(r + 1) % 3] * R[(r + 2) % 3, c] - t[(r + 2) % 3] * R[(r + 1) % 3, c]
    return E


def normalise_K(pts_f32, K):
    """(n, 2) f32 pixels -> (n, 2) f64 normalised coordinates on the single-K path"""
    p = np.asarray(pts_f32, np.float32).astype(np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64).reshape(9)
    fx, cx, fy, cy = K[0], K[2], K[4], K[5]
    return np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], 1)


def focal_K(K):
    K = np.asarray(K, np.float64).reshape(9)
    return (K[0] + K[4]) / 2


def thr2_of(gate_px, focal):
    thr = gate_px / focal
    return thr * thr


def query_terms(E, x1):
    """l_0, l_1, l_2 and s1 of every query"""
    x, y = x1[:, 0], x1[:, 1]
    l = [(E[k, 0] * x + E[k, 1] * y) + E[k, 2] for k in range(3)]
    return l[0], l[1], l[2], l[0] * l[0] + l[1] * l[1]


def train_terms(E, x2):
    """s2 of every train"""
    x, y = x2[:, 0], x2[:, 1]
    m = [(E[0, k] * x + E[1, k] * y) + E[2, k] for k in range(2)]
    return m[0] * m[0] + m[1] * m[1]


def hamming_block(d1, d2):
    """(a, 32) u8 x (b, 32) u8 -> (a, b) Hamming distances: |q| + |t| - 2 q.t over the unpacked bits (exact in f32)"""
    b1 = np.unpackbits(np.asarray(d1, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    b2 = np.unpackbits(np.asarray(d2, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return (b1.sum(1)[:, None] + b2.sum(1)[None, :] - 2 * (b1 @ b2.T)).astype(np.int64)


def gate_block(E, x1, x2, thr2):
    """(a, b) bool: the Sampson test of every (query, train) entry; a comparison with a NaN is false"""
    l0, l1, l2, s1 = query_terms(E, x1)
    s2 = train_terms(E, x2)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (l0[:, None] * x2[None, :, 0] + l1[:, None] * x2[None, :, 1]) + l2[:, None]
        return v * v <= thr2 * (s1[:, None] + s2[None, :])


def guided_match(desc1, x1, desc2, x2, R, t, thr2, max_distance=256, max_matches=None):
    """desc (n, 32) u8, x (n, 2) f64 normalised points of the two images -> (qidx, tidx, dist) int arrays: the guided
    matches sorted by (dist, qidx), the first max_matches of them (None: all)"""
    d1 = np.asarray(desc1, np.uint8).reshape(-1, 32); d2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    x1 = np.asarray(x1, np.float64).reshape(-1, 2); x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    n1, n2 = len(d1), len(d2)
    empty = np.zeros(0, np.int64)
    if n1 == 0 or n2 == 0:
        return empty, empty, empty
    E = essential(R, t)
    nnt = np.full(n1, -1, np.int64); nnt_d = np.full(n1, NONE, np.int64)
    nnq = np.full(n2, -1, np.int64); nnq_d = np.full(n2, NONE, np.int64)
    for a in range(0, n1, ROW_BLOCK):
        b = min(n1, a + ROW_BLOCK)
        ham = hamming_block(d1[a:b], d2)
        adm = gate_block(E, x1[a:b], x2, thr2) & (ham <= max_distance)
        masked = np.where(adm, ham, NONE)
        j = masked.argmin(1)                                    # lowest j on ties
        dj = masked[np.arange(b - a), j]
        ok = dj != NONE
        nnt[a:b][ok] = j[ok]; nnt_d[a:b][ok] = dj[ok]
        i = masked.argmin(0)                                    # lowest i of the block on ties; earlier blocks hold lower i
        di = masked[i, np.arange(n2)]
        better = di < nnq_d
        nnq[better] = i[better] + a; nnq_d[better] = di[better]
    q = np.array([i for i in range(n1) if nnt[i] >= 0 and nnq[nnt[i]] == i], np.int64)
    if q.size == 0:
        return empty, empty, empty
    order = np.argsort(nnt_d[q], kind="stable")                 # q ascends: ties keep the lower query first
    q = q[order]
    if max_matches is not None:
        q = q[:max_matches]
    return q, nnt[q], nnt_d[q]


def guided_match_slow(desc1, x1, desc2, x2, R, t, thr2, max_distance=256, max_matches=None):
    """the same rule as plain loops over queries, trains and descriptor bytes (tiny inputs only)"""
    n1, n2 = len(desc1), len(desc2)
    E = essential(R, t)
    ham = [[0] * n2 for _ in range(n1)]
    adm = [[False] * n2 for _ in range(n1)]
    for i in range(n1):
        x, y = float(x1[i][0]), float(x1[i][1])
        l = [(E[k, 0] * x + E[k, 1] * y) + E[k, 2] for k in range(3)]
        s1 = l[0] * l[0] + l[1] * l[1]
        for j in range(n2):
            u, w = float(x2[j][0]), float(x2[j][1])
            m = [(E[0, k] * u + E[1, k] * w) + E[2, k] for k in range(2)]
            s2 = m[0] * m[0] + m[1] * m[1]
            d = 0
            for k in range(32):
                d += bin(int(desc1[i][k]) ^ int(desc2[j][k])).count("1")
            v = (l[0] * u + l[1] * w) + l[2]
            ham[i][j] = d
            adm[i][j] = bool(v * v <= thr2 * (s1 + s2)) and d <= max_distance
    def nearest(cands):
        return min(cands)[1] if cands else -1
    nnt = [nearest([(ham[i][j], j) for j in range(n2) if adm[i][j]]) for i in range(n1)]
    nnq = [nearest([(ham[i][j], i) for i in range(n1) if adm[i][j]]) for j in range(n2)]
    out = sorted((ham[i][nnt[i]], i, nnt[i]) for i in range(n1) if nnt[i] >= 0 and nnq[nnt[i]] == i)
    if max_matches is not None:
        out = out[:max_matches]
    a = np.array(out, np.int64).reshape(-1, 3)
    return a[:, 1], a[:, 2], a[:, 0]
