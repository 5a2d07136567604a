"""Seeded descriptor sets for the matcher tests, shared by tests/test_match_model_cpu.py (model against the C oracle) and
tests/test_gpu_match_model.py (kernels against the model).  A case is a name and two uint8 arrays (n1, dim), (n2, dim):
dim = 32 serves the Hamming matchers and ORB bytes under NORM_L2, dim = 128 serves SIFT.  A case list belongs to one
engine of the GPU tests: it fixes the norm, the mode, max_matches and the sizes that reach that engine's launch forms.

What a "mixed" case holds, as far as its sizes allow:
  - random bytes; a third of the train rows are copies of random query rows with 0 to 2 flipped bits, so that many
    matches survive crossCheck and the ratio test, at distances that repeat;
  - an all-zero and an all-ones row on each side and a row one bit away from each: Hamming distances 0, 1, 255 and 256
    occur, and for L2 every dimension of some row pair is 0 against 255 (distance^2 = dim x 65025);
  - equal rows in the train set at indices {3, 4}, {31, 32}, {255, 256} and at the last two, each equal to one query; the
    same in the query set, each equal to one train; three scattered queries equal to one train row.  The duplicated trains
    are best == second for their query: the ratio test drops it for every ratio <= 1.
A "far" case holds nothing but extremes: queries with at most two bits set against trains with at most two bits clear
(Hamming distances 252 .. 256, ties everywhere), or for L2 near-zero against near-255 rows that differ in the last eight
dimensions only: squared distances beyond 2^22, where neighbouring integers share one float32 root.

check_list() asserts, from the model alone, that a list cannot pass vacuously: see there."""
import collections
import functools
import zlib

import numpy as np

from tests import match_model as M

Case = collections.namedtuple("Case", "name desc1 desc2")
# norm: "hamming" | "l2"; mode: "cross" | "ratio"; ratios: the engines' match_ratio values (ratio lists only)
Spec = collections.namedtuple("Spec", "norm dim mode ratios max_matches sizes")

TIE_PAIRS = ((3, 4), (31, 32), (255, 256))


def _flip_bits(rng, rows, most):
    """flip 0 .. most random bits of every row, in place"""
    for r in rows:
        for _ in range(int(rng.integers(0, most + 1))):
            r[rng.integers(0, rows.shape[1])] ^= np.uint8(1 << rng.integers(0, 8))


def _mixed(rng, n1, n2, dim):
    a = rng.integers(0, 256, (n1, dim), dtype=np.uint8); b = rng.integers(0, 256, (n2, dim), dtype=np.uint8)
    if n1 == 1 and n2 == 1:                                # the only pair IS the match: Hamming 256, L2^2 = dim x 65025
        a[:] = 0; b[:] = 255
        return a, b
    if n1 and n2:
        rows = rng.permutation(n2)[:max(n2 // 3, 1)]
        b[rows] = a[rng.integers(0, n1, len(rows))]
        copies = b[rows]; _flip_bits(rng, copies, 2); b[rows] = copies
    free = [list(rng.permutation(np.arange(n))) for n in (n1, n2)]
    d = [a, b]

    def take(side, idx=None):
        """reserve row idx (or any free row) of a side; None if it is taken or absent"""
        if idx is None:
            return int(free[side].pop()) if free[side] else None
        if idx in free[side]:
            free[side].remove(idx)
            return int(idx)
        return None

    for side, n in ((0, n1), (1, n2)):
        if n < 8:
            continue
        zero, ones = (0, 5) if side == 0 else (5, 1)      # query 0 / train 5 are zero, query 5 / train 1 all ones
        for base, fill in ((zero, 0), (ones, 255)):
            r0, r1 = take(side, base), take(side, base + 1)
            d[side][r0] = fill; d[side][r1] = fill
            d[side][r1, rng.integers(0, dim)] ^= np.uint8(1 << rng.integers(0, 8))
    for side, n in ((1, n2), (0, n1)):                     # equal rows on a side, one row of the other side equal to them
        if n < 8:
            continue
        for p, q in TIE_PAIRS + ((n - 2, n - 1),):
            if q >= n or p not in free[side] or q not in free[side]:
                continue
            other = take(1 - side)
            if other is None:
                continue
            take(side, p); take(side, q)
            d[side][p] = d[side][q] = d[1 - side][other] = rng.integers(0, 256, dim, dtype=np.uint8)
    if n1 >= 32 and n2 >= 8:                               # several queries equal one train row
        t = take(1)
        for i in [take(0) for _ in range(3)] if t is not None else []:
            if i is not None:
                a[i] = b[t]
    return a, b


def _far(rng, n1, n2, dim, norm):
    if norm == "hamming":
        a = np.zeros((n1, dim), np.uint8); b = np.full((n2, dim), 255, np.uint8)
        _flip_bits(rng, a, 2); _flip_bits(rng, b, 2)
        if n1 > 2: a[n1 // 2] = 0                          # the exact extremes, away from the ends
        if n2 > 2: b[n2 // 2] = 255
        return a, b
    a = np.zeros((n1, dim), np.uint8); b = np.full((n2, dim), 255, np.uint8)
    a[:, dim - 8:] = rng.integers(0, 4, (n1, 8)); b[:, dim - 8:] = rng.integers(0, 4, (n2, 8))
    if n1 > 2: a[n1 // 2] = 0
    if n2 > 2: b[n2 // 2] = 255
    return a, b


def make_case(tag, n1, n2, dim, norm, kind):
    name = f"{tag}:{kind}:{n1}x{n2}"
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    a, b = _mixed(rng, n1, n2, dim) if kind == "mixed" else _far(rng, n1, n2, dim, norm)
    a.setflags(write=False); b.setflags(write=False)
    return Case(name, a, b)


def _m(*sizes):
    return [(n1, n2, "mixed") for n1, n2 in sizes]


_SMALL = [(0, 7), (7, 0), (1, 1), (1, 40), (40, 1), (31, 33), (32, 32), (33, 31), (129, 160), (160, 129), (160, 160)]
_RATIO_H = [(n1, n2) for n1 in (1, 257, 1500) for n2 in (0, 1, 2, 1023, 1024, 1025, 2049)]
_RATIO_L2 = [(n1, n2) for n1 in (1, 255, 257) for n2 in (0, 1, 2, 255, 256, 257, 512)]
_L2_SMALL = [(127, 1), (1, 129), (128, 33), (33, 128), (129, 96), (96, 127), (128, 288), (288, 129), (127, 512), (512, 512)]
_L2_RING = [(40, 32), (40, 33), (40, 65), (40, 97), (40, 129), (40, 161), (32, 40), (33, 40), (65, 40), (97, 40), (129, 40), (161, 40),
            (0, 9), (9, 0), (1, 1), (2, 3), (5, 2), (8, 8), (17, 12)]


def _l2_lists(dim):
    s = "sift" if dim == 128 else "orb"
    return {
        # kcap 512, one pair per call: the scanned tiles are dealt over 8 workgroups
        f"l2_{s}_448": Spec("l2", dim, "cross", (), 40, _m(*_L2_SMALL) + [(129, 96, "far"), (288, 288, "far")]),
        # kcap 2048, 32 pairs per call: one workgroup walks 1 .. 6 tiles through the prefetch ring
        f"l2_{s}_1984_ring": Spec("l2", dim, "cross", (), 12, _m(*_L2_RING) + [(40, 161, "far"), (97, 40, "far")]),
        # kcap 2048, one pair: 8 chunks of 8 tiles
        f"l2_{s}_1984_full": Spec("l2", dim, "cross", (), 100, _m((2048, 2048)) + [(300, 2048, "far")]),
        f"l2_{s}_448_ratio": Spec("l2", dim, "ratio", (0.8, 1.0), 40, _m(*_RATIO_L2) + [(255, 257, "far")]),
    }


SPECS = {
    # kcap 160: one round of owner tiles
    "ham_96": Spec("hamming", 32, "cross", (), 20, _m(*_SMALL) + [(33, 31, "far"), (160, 129, "far")]),
    # kcap 512: two rounds
    "ham_448": Spec("hamming", 32, "cross", (), 60, _m((100, 100), (255, 257), (257, 255), (256, 256), (512, 512), (0, 100)) + [(257, 255, "far")]),
    # kcap 512, 64 and 65 pairs per call
    "ham_448_many": Spec("hamming", 32, "cross", (), 60, _m((512, 512), *_SMALL) + [(33, 31, "far"), (160, 129, "far")]),
    # kcap 5064: the election words do not fit LDS
    "ham_5000": Spec("hamming", 32, "cross", (), 200, _m((5064, 5000)) + [(64, 64, "far")] + _m(*_SMALL[:8], (64, 50), (50, 64))),
    "ham_8000_ratio": Spec("hamming", 32, "ratio", (0.75, 1.0), 100, _m(*_RATIO_H) + [(257, 6, "far")]),
    **_l2_lists(128), **_l2_lists(32),
    # kcap 16384: the select kernel sorts 16384 keys
    "l2_sift_uncapped": Spec("l2", 128, "cross", (), 40, _m((8200, 70), (70, 8200)) + [(70, 300, "far")]),
}


@functools.lru_cache(maxsize=None)
def cases(list_name):
    spec = SPECS[list_name]
    return tuple(make_case(list_name, n1, n2, spec.dim, spec.norm, kind) for n1, n2, kind in spec.sizes)


def case(list_name, n1, n2, kind="mixed"):
    hit = [c for c in cases(list_name) if c.name == f"{list_name}:{kind}:{n1}x{n2}"]
    assert len(hit) == 1, (list_name, n1, n2, kind)
    return hit[0]


Facts = collections.namedtuple("Facts", "full last int_differs tied")
_expected, _facts = {}, {}


def _solve(list_name, c):
    """The model on one case, computed once: for every ratio of the list (None for crossCheck) the answer with the list's
    max_matches, the untruncated answer and the untruncated last-occurrence answer."""
    spec = SPECS[list_name]
    D = M.hamming_matrix(c.desc1, c.desc2) if spec.norm == "hamming" else M.l2_matrix(c.desc1, c.desc2)
    big = max(len(c.desc1), 1)
    int_differs = False
    if spec.norm == "l2" and D.size:
        S = M.l2_squared_matrix(c.desc1, c.desc2)
        int_differs = bool((S.argmin(1) != D.argmin(1)).any() and (S.argmin(0) != D.argmin(0)).any())
    for r in spec.ratios or (None,):
        run = (lambda mm, last: M.cross_check(D, mm, last)) if r is None else (lambda mm, last: M.ratio_test(D, r, mm, last))
        full = run(big, False)
        _expected[c.name, r] = tuple(x[:spec.max_matches] for x in full)
        two = np.partition(D, 1, axis=1)[:, :2] if r is not None and D.shape[1] >= 2 else np.zeros((0, 2))
        tied = bool((two[:, 0] == two[:, 1]).any())
        _facts[c.name, r] = Facts(full, run(big, True), int_differs, tied)


def expected(list_name, c, ratio=None):
    """(qidx, tidx, dist) of the model for a case of a list, under the list's max_matches; shared, never modified"""
    if (c.name, ratio) not in _expected:
        _solve(list_name, c)
    return _expected[c.name, ratio]


def check_list(list_name):
    """Conditions on the inputs, from the model alone:
      - every case with both sides >= 2 has a model match: a mixed case under every ratio of a ratio list, a far case
        under the largest (its distances are within 2 % of each other: only best < 1.0 x second can hold);
      - some case has more valid matches than max_matches, with equal distances on both sides of the cut;
      - some case changes its answer when every argmin takes the last occurrence: its ties matter.  A ratio list cannot
        have such a case: two equal best trains are best == second, and the query is dropped whichever of them argmin
        names.  There the condition is that some query of some case has best == second;
      - a 128-dimensional L2 list has a case whose integer and float32 argmins differ along both axes."""
    spec = SPECS[list_name]
    cut = ties = collide = False
    for c in cases(list_name):
        for r in spec.ratios or (None,):
            expected(list_name, c, r)
            f = _facts[c.name, r]
            n = len(f.full[0])
            if len(c.desc1) >= 2 and len(c.desc2) >= 2 and (":mixed:" in c.name or r in (None, max(spec.ratios or (0,)))):
                assert n >= 1, (c.name, r, "no model match")
            mm = spec.max_matches
            cut = cut or (n > mm and f.full[2][mm - 1] == f.full[2][mm])
            ties = ties or f.tied or not all(np.array_equal(x, y) for x, y in zip(f.full, f.last))
            collide = collide or f.int_differs
    assert cut, (list_name, "no case is truncated inside a run of equal distances")
    assert ties, (list_name, "no case depends on first-occurrence argmin" if not spec.ratios else "no query with best == second")
    if spec.norm == "l2" and spec.dim == 128:
        assert collide, (list_name, "no case where integer and float32 argmin differ along both axes")
