"""Matched-point families that reach the rare paths of the root chain of the five-point solver (ransac_roots_kernel;
poly_real_roots in oracle/geom_oracle.c): the generic path (leading coefficient trimmed, degree below 10), levels 9 and 10
with more than 8 intervals (two rounds of a group's 8 lanes) and solves with more than 8 roots (a second back-substitution
round).  oracle.poly_counters() says which of them a run took; the floors are asserted in tests/test_oracle_cpu.py.

  A  "grid shift, five points": 256 pairs of M = 5 points on a 16-pixel grid, the second image shifted by 8 pixels in x.
     One solve per pair (M == 5: the solver runs on all points and the models come back stacked).
  B  "grid shift with outliers": 64 pairs of M = 16 such points, the first int(0.3 M) of the second image replaced by
     uniform integer pixels.
  C  "no geometry": 16 pairs of M = 16 unrelated uniform points: RANSAC runs its 1000 iterations.

Every array is drawn pair by pair, in the order written."""
import numpy as np

W, H = 640, 480


def _grid(rng, M):
    p1 = np.stack([16 * rng.integers(0, 40, M), 16 * rng.integers(0, 30, M)], axis=1).astype(np.float32)
    return p1, p1 + np.float32([8, 0])


def family_a():
    rng = np.random.default_rng(5)
    return [_grid(rng, 5) for _ in range(256)]


def family_b():
    rng = np.random.default_rng(5)
    out = []
    for _ in range(64):
        p1, p2 = _grid(rng, 16)
        no = int(0.3 * 16)
        p2[:no] = np.stack([rng.integers(0, W, no), rng.integers(0, H, no)], axis=1)
        out.append((p1, p2))
    return out


def family_c():
    rng = np.random.default_rng(7)
    out = []
    for _ in range(16):
        p1 = (rng.uniform(0, 1, (16, 2)) * [W, H]).astype(np.float32)
        p2 = (rng.uniform(0, 1, (16, 2)) * [W, H]).astype(np.float32)
        out.append((p1, p2))
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c}

# floors on oracle.poly_counters()[1:] (degree below 10, two-round levels, more than 8 roots) over a whole family; None: the
# count must be zero.  About half of what the oracle gives, so a run cannot pass while missing a path.
FLOORS = {"A": (5, 7, None), "B": (6, 18, 3), "C": (None, 70, None)}
