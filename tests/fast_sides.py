"""numpy model of the FAST kernel's side split (csrc/orb_kernels.hip, fast_nms_kernel) and the test images that exercise
it; shared by tests/test_fast_sides_cpu.py and tests/test_gpu_fast_sides.py.

Phase 1 of the kernel tests the four opposite ring pairs for each side apart: a darker arc (every ring pixel of a 9-arc
below v - thr) needs one pixel of every pair below v - thr, a brighter arc one above v + thr.  Phase 2 then scores only
the side(s) that phase 1 left possible:
    darker   A   = v - min_k max_{arc9(k)} r
    brighter -Bm = max_k min_{arc9(k)} r - v
and keeps s - 1 where s > thr, which equals the full cornerScore max(A, -Bm) wherever that is above thr."""
import numpy as np

# Bresenham circle of radius 3 (fast.cpp), the kernel's CIRC_DX / CIRC_DY
CIRC = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
PAIRS = [(0, 8), (4, 12), (2, 10), (6, 14)]


def ring(lvl):
    """centre values and the 16 ring values of every pixel at least 3 px from the border: v [h-6, w-6], r [16, h-6, w-6]"""
    lvl = np.asarray(lvl, np.int32)
    h, w = lvl.shape
    v = lvl[3:h - 3, 3:w - 3]
    r = np.stack([lvl[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRC])
    return v, r


def sides(v, r, thr=15):
    """phase 1's flags: (darker arc possible, brighter arc possible)"""
    lo = np.max([np.minimum(r[a], r[b]) for a, b in PAIRS], axis=0)
    hi = np.min([np.maximum(r[a], r[b]) for a, b in PAIRS], axis=0)
    return v - lo > thr, hi - v > thr


def one_sided_score_map(lvl, thr=15):
    """the kernel's score map (s - 1 where s > thr, else 0) computed side by side as phase 2 does"""
    lvl = np.ascontiguousarray(lvl, np.uint8)
    v, r = ring(lvl)
    dark, brt = sides(v, r, thr)
    rr = np.concatenate([r, r[:8]])
    arc_max = np.stack([rr[k:k + 9].max(axis=0) for k in range(16)])
    arc_min = np.stack([rr[k:k + 9].min(axis=0) for k in range(16)])
    a = v - arc_max.min(axis=0)
    bneg = arc_min.max(axis=0) - v
    s = np.maximum(np.where(dark, a, 0), np.where(brt, bneg, 0))
    out = np.zeros(lvl.shape, np.uint8)
    out[3:-3, 3:-3] = np.where(s > thr, s - 1, 0)
    return out


def both_sided_stamps(W=640, H=480, seed=5):
    """grey image with stamps whose centre passes BOTH pair tests: ring pixels 0, 2, 4, 6 dark and 8, 10, 12, 14 bright
    (every opposite pair holds one of each); the odd ring pixels are random, so some stamps are corners of either side
    and some are not corners at all"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.uint8)
    for y in range(8, H - 8, 11):
        for x in range(8, W - 8, 11):
            for k, (dx, dy) in enumerate(CIRC):
                if k % 2 == 0:
                    img[y + dy, x + dx] = 20 if k < 8 else 235
                else:
                    img[y + dy, x + dx] = rng.choice([20, 128, 235])
    return img


def blobs_two_sides(W=640, H=480, seed=11):
    """mid-grey image with dark and bright rectangles: corners of each side, plus edges that pass phase 1 but are not
    corners"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.uint8)
    for i in range(120):
        w, h = rng.integers(4, 40, 2)
        x = rng.integers(0, W - w); y = rng.integers(0, H - h)
        img[y:y + h, x:x + w] = rng.integers(0, 60) if i % 2 else rng.integers(200, 256)
    return img


def dense_noise(W=640, H=480, seed=3):
    """full-contrast noise: tiles with far more than 1024 phase-1 candidates and 256 corners"""
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def soft_noise(W=640, H=480, seed=4):
    """low-contrast noise around the threshold: many candidates that are not corners"""
    return np.clip(128 + np.random.default_rng(seed).normal(0, 14, (H, W)), 0, 255).astype(np.uint8)


def side_images():
    return np.stack([both_sided_stamps(), blobs_two_sides(), dense_noise(), soft_noise()])
