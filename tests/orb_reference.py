"""Independent NumPy model of the ORB stages behind FAST, as the reference configures cv2.ORB_create: 12 levels, scale
factor 1.1f, edge threshold 31, patch size 31, HARRIS_SCORE, FAST threshold 15 (OpenCV 4.x features2d/orb.cpp, imgproc
resize.cpp, features2d/keypoint.cpp).  Written from those definitions, not from oracle/orb_oracle.c or the kernels, and it
never calls either: whole-array operations, integer stages in exact int64, float stages in float64 where the
implementations use f32.  tests/orb_stage_checks.py compares an implementation with it stage by stage.

What is taken as data: the 256 rBRIEF test pairs (oracle/orb_pattern.inc, pinned by test_oracle_cpu.py::test_pattern_table).

cv2 conventions the model states explicitly (each is cv2's own, read off orb.cpp):
- layout: scale_l = (float)pow((double)1.1f, l); size = cvRound(cols * (1.f / scale_l)) in f32; quotas from the f32
  geometric series with factor (float)(1 / (double)1.1f), cvRound per level, the remainder to the last level.  These are
  the only places where the model uses f32 itself: sizes and quotas are integers decided by f32 values;
- Harris: k is the f32 constant 0.04f; block 7x7 of 3x3 Sobel responses (1 2 1 weights), scale 1 / (4 * 7 * 255);
- patch disc: half-width per row cvRound(sqrt(15^2 - v^2)) for the rows below the diagonal, mirrored above it, i.e. a
  pixel is inside when the larger of |u|, |v| is at most cvRound(sqrt(225 - min(|u|, |v|)^2)): 749 pixels, row
  half-widths 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3;
- descriptor: pattern point rotated by the keypoint angle, each coordinate rounded half to even (cvRound), bit =
  blurred(p0) < blurred(p1), bit b of byte i from pair 8 i + b;
- retainBest(n): nothing is dropped when the list holds at most n; otherwise everything >= the n-th best stays."""
import os
import re

import numpy as np

NLEVELS = 12
EDGE = 31
HALF_PATCH = 15
FAST_THRESHOLD = 15
HARRIS_BLOCK = 7
HARRIS_K = float(np.float32(0.04))
HARRIS_SCALE4 = (1.0 / (4 * HARRIS_BLOCK * 255.0)) ** 4


# ------------------------------------------------------------------------------------------ layout
def layout(W, H, nfeatures):
    """(scale[12] f32, w[12], h[12], quota[12])"""
    sf = np.float64(np.float32(1.1))
    scale = np.power(sf, np.arange(NLEVELS, dtype=np.float64)).astype(np.float32)
    inv = np.float32(1) / scale
    w = np.rint((np.float32(W) * inv).astype(np.float64)).astype(np.int64)
    h = np.rint((np.float32(H) * inv).astype(np.float64)).astype(np.int64)
    factor = np.float32(1.0 / sf)
    nd = np.float32(nfeatures) * (np.float32(1) - factor) / (np.float32(1) - np.float32(np.float64(factor) ** NLEVELS))
    quota = np.zeros(NLEVELS, np.int64)
    for l in range(NLEVELS - 1):
        quota[l] = int(np.rint(np.float64(nd)))
        nd = np.float32(nd * factor)
    quota[-1] = max(nfeatures - int(quota[:-1].sum()), 0)
    return scale, w, h, quota


def split_levels(flat, w, h):
    """packed pyramid (levels back to back) -> list of (h_l, w_l) views"""
    out, off = [], 0
    for wl, hl in zip(w, h):
        out.append(flat[off:off + wl * hl].reshape(hl, wl))
        off += int(wl * hl)
    assert off == flat.size, (off, flat.size)
    return out


# ------------------------------------------------------------------------------------------ resize
def _axis_map(src, dst):
    """pixel-centre map of cv2.resize with edge clamping: left tap, right tap, weight of the right tap"""
    f = np.clip((np.arange(dst) + 0.5) * (src / dst) - 0.5, 0.0, src - 1.0)
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, src - 1), f - i0


def resize_linear(prev, w, h):
    """one level from the previous one: (unrounded float64 bilinear value, max - min of the four taps)"""
    p = prev.astype(np.float64)
    y0, y1, b = _axis_map(prev.shape[0], h)
    x0, x1, a = _axis_map(prev.shape[1], w)
    t = np.stack([p[np.ix_(y0, x0)], p[np.ix_(y0, x1)], p[np.ix_(y1, x0)], p[np.ix_(y1, x1)]])
    a = a[None, :]; b = b[:, None]
    val = (1 - b) * ((1 - a) * t[0] + a * t[1]) + b * ((1 - a) * t[2] + a * t[3])
    return val, t.max(axis=0) - t.min(axis=0)


# ------------------------------------------------------------------------------------------ Harris
def _box_sum(v, r):
    """sum over the (2r+1)^2 block around every pixel at least r from the border (int64, exact); output index = pixel - r"""
    c = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
    c[1:, 1:] = v.cumsum(0).cumsum(1)
    n = 2 * r + 1
    return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]


def harris_sums(level):
    """a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7x7 block, for every pixel at least 4 from the border.
    Returned arrays are indexed [y - 4, x - 4]."""
    p = level.astype(np.int64)
    ix = (p[1:-1, 2:] - p[1:-1, :-2]) * 2 + (p[:-2, 2:] - p[:-2, :-2]) + (p[2:, 2:] - p[2:, :-2])
    iy = (p[2:, 1:-1] - p[:-2, 1:-1]) * 2 + (p[2:, :-2] - p[:-2, :-2]) + (p[2:, 2:] - p[:-2, 2:])
    r = HARRIS_BLOCK // 2
    return _box_sum(ix * ix, r), _box_sum(iy * iy, r), _box_sum(ix * iy, r)


def harris_at(level, x, y):
    """(response float64, magnitude float64, a, b, c int64) at the pixels (x, y) of a level"""
    A, B, C = harris_sums(level)
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64)
    a, b, c = A[y - 4, x - 4], B[y - 4, x - 4], C[y - 4, x - 4]
    return harris_eval(a, b, c) + (a, b, c)


def harris_eval(a, b, c):
    fa, fb, fc = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    s2 = HARRIS_K * (fa + fb) ** 2
    return (fa * fb - fc * fc - s2) * HARRIS_SCALE4, (fa * fb + fc * fc + s2) * HARRIS_SCALE4


# ------------------------------------------------------------------------------------------ angle
def patch_disc():
    """bool [31, 31], index [v + 15, u + 15]: the pixels of the radius-15 orientation patch"""
    g = np.abs(np.arange(-HALF_PATCH, HALF_PATCH + 1))
    lo = np.minimum(g[:, None], g[None, :]); hi = np.maximum(g[:, None], g[None, :])
    d = hi <= np.rint(np.sqrt(np.maximum(HALF_PATCH ** 2 - lo.astype(np.float64) ** 2, 0.0)))
    assert np.array_equal(d, d.T) and np.array_equal(d, d[::-1]) and np.array_equal(d, d[:, ::-1])
    return d


def _patches(level, x, y, r):
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64)
    o = np.arange(-r, r + 1)
    return level[(y[:, None] + o[None, :])[:, :, None], (x[:, None] + o[None, :])[:, None, :]]


def moments(level, x, y):
    """(m01, m10) int64 over the disc around every (x, y)"""
    p = _patches(level, x, y, HALF_PATCH).astype(np.int64)
    d = patch_disc().astype(np.int64)
    o = np.arange(-HALF_PATCH, HALF_PATCH + 1, dtype=np.int64)
    m10 = (p * (d * o[None, :])[None]).sum(axis=(1, 2))
    m01 = (p * (d * o[:, None])[None]).sum(axis=(1, 2))
    return m01, m10


def angle_deg(m01, m10):
    a = np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64))) % 360.0
    return np.where((m01 == 0) & (m10 == 0), 0.0, a)


# ------------------------------------------------------------------------------------------ blur
def gauss_taps():
    g = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / (2 * 2.0 ** 2))
    return g / g.sum()


def blur(level):
    """GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) in float64, unrounded"""
    g = gauss_taps()
    h, w = level.shape
    p = np.pad(level.astype(np.float64), 3, mode="reflect")
    rows = sum(g[k] * p[:, k:k + w] for k in range(7))
    return sum(g[k] * rows[k:k + h] for k in range(7))


# ------------------------------------------------------------------------------------------ descriptor
def load_pattern():
    """the 256 test pairs (x0, y0, x1, y1) as data"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "orb_pattern.inc")
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    v = np.array([int(t) for t in re.findall(r"-?\d+", text)], np.int64)
    assert v.size == 1024, v.size
    return v.reshape(256, 4)


def descriptor_bits(blurred, x, y, angle):
    """bits [n, 256] (0 / 1) and, per bit, the smallest distance of its four rotated coordinates to a half-integer.
    blurred: u8 level; x, y: level pixels; angle: degrees."""
    pat = load_pattern().astype(np.float64)
    t = np.radians(np.asarray(angle, np.float64))[:, None]
    cs, sn = np.cos(t), np.sin(t)
    coords = []
    for k in (0, 2):
        px, py = pat[None, :, k], pat[None, :, k + 1]
        coords += [px * cs - py * sn, px * sn + py * cs]
    coords = np.stack(coords)                                     # [4, n, 256]: x0, y0, x1, y1
    margin = np.abs(coords - np.floor(coords) - 0.5).min(axis=0)
    r = np.rint(coords).astype(np.int64)
    x = np.asarray(x, np.int64)[:, None]; y = np.asarray(y, np.int64)[:, None]
    t0 = blurred[y + r[1], x + r[0]].astype(np.int64)
    t1 = blurred[y + r[3], x + r[2]].astype(np.int64)
    return (t0 < t1).astype(np.uint8), margin


def pack_bits(bits):
    return np.packbits(bits.reshape(len(bits), 32, 8), axis=2, bitorder="little").reshape(len(bits), 32)


def unpack_bits(desc):
    return np.unpackbits(np.asarray(desc, np.uint8).reshape(len(desc), 32, 1), axis=2, bitorder="little").reshape(len(desc), 256)


# ------------------------------------------------------------------------------------------ selection
def band_corners(nms):
    """(x, y, FAST score) of the non-zero entries of an NMS map inside the 31-px band"""
    h, w = nms.shape
    m = np.zeros_like(nms, bool)
    if w > 2 * EDGE and h > 2 * EDGE:
        m[EDGE:h - EDGE, EDGE:w - EDGE] = nms[EDGE:h - EDGE, EDGE:w - EDGE] > 0
    y, x = np.nonzero(m)
    return x, y, nms[y, x].astype(np.int64)


def kth_best(v, k):
    """the k-th largest value (k >= 1, k <= len)"""
    return np.partition(v, len(v) - k)[len(v) - k]


def keep_by_score(score, n):
    """retainBest(n) as a set: mask of the entries >= the n-th best; everything when there are at most n"""
    if n <= 0:
        return np.zeros(len(score), bool)
    if len(score) <= n:
        return np.ones(len(score), bool)
    return score >= kth_best(score, n)


def select(level, nms, q):
    """the level's keypoints as cv2 selects them: corners with FAST score >= the 2q-th best, of those the ones with
    Harris response >= the q-th best.  Returns a dict with the stage-1 survivors (x, y), their float64 response,
    magnitude and integer sums, and the stage-2 mask."""
    x, y, s = band_corners(nms)
    k1 = keep_by_score(s, 2 * q)
    x, y = x[k1], y[k1]
    if len(x):
        resp, mag, a, b, c = harris_at(level, x, y)
    else:
        resp = mag = np.zeros(0); a = b = c = np.zeros(0, np.int64)
    return {"x": x, "y": y, "resp": resp, "mag": mag, "a": a, "b": b, "c": c, "keep": keep_by_score(resp, q),
            "n_corners": len(s)}
