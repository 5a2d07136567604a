"""A plain float64 model of OpenCV 4.x SIFT (features2d sift.dispatch.cpp / sift.simd.hpp), stage by stage.

Written from the algorithm (nOctaveLayers 3, contrastThreshold 0.04, edgeThreshold 10, sigma 1.6, firstOctave -1), not
from oracle/sift_oracle.c, and with exact np.exp / np.arctan2 / np.cos / np.sin: it shares none of the project's own
conventions (summation trees, det_expf, the fastAtan2 polynomial).  Every stage takes its input explicitly, so a test can
feed it the upstream output of the implementation under test and compare one stage at a time with tight tolerances.

Besides each stage's value, the stages that end in a discrete decision (round, compare) return how far the float64
value sits from that decision, so a test can set aside the few cases an f32 implementation may legitimately decide the
other way.  NumPy only, plus the real std::nth_element through tests/native/retain_best_host.cpp for retainBest.
"""
import ctypes as C
import os
import subprocess

import numpy as np

NOL = 3                      # nOctaveLayers
SIGMA = 1.6
BORDER = 5                   # SIFT_IMG_BORDER
CONTRAST = 0.04
EDGE = 10.0
ORI_BINS = 36
ORI_RADIUS = 4.5             # SIFT_ORI_RADIUS (x scale)
ORI_SIG = 1.5                # SIFT_ORI_SIG_FCTR
ORI_PEAK = 0.8
DESCR_WIDTH = 4
DESCR_BINS = 8
DESCR_SCL = 3.0
DESCR_MAG_THR = 0.2
INT_DESCR_FCTR = 512.0
FLT_EPSILON = float(np.finfo(np.float32).eps)
SEED_THRESHOLD = np.floor(0.5 * CONTRAST / NOL * 255)          # = 1

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])


def cv_round(v):
    """cvRound: round half to even (lrint)"""
    return np.rint(v).astype(np.int64)


# ------------------------------------------------------------------------------------------ geometry
def n_octaves(W, H):
    return int(cv_round(np.log2(min(2 * W, 2 * H)) - 2)) + 1


def octave_sizes(W, H):
    w, h, out = 2 * W, 2 * H, []
    for _ in range(n_octaves(W, H)):
        out.append((w, h))
        w, h = w // 2, h // 2
    return out


def split_pyramid(flat, W, H):
    """The implementation's flat Gaussian pyramid (octave-major, NOL + 3 levels of h x w each) -> list of (6, h, w)."""
    out, off = [], 0
    for w, h in octave_sizes(W, H):
        n = (NOL + 3) * w * h
        out.append(np.asarray(flat[off:off + n]).reshape(NOL + 3, h, w))
        off += n
    assert off == len(flat)
    return out


# ------------------------------------------------------------------------------------------ Gaussian pyramid
def initial_sigma():
    """createInitialImage: the input is assumed blurred by 0.5, doubled by the 2x upsample"""
    return np.sqrt(max(SIGMA ** 2 - 0.5 ** 2 * 4, 0.01))


def level_sigmas():
    """buildGaussianPyramid: sig[i] = sqrt((k^i sigma)^2 - (k^(i-1) sigma)^2), k = 2^(1/nOctaveLayers)"""
    k = 2.0 ** (1.0 / NOL)
    return [None] + [np.sqrt((k ** i * SIGMA) ** 2 - (k ** (i - 1) * SIGMA) ** 2) for i in range(1, NOL + 3)]


def kernel_size(sigma):
    return int(cv_round(sigma * 8 + 1)) | 1


def gaussian_kernel(sigma):
    ks = kernel_size(sigma)
    x = np.arange(ks) - (ks - 1) * 0.5
    t = np.exp(-0.5 * x * x / (sigma * sigma))
    return t / t.sum()


def blur(img, sigma):
    """GaussianBlur, separable, BORDER_REFLECT_101 (numpy's 'reflect' mode), float64"""
    k = gaussian_kernel(sigma)
    r = len(k) // 2
    img = np.asarray(img, np.float64)
    p = np.pad(img, ((0, 0), (r, r)), mode="reflect") if img.shape[1] > 1 else np.repeat(img, 2 * r + 1, 1)
    row = sum(k[i] * p[:, i:i + img.shape[1]] for i in range(len(k)))
    p = np.pad(row, ((r, r), (0, 0)), mode="reflect") if img.shape[0] > 1 else np.repeat(row, 2 * r + 1, 0)
    return sum(k[i] * p[i:i + img.shape[0]] for i in range(len(k)))


def upsample2x(img):
    """resize(fx = fy = 2, INTER_LINEAR): src = (dst + 0.5) * 0.5 - 0.5, clamped to the image at both ends"""
    img = np.asarray(img, np.float64)
    H, W = img.shape

    def axis(n_src):
        s = (np.arange(2 * n_src) + 0.5) * 0.5 - 0.5
        s0 = np.floor(s).astype(np.int64)
        f = s - s0
        lo, hi = np.clip(s0, 0, n_src - 1), np.clip(s0 + 1, 0, n_src - 1)
        f = np.where(s0 < 0, 0.0, np.where(s0 >= n_src - 1, 0.0, f))
        return lo, hi, f

    ylo, yhi, fy = axis(H)
    xlo, xhi, fx = axis(W)
    rows = img[ylo] * (1 - fy)[:, None] + img[yhi] * fy[:, None]
    return rows[:, xlo] * (1 - fx)[None] + rows[:, xhi] * fx[None]


def octave0_level0(img_u8):
    return blur(upsample2x(img_u8), initial_sigma())


def next_level(prev_level, i):
    """level i of an octave from level i - 1 (of the implementation under test)"""
    return blur(prev_level, level_sigmas()[i])


def octave_base(level3_prev):
    """base of octave o > 0: level nOctaveLayers of octave o - 1, every second pixel from (0, 0) (INTER_NEAREST)"""
    w, h = level3_prev.shape[1] // 2, level3_prev.shape[0] // 2
    return np.asarray(level3_prev)[0:2 * h:2, 0:2 * w:2]


# ------------------------------------------------------------------------------------------ DoG seeds + adjustLocalExtrema
def dog(gauss_oct):
    """D_i = G_{i+1} - G_i in the pyramid's own precision (an f32 pyramid gives the implementation's DoG bit for bit)"""
    g = np.asarray(gauss_oct)
    return (g[1:] - g[:-1])


def find_seeds(dog_oct):
    """findScaleSpaceExtrema's candidate test: |v| > threshold and >= / <= all 26 neighbours, layers 1..nOctaveLayers,
    SIFT_IMG_BORDER pixels kept clear.  Returns (layer, row, col) arrays in raster order per layer."""
    D = np.asarray(dog_oct)
    _, h, w = D.shape
    if w <= 2 * BORDER or h <= 2 * BORDER:
        return np.zeros((3, 0), np.int64)
    out = []
    for i in range(1, NOL + 1):
        v = D[i, BORDER:h - BORDER, BORDER:w - BORDER]
        ismax = v > SEED_THRESHOLD
        ismin = v < -SEED_THRESHOLD
        for dl in (-1, 0, 1):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    nb = D[i + dl, BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                    ismax &= v >= nb
                    ismin &= v <= nb
        r, c = np.nonzero(ismax | ismin)
        out.append(np.stack([np.full(len(r), i), r + BORDER, c + BORDER]))
    return np.concatenate(out, 1)


def _derivs(D, l, r, c):
    """first derivatives and Hessian at integer (l, r, c), scaled like adjustLocalExtrema (1/255, 1/2, 1/4)"""
    s = 1.0 / 255
    v = D[l, r, c]
    dD = np.stack([(D[l, r, c + 1] - D[l, r, c - 1]) * s * 0.5,
                   (D[l, r + 1, c] - D[l, r - 1, c]) * s * 0.5,
                   (D[l + 1, r, c] - D[l - 1, r, c]) * s * 0.5], -1)
    dxx = (D[l, r, c + 1] + D[l, r, c - 1] - 2 * v) * s
    dyy = (D[l, r + 1, c] + D[l, r - 1, c] - 2 * v) * s
    dss = (D[l + 1, r, c] + D[l - 1, r, c] - 2 * v) * s
    dxy = (D[l, r + 1, c + 1] - D[l, r + 1, c - 1] - D[l, r - 1, c + 1] + D[l, r - 1, c - 1]) * s * 0.25
    dxs = (D[l + 1, r, c + 1] - D[l + 1, r, c - 1] - D[l - 1, r, c + 1] + D[l - 1, r, c - 1]) * s * 0.25
    dys = (D[l + 1, r + 1, c] - D[l + 1, r - 1, c] - D[l - 1, r + 1, c] + D[l - 1, r - 1, c]) * s * 0.25
    Hm = np.stack([np.stack([dxx, dxy, dxs], -1), np.stack([dxy, dyy, dys], -1), np.stack([dxs, dys, dss], -1)], -2)
    return v, dD, Hm, (dxx, dyy, dxy)


def _half_distance(x):
    """distance of x to the nearest half-integer: cvRound and the |offset| < 0.5 test flip there"""
    return np.abs(np.abs(x - np.floor(x)) - 0.5)


def adjust_local_extrema(dog_oct, seeds):
    """adjustLocalExtrema for every seed at once (<= 5 Newton steps on the f64 DoG).

    Returns a dict of arrays over the seeds that survive: final integer (l, r, c), offsets (xi, xr, xc), contrast, and
    the margins of every decision taken on the way -- 'off_margin' (the smallest distance of any offset, at any step, to a
    half-integer), 'contr_margin' and 'edge_margin' (relative distances of the contrast and edge tests to their
    thresholds), also for the seeds that were dropped ('dropped_margin'), so that a test can tell a near-threshold drop
    from a real one."""
    D = np.asarray(dog_oct, np.float64)
    _, h, w = D.shape
    l, r, c = (np.array(a, np.int64) for a in seeds)
    n = len(l)
    alive = np.ones(n, bool)
    conv = np.zeros(n, bool)
    off_m = np.full(n, np.inf)
    x = np.zeros((n, 3))
    for _ in range(5):
        a = np.nonzero(alive & ~conv)[0]
        if len(a) == 0:
            break
        _, dD, Hm, _ = _derivs(D, l[a], r[a], c[a])
        det = np.linalg.det(Hm)
        sing = np.abs(det) < 1e-30
        Hs = np.where(sing[:, None, None], np.eye(3), Hm)
        X = np.linalg.solve(Hs, dD[..., None])[..., 0]
        X[sing] = 0
        xa = -X                                          # (xc, xr, xi)
        x[a] = xa
        off_m[a] = np.minimum(off_m[a], _half_distance(xa).min(1))
        done = np.all(np.abs(xa) < 0.5, 1)
        conv[a[done]] = True
        mv = a[~done]
        xm = xa[~done]
        if np.any(np.abs(xm) > 2 ** 31 / 3):
            big = np.any(np.abs(xm) > 2 ** 31 / 3, 1)
            alive[mv[big]] = False
            mv, xm = mv[~big], xm[~big]
        c[mv] += cv_round(xm[:, 0]); r[mv] += cv_round(xm[:, 1]); l[mv] += cv_round(xm[:, 2])
        out = (l[mv] < 1) | (l[mv] > NOL) | (c[mv] < BORDER) | (c[mv] >= w - BORDER) | (r[mv] < BORDER) | (r[mv] >= h - BORDER)
        alive[mv[out]] = False
    ok = alive & conv
    k = np.nonzero(ok)[0]
    v, dD, _, (dxx, dyy, dxy) = _derivs(D, l[k], r[k], c[k])
    contr = v / 255 + 0.5 * np.einsum("ij,ij->i", dD, x[k])
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    pass_c = np.abs(contr) * NOL >= CONTRAST
    pass_e = (det > 0) & (tr * tr * EDGE < (EDGE + 1) ** 2 * det)
    contr_m = np.abs(np.abs(contr) * NOL - CONTRAST) / CONTRAST
    edge_m = np.abs((EDGE + 1) ** 2 * det - tr * tr * EDGE) / np.maximum((EDGE + 1) ** 2 * np.abs(det) + tr * tr * EDGE, 1e-300)
    keep = pass_c & pass_e
    kk = k[keep]
    # seeds that were dropped, with the margin of the decision that dropped them (inf when it was no close call)
    drop_m = np.where(~pass_c, contr_m, np.where(~pass_e, edge_m, np.inf))[~keep]
    return {"l": l[kk], "r": r[kk], "c": c[kk], "xc": x[kk, 0], "xr": x[kk, 1], "xi": x[kk, 2], "contr": contr[keep],
            "off_margin": off_m[kk], "contr_margin": contr_m[keep], "edge_margin": edge_m[keep],
            "dropped": np.stack([l[k[~keep]], r[k[~keep]], c[k[~keep]]]), "dropped_margin": np.minimum(drop_m, off_m[k[~keep]]),
            "lost_margin": off_m[~ok & (off_m < np.inf)]}


def keypoint_fields(o, ref):
    """pt, size, packed octave and response of refined extrema in octave o (internal index, 0 = the 2x upsampled one)"""
    s = 2.0 ** o
    return {"x": (ref["c"] + ref["xc"]) * s, "y": (ref["r"] + ref["xr"]) * s,
            "size": SIGMA * 2.0 ** ((ref["l"] + ref["xi"]) / NOL) * s * 2,
            "octave": o + (ref["l"] << 8) + (cv_round((ref["xi"] + 0.5) * 255) << 16),
            "response": np.abs(ref["contr"])}


# ------------------------------------------------------------------------------------------ orientation
def orientation_hist(img, c, r, s, atan_err_deg=0.0):
    """calcOrientationHist at integer (r, c) of a level image, scl_octv = s: radius round(4.5 s), Gaussian sigma 1.5 s,
    36 bins by round(36/360 * angle), then [1 4 6 4 1]/16 smoothing with wrap.  Also returns, for every sample whose angle
    lies within atan_err_deg of a bin edge, the change of the smoothed histogram if that sample went to the other bin."""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    radius = int(cv_round(ORI_RADIUS * s))
    sigma = ORI_SIG * s
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = r + i, c + j
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    wgt = np.exp(-(i * i + j * j) / (2 * sigma * sigma))
    ang = np.degrees(np.arctan2(dy, dx)) % 360.0
    mag = np.hypot(dx, dy) * wgt
    fb = ORI_BINS / 360.0 * ang
    b = cv_round(fb) % ORI_BINS
    amb = np.nonzero((_half_distance(fb) < atan_err_deg * ORI_BINS / 360.0) & (mag > 0))[0]
    alt = np.where(fb[amb] - np.floor(fb[amb]) < 0.5, b[amb] + 1, b[amb] - 1) % ORI_BINS

    def smooth(t):
        return (np.roll(t, 2) + np.roll(t, -2)) / 16 + (np.roll(t, 1) + np.roll(t, -1)) * 4 / 16 + t * 6 / 16
    hist = smooth(np.bincount(b, mag, ORI_BINS))
    flips = []
    for k, a in zip(amb, alt):
        t = np.zeros(ORI_BINS)
        t[b[k]] -= mag[k]
        t[a] += mag[k]
        flips.append(smooth(t))
    return hist, flips


def orientation_peaks(hist):
    """peaks > both neighbours and >= 0.8 max, parabolic refinement; angle = 360 - 10 * bin, 360 -> 0.  Returns the angles
    and the smallest relative margin of the peak decisions (neighbour comparisons and the 0.8 max threshold)."""
    mx = hist.max()
    thr = mx * ORI_PEAK
    lf, rt = np.roll(hist, 1), np.roll(hist, -1)
    is_pk = (hist > lf) & (hist > rt) & (hist >= thr)
    cand = (hist >= thr * 0.999)            # bins that could be peaks near the threshold
    scale = max(mx, 1e-300)
    m = np.concatenate([np.abs(hist - lf)[cand], np.abs(hist - rt)[cand], np.abs(hist - thr)[cand]]) / scale
    angles = []
    for j in np.nonzero(is_pk)[0]:
        bn = j + 0.5 * (lf[j] - rt[j]) / (lf[j] - 2 * hist[j] + rt[j])
        bn = bn + ORI_BINS if bn < 0 else bn - ORI_BINS if bn >= ORI_BINS else bn
        a = 360.0 - 360.0 / ORI_BINS * bn
        angles.append(0.0 if abs(a - 360.0) < FLT_EPSILON else a)
    return np.array(angles), (m.min() if len(m) else np.inf)


def orientations(img, c, r, s, atan_err_deg=0.0):
    """angles at one location, and the reference's confidence: (angles, tolerance per angle in degrees, margin).
    An implementation may bin each near-edge sample either way.  The tolerance bounds the effect of any subset of those
    choices to first order: the sum over the samples of the angle change when that one sample alone is flipped (and at
    least the change when all are).  None when a flip changes which bins are peaks (a near-decision to be set aside)."""
    h, flips = orientation_hist(img, c, r, s, atan_err_deg)
    a1, margin = orientation_peaks(h)
    tol, spread_all = np.zeros(len(a1)), np.zeros(len(a1))
    for k, dh in enumerate(flips + ([sum(flips)] if len(flips) > 1 else [])):
        a2, m2 = orientation_peaks(h + dh)
        if len(a2) != len(a1):
            return a1, None, 0.0
        margin = min(margin, m2)
        d = np.abs((a1 - a2 + 180) % 360 - 180)
        if k < len(flips):
            tol += d
        else:
            spread_all = d
    return a1, np.maximum(tol, spread_all), margin


# ------------------------------------------------------------------------------------------ descriptor
def descriptor(img, ptx, pty, ori, scl):
    """calcSIFTDescriptor (d = 4, n = 8) at octave coordinates (ptx, pty), ori = 360 - angle (degrees), scl = the
    keypoint's size * scale * 0.5.  Returns the 128 values as u8-rounded float64."""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    d, n = DESCR_WIDTH, DESCR_BINS
    px, py = int(cv_round(ptx)), int(cv_round(pty))
    cos_t, sin_t = np.cos(np.radians(ori)), np.sin(np.radians(ori))
    hist_width = DESCR_SCL * scl
    radius = int(cv_round(hist_width * np.sqrt(2) * (d + 1) * 0.5))
    radius = min(radius, int(np.sqrt(float(w) * w + float(h) * h)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    c_rot = j * cos_t - i * sin_t
    r_rot = j * sin_t + i * cos_t
    rbin = r_rot + d / 2 - 0.5
    cbin = c_rot + d / 2 - 0.5
    y, x = py + i, px + j
    ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    rbin, cbin, c_rot, r_rot, y, x = rbin[ok], cbin[ok], c_rot[ok], r_rot[ok], y[ok], x[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    wgt = np.exp(-(c_rot ** 2 + r_rot ** 2) / (d * d * 0.5))
    o = np.degrees(np.arctan2(dy, dx)) % 360.0
    mag = np.hypot(dx, dy) * wgt
    obin = (o - ori) * (n / 360.0)
    r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    o0 = o0 % n
    hist = np.zeros((d + 2, d + 2, n + 2))
    for dr, wr in ((0, 1 - rbin), (1, rbin)):
        for dc, wc in ((0, 1 - cbin), (1, cbin)):
            for do, wo in ((0, 1 - obin), (1, obin)):
                np.add.at(hist, (r0 + 1 + dr, c0 + 1 + dc, o0 + do), mag * wr * wc * wo)
    hist[:, :, 0] += hist[:, :, n]
    hist[:, :, 1] += hist[:, :, n + 1]
    v = hist[1:d + 1, 1:d + 1, :n].reshape(-1)
    thr = np.linalg.norm(v) * DESCR_MAG_THR
    v = np.minimum(v, thr)
    v = v * (INT_DESCR_FCTR / max(np.linalg.norm(v), FLT_EPSILON))
    return np.clip(np.rint(v), 0, 255)


# ------------------------------------------------------------------------------------------ post-processing
def unpack_octave(octave):
    """(octave index with -1 for the upsampled one, layer, xi byte) of cv2's packed KeyPoint.octave"""
    octave = np.asarray(octave, np.int64)
    o = octave & 255
    return np.where(o >= 128, o - 256, o), (octave >> 8) & 255, (octave >> 16) & 255


def lessthan_order(kps):
    """KeyPoint_LessThan: x, y ascending, size descending, angle ascending, response descending, octave descending"""
    return np.lexsort((-kps["octave"].astype(np.int64), -kps["response"].astype(np.float64), kps["angle"],
                       -kps["size"].astype(np.float64), kps["y"], kps["x"]))


def remove_duplicated_sorted(kps):
    """sort by KeyPoint_LessThan, then drop entries equal to their predecessor in pt, size and angle"""
    s = kps[lessthan_order(kps)]
    if len(s) < 2:
        return s
    same = (s["x"][1:] == s["x"][:-1]) & (s["y"][1:] == s["y"][:-1]) & (s["size"][1:] == s["size"][:-1]) & \
           (s["angle"][1:] == s["angle"][:-1])
    return s[np.concatenate([[True], ~same])]


_RB = None
_RB_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "retain_best_host.cpp")
_RB_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "build", "libretain_best_sift_model.so")


def _rb():
    global _RB
    if _RB is None:
        os.makedirs(os.path.dirname(_RB_OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-o", _RB_OUT, _RB_SRC])
        _RB = C.CDLL(_RB_OUT)
    return _RB


def retain_best(kps, n_points, runtime="libstdc++"):
    """KeyPointsFilter::retainBest: std::nth_element (response greater) + std::partition (>= the n-th), no sort after.
    runtime "libstdc++" runs the real library; "msvc" the MSVC STL selection (retain_best_emul.h)."""
    if n_points <= 0 or len(kps) <= n_points:
        return kps
    resp = np.ascontiguousarray(kps["response"], np.float32)
    n = len(resp)
    a = np.zeros(n, np.int32); b = np.zeros(n, np.int32); na = C.c_int(0); nb = C.c_int(0)
    _rb().rb_run(resp.ctypes.data_as(C.c_void_p), n, int(n_points), 0 if runtime == "libstdc++" else 1,
                 a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(na), C.byref(nb))
    return kps[a[:na.value]] if runtime == "libstdc++" else kps[b[:nb.value]]


def rescale_first_octave(kps):
    """firstOctave = -1: pt and size x 0.5, octave byte - 1 (mod 256)"""
    out = kps.copy()
    out["x"] = kps["x"] * 0.5; out["y"] = kps["y"] * 0.5; out["size"] = kps["size"] * 0.5
    oc = kps["octave"].astype(np.int64)
    out["octave"] = ((oc & ~255) | ((oc - 1) & 255)).astype(np.int32)
    return out


def unscale_first_octave(kps):
    """inverse of rescale_first_octave (exact in f32: powers of two)"""
    out = kps.copy()
    out["x"] = kps["x"] * 2; out["y"] = kps["y"] * 2; out["size"] = kps["size"] * 2
    oc = kps["octave"].astype(np.int64)
    out["octave"] = ((oc & ~255) | ((oc + 1) & 255)).astype(np.int32)
    return out


def post_process(kps_unscaled, nfeatures=0, runtime="libstdc++"):
    """removeDuplicatedSorted, retainBest(nfeatures), firstOctave rescale -- in SIFT_Impl::detectAndCompute's order"""
    return rescale_first_octave(retain_best(remove_duplicated_sorted(kps_unscaled), nfeatures, runtime))


# ------------------------------------------------------------------------------------------ helpers for tests
def locate(kps):
    """internal octave index (0 = upsampled), layer and integer (r, c) of reported keypoints: c = round(x / 2^octave),
    exact because |offset| < 0.5 and the scalings are powers of two"""
    o, l, xib = unpack_octave(kps["octave"])
    s = np.ldexp(1.0, -o.astype(np.int64))
    return o + 1, l, cv_round(kps["y"].astype(np.float64) * s), cv_round(kps["x"].astype(np.float64) * s), xib
