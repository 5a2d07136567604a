"""Stage-by-stage comparison of an ORB implementation (the CPU oracle or the HIP kernels) with the NumPy model in
tests/orb_reference.py.  Each check feeds the model the implementation's own upstream output (its pyramid, NMS map,
blurred level, f32 angle), so errors do not compound, and returns what it measured: the largest error and the share it
set aside.  An implementation is handed over as a `run` dict, see make_run().

Tolerances, with their derivations (u = 2^-24, the f32 unit roundoff):

- Layout: level sizes, scales (f32 bits) and quotas are exact.
- Pyramid: INTER_LINEAR_EXACT holds each axis weight as a multiple of 1/256, so it is off by da, db <= 1/512.  A bilinear
  form moves by da * df/da + db * df/db, both partial derivatives being convex combinations of tap differences, so by at
  most (da + db) * spread = spread / 256 (spread = max - min of the four taps).  Its integer arithmetic is exact up to the
  final rounding (<= 0.5).  Bound per pixel: |impl - model| <= 0.5 + spread / 256 (+ 1e-9 for the float64 model); level
  0 is the image itself.  Reported: the largest |impl - model| - 0.5.
- Harris: resp = ((float)a (float)b - (float)c (float)c - 0.04f ((float)a + (float)b)^2) * scale^4 in f32, relative to
  magnitude = (a b + c^2 + 0.04 (a + b)^2) scale^4.  Roundings, in units of u times the term they act on: the product
  a b carries 2 conversions + 1 product = 3, c c the same 3, 0.04 s s carries s twice (2 conversions, which are
  relative to a, b >= 0, + 1 sum = 2 each) + 2 products = 6; the first subtraction 1 (on a b + c^2), the second 1, the
  final product 1, and scale^4 = an f32 quotient raised by three f32 products = 4 + 3 = 7.  The worst term collects
  6 + 1 + 1 + 7 = 15; HARRIS_C = 16 leaves one for second-order terms.  No relative tolerance on the response itself (it
  cancels).  k = 0.04f is the same constant in model and implementation.
- Angle: |m01|, |m10| <= 255 * 15 * 749 < 2^24, so (float)m is exact and only fastAtan2 differs from atan2:
  ATAN_ERR_DEG (sift_stage_checks.py: measured 0.00955 against atan2, allowed 0.01) + the two f32 subtractions from 180
  and 360 (half an ulp of a value <= 360 each: 2 * 2^-16).  Compared on the circle.
- x, y: lx * scale is one f32 product of two f32 values: within one ulp of the float64 product (half an ulp in fact).
  cvRound(x / scale) must return lx (the descriptor centre): |x / scale - lx| <= 2 u lx << 0.5, so no tolerance.
- Blur: every pixel within 1 of the rounded float64 model; the share of pixels that are not exact is capped (below).
- Descriptor: the rotated coordinate x cos - y sin in f32, |x|, |y| <= 15: the angle in radians (<= 6.3, one rounded
  constant and one product: 2 u * 6.3 = 7.5e-7 rad) moves a point of radius <= 21.3 by 1.6e-5 px; the f32 rounding of
  cos and sin adds 2 * u * 15 = 1.8e-6, the two products and the sum 3 u * 30 = 5.4e-6: 2.3e-5 px in all.
  DESC_MARGIN = 1e-4 is 4.3 times that.  A bit with a coordinate that close to a half-integer is a close call; every
  other bit is equal (the two sampled values are u8 of the implementation's own blurred level: no tolerance).
- Selection: with eps_i = HARRIS_C u magnitude_i, the implementation's f32 threshold (the q-th best f32 response) lies
  between the q-th best of resp - eps and the q-th best of resp + eps.  A corner is surely kept when resp - eps >= the
  upper end, surely dropped when resp + eps < the lower end, a close call otherwise.  Ties are not close calls: corners
  with equal (min(a, b), max(a, b), |c|) have the same f32 response (cv2's expression is symmetric in IEEE arithmetic), so
  when all undecided corners form one such group and fewer than q corners are surely kept, the group holds the
  threshold and is kept whole.  The first retainBest (FAST scores) is exact integers.  Apart from close calls the
  implementation's set per level equals the model's.  Only with clear capacity flags.

Caps on what a check may set aside, per image (conditions, not measurements): MAX_SET_ASIDE = 1 % of descriptor bits,
of blur pixels not exact, and of keypoints as selection close calls.

Largest figures over all inputs of tests/test_orb_reference_cpu.py (the CPU oracle) and of the MI355X run of
tests/test_gpu_orb_reference.py (the kernels); the two runs gave the same figure in every row, as they should, the
kernels being equal to the oracle bit for bit:
  stage        bound                          measured, oracle = MI355X        set aside, oracle = MI355X
  layout       exact                          exact                            -
  pyramid      0.5 + spread / 256             0.62 beyond the model (noise);   -
                                              at most 76 % of spread / 256 used
  Harris       16 u magnitude                 4.15 u magnitude (saturated      -
                                              blocks, sums above 2^24)
  angle        0.01003 degrees                0.00954 degrees (noise)          -
  x, y         1 ulp; cvRound exact           0.5 ulp; exact                   -
  blur         1                              1                                1.1e-5 of the pixels not exact
  descriptor   equal outside the margin       equal; also equal inside it      0.10 % of the bits (noise)
  selection    equal sets                     equal sets                       0 keypoints
"""
import numpy as np

import orb_reference as ref
from sift_stage_checks import ATAN_ERR_DEG

U = 2.0 ** -24
HARRIS_C = 16
ANGLE_TOL = ATAN_ERR_DEG + 2 * 2.0 ** -16
DESC_MARGIN = 1e-4
MAX_SET_ASIDE = 0.01
OVF_ORB_CANDIDATES, OVF_ORB_KEYPOINTS = 1, 2


def make_run(img, nfeatures, pyr, nms, blur, kps, desc, flags, layout=None):
    """pyr / nms / blur: the implementation's packed pyramids (levels back to back); layout: the implementation's own
    (scale, w, h, quota) where it can report one (the oracle), else None: the packed size must then fit the model's."""
    H, W = img.shape
    scale, w, h, quota = ref.layout(W, H, nfeatures)
    assert pyr.size == int((w * h).sum()), ("packed pyramid size", pyr.size, int((w * h).sum()))
    return {"img": img, "nfeatures": nfeatures, "scale": scale, "w": w, "h": h, "quota": quota, "layout": layout,
            "pyr": ref.split_levels(pyr, w, h), "nms": ref.split_levels(nms, w, h), "blur": ref.split_levels(blur, w, h),
            "kps": kps, "desc": desc, "flags": int(flags)}


def _sampled(n, sample, rng):
    if sample is None or n <= sample:
        return np.arange(n)
    return np.sort((rng or np.random.default_rng(0)).choice(n, sample, replace=False))


def _by_level(kps, idx):
    for l in range(ref.NLEVELS):
        i = idx[kps["octave"][idx] == l]
        if len(i):
            yield l, i


def check_layout(run):
    scale, w, h, quota = ref.layout(run["img"].shape[1], run["img"].shape[0], run["nfeatures"])
    if run["layout"] is not None:
        s_i, w_i, h_i, q_i = run["layout"]
        assert np.array_equal(np.asarray(w_i), w) and np.array_equal(np.asarray(h_i), h), ("sizes", list(w_i), list(h_i), w, h)
        assert np.array_equal(np.asarray(q_i), quota), ("quotas", list(q_i), quota)
        assert np.array_equal(np.asarray(s_i, np.float32).view(np.uint32), scale.view(np.uint32)), "scales"
    assert quota.sum() >= run["nfeatures"] - 1 and np.all(quota >= 0)
    return {"levels": ref.NLEVELS, "quota_sum": int(quota.sum())}


def check_pyramid(run):
    pyr = run["pyr"]
    assert np.array_equal(pyr[0], run["img"]), "level 0 is not the image"
    worst, at, used = -0.5, None, 0.0
    for l in range(1, ref.NLEVELS):
        val, spread = ref.resize_linear(pyr[l - 1], int(run["w"][l]), int(run["h"][l]))
        d = np.abs(pyr[l].astype(np.float64) - val)
        bad = d > 0.5 + spread / 256 + 1e-9
        assert not bad.any(), ("pyramid level", l, int(bad.sum()), float((d - spread / 256).max()))
        ex = float((d - 0.5).max())
        if ex > worst:
            worst, at = ex, l
        used = max(used, float(((d - 0.5) / np.maximum(spread / 256, 1e-300))[spread > 0].max(initial=0.0)))
    return {"excess": worst, "level": at, "allowance_used": used}


def check_blur(run):
    worst, nonexact, total = 0, 0, 0
    for l in range(ref.NLEVELS):
        if not np.any(run["kps"]["octave"] == l):
            continue                                              # blurred only where a descriptor needs it
        m = np.rint(ref.blur(run["pyr"][l]))
        d = np.abs(run["blur"][l].astype(np.int64) - m.astype(np.int64))
        assert d.max() <= 1, ("blur level", l, int(d.max()), int((d > 1).sum()))
        worst = max(worst, int(d.max())); nonexact += int(np.count_nonzero(d)); total += d.size
    share = nonexact / max(total, 1)
    assert share < MAX_SET_ASIDE, ("blur pixels not exact", share)
    return {"blur": worst, "nonexact": share}


def check_keypoint_fields(run, sample=None, rng=None):
    """response, angle, x, y of (sampled) keypoints, each from the implementation's own level image and (lx, ly)"""
    kps = run["kps"]
    idx = _sampled(len(kps), sample, rng)
    out = {"response": 0.0, "angle": 0.0, "xy_ulp": 0.0, "inexact_sums": 0, "compared": len(idx)}
    for l, i in _by_level(kps, idx):
        w, h = int(run["w"][l]), int(run["h"][l])
        x, y = kps["lx"][i].astype(np.int64), kps["ly"][i].astype(np.int64)
        assert np.all((x >= ref.EDGE) & (x < w - ref.EDGE) & (y >= ref.EDGE) & (y < h - ref.EDGE)), ("band", l)
        resp, mag, a, b, c = ref.harris_at(run["pyr"][l], x, y)
        e = np.abs(kps["response"][i].astype(np.float64) - resp)
        k = int(np.argmax(e - HARRIS_C * U * mag))
        assert e[k] <= HARRIS_C * U * mag[k], ("response", l, int(x[k]), int(y[k]), float(kps["response"][i][k]), resp[k], e[k] / (U * mag[k]))
        out["response"] = max(out["response"], float((e / np.maximum(U * mag, 1e-300)).max()))
        out["inexact_sums"] += int(np.sum(np.maximum(a, b) > 2 ** 24))
        m01, m10 = ref.moments(run["pyr"][l], x, y)
        assert max(np.abs(m01).max(), np.abs(m10).max()) < 2 ** 24
        d = np.abs((kps["angle"][i].astype(np.float64) - ref.angle_deg(m01, m10) + 180.0) % 360.0 - 180.0)
        k = int(np.argmax(d))
        assert d[k] <= ANGLE_TOL, ("angle", l, int(x[k]), int(y[k]), float(kps["angle"][i][k]), int(m01[k]), int(m10[k]), d[k])
        assert np.all((kps["angle"][i] >= 0) & (kps["angle"][i] <= 360))
        out["angle"] = max(out["angle"], float(d[k]))
        s = np.float64(run["scale"][l])
        for f, v in (("x", x), ("y", y)):
            got = kps[f][i].astype(np.float64)
            ulp = np.spacing(np.abs(kps[f][i]).astype(np.float32)).astype(np.float64)
            r = np.abs(got - v * s) / ulp
            assert r.max() <= 1.0, (f, l, float(r.max()))
            assert np.array_equal(np.rint(got / s).astype(np.int64), v), (f, "cvRound(x / scale) != lx", l)
            out["xy_ulp"] = max(out["xy_ulp"], float(r.max()))
    return out


def check_descriptors(run, sample=None, rng=None):
    kps = run["kps"]
    idx = _sampled(len(kps), sample, rng)
    n_close, n_bits, n_close_diff = 0, 0, 0
    for l, i in _by_level(kps, idx):
        bits, margin = ref.descriptor_bits(run["blur"][l], kps["lx"][i], kps["ly"][i], kps["angle"][i])
        got = ref.unpack_bits(run["desc"][i])
        close = margin < DESC_MARGIN
        diff = (bits != got)
        bad = diff & ~close
        assert not bad.any(), ("descriptor bits", l, int(bad.sum()), [(int(i[k]), int(b)) for k, b in zip(*np.nonzero(bad))][:8])
        n_close += int(close.sum()); n_bits += close.size; n_close_diff += int((diff & close).sum())
    share = n_close / max(n_bits, 1)
    assert share < MAX_SET_ASIDE, ("descriptor close calls", share)
    return {"close": share, "close_differing": n_close_diff, "compared": len(idx)}


def model_selection(run, l, quota=None):
    """(surely kept, close calls, stage-1 survivors) of level l as sets of (x, y), from the run's NMS map and level"""
    q = int((run["quota"] if quota is None else quota)[l])
    sel = ref.select(run["pyr"][l], run["nms"][l], q)
    n = len(sel["x"])
    pts = list(zip(sel["x"].tolist(), sel["y"].tolist()))
    if q <= 0 or n == 0:
        return set(), set(), sel
    if n <= q:
        return set(pts), set(), sel
    eps = HARRIS_C * U * sel["mag"]
    hi = ref.kth_best(sel["resp"] + eps, q)
    lo = ref.kth_best(sel["resp"] - eps, q)
    sure = sel["resp"] - eps >= hi
    unsure = ~sure & ~(sel["resp"] + eps < lo)
    if unsure.any() and sure.sum() < q:
        key = np.stack([np.minimum(sel["a"], sel["b"]), np.maximum(sel["a"], sel["b"]), np.abs(sel["c"])], 1)[unsure]
        if np.all(key == key[0]):                                  # one tie group holds the threshold: kept whole
            sure = sure | unsure
            unsure = np.zeros(n, bool)
    return {p for p, s in zip(pts, sure) if s}, {p for p, s in zip(pts, unsure) if s}, sel


def check_selection(run, quota=None):
    assert run["flags"] == 0, "selection is only comparable when no workspace cap was hit"
    kps = run["kps"]
    assert np.all(np.diff(kps["octave"]) >= 0), "keypoints are not level-major"
    n_close, n_model = 0, 0
    for l in range(ref.NLEVELS):
        k = kps[kps["octave"] == l]
        impl = set(zip(k["lx"].tolist(), k["ly"].tolist()))
        assert len(impl) == len(k), ("a keypoint twice", l)
        sure, close, _ = model_selection(run, l, quota)
        assert sure <= impl, ("model keypoints the implementation lacks", l, sorted(sure - impl)[:8], len(sure - impl))
        assert impl <= sure | close, ("implementation keypoints the model rejects", l, sorted(impl - sure - close)[:8])
        n_close += len(close); n_model += len(sure) + len(close)
    share = n_close / max(len(kps), 1)
    assert share < MAX_SET_ASIDE, ("selection close calls", share)
    return {"close": share, "keypoints": len(kps), "model": n_model}


def check_all(run, sample=None, expect_overflow=False):
    """every stage; the selection only with clear flags (expect_overflow: assert that they are set instead)"""
    st = {"layout": check_layout(run), "pyramid": check_pyramid(run), "blur": check_blur(run),
          "fields": check_keypoint_fields(run, sample), "descriptor": check_descriptors(run, sample)}
    if expect_overflow:
        assert run["flags"] & (OVF_ORB_CANDIDATES | OVF_ORB_KEYPOINTS), run["flags"]
    else:
        assert run["flags"] == 0, run["flags"]
        st["selection"] = check_selection(run)
    return st


# ------------------------------------------------------------------------------------------ inputs
SCENES = [(640, 480, 1000), (640, 480, 4000), (848, 478, 4000), (1920, 1080, 2000), (130, 98, 300), (333, 257, 500),
          (1001, 203, 1500), (96, 96, 100)]
HD_SAMPLE = 1500


def scene_overflows(W, H):
    """a textured 1920x1080 frame holds more than the 8192 raster corners a level's workspace takes: the capacity flag
    is set and the keypoint set is the workspace's, not cv2's"""
    return W * H > 10 ** 6


def scene(W, H):
    from relative_pose_estimation_amd import synthetic, geometry
    return synthetic.make_batch(1, geometry.default_camera_matrix(W, H), W, H, cfg=5)[0][0]


def _peak(im, x, y):
    im[y - 1:y + 2, x - 1:x + 2] = 170
    im[y, x] = 255


BAND_LEVEL = 4


def band_edge(W=480, H=360):
    """peaks centred exactly on the first / last pixel of the 31-px band and one pixel outside it at level 0, and
    Gaussian blobs stepped by a quarter of a level pixel across x = 31 of level BAND_LEVEL"""
    im = np.full((H, W), 30.0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    s = float(ref.layout(W, H, 500)[0][BAND_LEVEL])
    for k in range(13):
        cx, cy = (31.0 + 0.25 * (k - 6)) * s + 0.5 * (s - 1), 50.0 + 18 * k
        im += 200 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * (1.3 * s) ** 2))
    im = np.clip(np.rint(im), 0, 255).astype(np.uint8)
    for px, py in band_edge_peaks(W, H):
        _peak(im, px, py)
    return im


def band_edge_peaks(W=480, H=360):
    """level-0 peak centres: even entries on the band edge (kept), odd ones one pixel outside (dropped)"""
    return [(31, 300), (30, 322), (W - 32, 40), (W - 31, 70), (150, 31), (200, 30), (250, H - 32), (300, H - 31)]


def tie_board(W=430, H=96, cell=9, row=32):
    """a two-tone board of 9-px cells; the cells of one row carry one pixel of the other tone at their centre (y = 32).
    (A plain checkerboard has no FAST-9 corner: around an X junction the ring alternates in runs of at most 7 equal / 4
    different pixels.)  Every centre pixel is a corner with the same FAST score, the same Harris sums and, the board
    being symmetric about it, m01 = m10 = 0.  Row 32 lies inside the border band of level 0 only (96 rows are the
    smallest legal image), so the ties stay exact: a resized board ties responses almost but not exactly (1e-9 relative,
    below f32), which would be close calls by the dozen and fit no cap."""
    yy, xx = np.mgrid[0:H, 0:W]
    yy = yy + (cell // 2 - row) % cell
    tone = ((xx // cell + yy // cell) % 2).astype(bool)
    centre = (xx % cell == cell // 2) & (np.mgrid[0:H, 0:W][0] == row)
    return np.where(tone ^ centre, 215, 40).astype(np.uint8)


WEDGE_OFFSETS = (-4.0, -1.5, 1.5, 4.0)


def wedges(W=480, H=360):
    """bright 44-degree wedges on a dark ground whose axes point 1.5 and 4 degrees either side of 0 / 90 / 180 / 270:
    the tip is a FAST corner and the intensity centroid of its patch lies along the axis"""
    im = np.full((H, W), 40, np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    n = 0
    for quad in range(4):
        for off in WEDGE_OFFSETS:
            cx, cy = 70 + 85 * (n % 4) + 20 * (quad % 2), 50 + 80 * quad
            th = 90.0 * quad + off
            dx, dy = x - cx, y - cy
            d = (np.degrees(np.arctan2(dy, dx)) - th + 180.0) % 360.0 - 180.0
            im[(np.abs(d) <= 22.0) & (dx * dx + dy * dy <= 30.0 ** 2)] = 230
            n += 1
    return im


def saturated_blocks(W=320, H=240, seed=21):
    """white rectangles on black: Sobel responses of +-1020, block sums above 2^24 (so (float)a is inexact)"""
    rng = np.random.default_rng(seed)
    im = np.zeros((H, W), np.uint8)
    for _ in range(40):
        w, h = rng.integers(8, 50, 2)
        x0 = rng.integers(0, W - w); y0 = rng.integers(0, H - h)
        im[y0:y0 + h, x0:x0 + w] = 255 - im[y0:y0 + h, x0:x0 + w]
    return im


def drawn_images():
    """name -> (u8 image, nfeatures, capacity flags expected)"""
    import fast_sides
    return {
        "band_edge": (band_edge(), 500, False),
        "tie_board": (tie_board(), 100, False),
        "wedges": (wedges(), 500, False),
        "saturated_blocks": (saturated_blocks(), 500, False),
        "dense_noise": (fast_sides.dense_noise(), 1000, True),
        "flat": (np.full((240, 320), 117, np.uint8), 500, False),
        "blobs_two_sides": (fast_sides.blobs_two_sides(), 1000, False),
        "soft_noise": (fast_sides.soft_noise(), 1000, True),
    }


def check_drawn_purpose(name, run, st):
    """what each drawn image is there for"""
    k = run["kps"]
    if name == "flat":
        assert len(k) == 0
    if name in ("dense_noise", "soft_noise"):
        assert run["flags"] & OVF_ORB_CANDIDATES and len(k) >= run["nfeatures"] // 3
    if name == "saturated_blocks":
        assert st["fields"]["inexact_sums"] >= 10                 # keypoints whose sums exceed 2^24
    if name == "band_edge":
        k0 = set(zip(k["lx"][k["octave"] == 0].tolist(), k["ly"][k["octave"] == 0].tolist()))
        for n, p in enumerate(band_edge_peaks()):
            assert (p in k0) == (n % 2 == 0), (p, "kept" if p in k0 else "dropped")
        l = BAND_LEVEL
        free = nms_without_band(run["pyr"][l])
        kl = k[k["octave"] == l]
        assert np.any(free[:, 30] > 0) and np.any(free[:, 31] > 0), "no corner beside / on the band edge at the coarse level"
        assert np.any(kl["lx"] == 31) and not np.any(run["nms"][l][:, :31]) and kl["lx"].min() == 31
        ys = np.nonzero(free[:, 31])[0]
        assert set(zip([31] * len(ys), ys.tolist())) <= set(zip(kl["lx"].tolist(), kl["ly"].tolist()))
    if name == "tie_board":
        k0 = k[k["octave"] == 0]
        q0 = int(run["quota"][0])
        assert len(k0) > 2 * q0, (len(k0), q0)                      # both thresholds fell on ties: everything kept
        assert len(np.unique(k0["response"])) == 1 and np.all(k0["angle"] == 0)
        m01, m10 = ref.moments(run["pyr"][0], k0["lx"], k0["ly"])
        assert not m01.any() and not m10.any()
    if name == "wedges":
        a = k["angle"][k["octave"] <= 2].astype(np.float64)
        for quad in range(4):
            d = (a - 90.0 * quad + 180.0) % 360.0 - 180.0
            assert np.any((d > 0) & (d < 8)) and np.any((d < 0) & (d > -8)), (quad, np.sort(d[np.abs(d) < 20]))


def nms_without_band(level):
    """FAST score -> strict 3x3 maximum, without the border filter (tests/fast_sides.py's score model)"""
    import fast_sides
    s = fast_sides.one_sided_score_map(level, ref.FAST_THRESHOLD).astype(np.int64)
    p = np.pad(s, 1)
    h, w = s.shape
    nb = [p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    return np.where((s > 0) & (s > np.max(nb, axis=0)), s, 0)
