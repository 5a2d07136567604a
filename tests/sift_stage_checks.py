"""Stage-by-stage comparison of a SIFT implementation (the CPU oracle or the HIP kernels) with the float64 model in
tests/sift_reference.py.  Each check feeds the model the implementation's own upstream output, so errors do not
compound, and returns the statistics it measured (largest error, excluded fraction) for the test to report.

Tolerances and margins, with their derivations (u = 2^-24, the f32 unit roundoff; grey values <= 255):

- PYR_TOL(ks): one separable pass of ks f32 taps is a chain of ks fused multiply-adds, each rounding by <= u * 255, plus
  the f32 rounding of the normalised coefficients (sum |dk| <= u, times 255).  Row pass <= (ks + 1) u 255; the column
  pass adds r + 1 = ks/2 + 1 roundings, u 255 for its pre-added tap pairs and u 255 for its coefficients, and carries
  the row error with weight sum(k) = 1.  Level 0 also carries the f32 INTER_LINEAR upsample (<= 4 u 255).  Measured
  on the oracle: 4.6e-5 (level 0), 6.5e-5 (others), against bounds of 3.7e-4 .. 6.7e-4.
- OFF_MARGIN: the implementation solves the 3x3 Newton system in f32 from the same f32 DoG; its offsets differ from the
  float64 solution by about cond(H) * u.  Measured on the oracle (320x240): largest xi difference 6.7e-7 (xc, xr are
  only visible through the f32 pt, see PT_TOL).  A decision (|offset| < 0.5, cvRound of a step) is set aside when the
  float64 offset lies within 1e-4 of a half-integer: over a hundred times the measured difference.
- CONTR_MARGIN / EDGE_MARGIN: relative distance of |contr| * 3 to 0.04 and of tr^2 * 10 to 11^2 * det; f32 evaluation
  of the contrast (a DoG value plus a 3-term dot product) and of the 2x2 Hessian terms is good to ~10 u relative away
  from cancellation, so 1e-4 is a hundred-fold margin.
- ATAN_ERR_DEG: cv::fastAtan2's degree-7 polynomial, measured against atan2 on 200k directions at four radii: largest
  error 0.00955 degrees.  An orientation sample within that distance of a bin edge may be binned either way; the model
  computes its histogram both ways and allows the spread of the resulting angles.
- ANGLE_TOL: on top of that spread, f32 accumulation of <= (2*14+1)^2 weighted magnitudes (relative ~ n u <= 5e-5) moves
  a parabolic peak by < 1e-3 bins = 0.01 degrees; 0.02 degrees is allowed.
- PEAK_MARGIN: the f32 histogram sums <= 29^2 = 841 samples per bin; rounding errors of a sum of n positive terms grow
  like sqrt(n) u in practice (n u = 5e-5 at worst), so 2e-5 relative to the maximum is ~10 sqrt(n) u.  A bin that close to
  a neighbour or to 0.8 max is a decision the f32 histogram may take either way; the location is set aside.
- Descriptors: every element within 1 of the float64 model; under 1 % not exact.  The descriptor is continuous in its
  inputs (trilinear weights vanish at every bin and window edge) apart from the final rounding to u8, so f32 sums and
  the fastAtan2 / exp conventions only flip elements that sit at .5.

Largest errors measured on the MI355X run of tests/test_gpu_sift_reference.py (the kernels equal the oracle bit for bit,
so the CPU rows measure the same): pyramid 7.3e-5 (HD frame); pt 1.2e-4 octave pixels (HD,
the f32 rounding of c + xc), size 1.5e-7 and response 1.6e-7 relative, xi byte 0; angle 3.9e-5 degrees beyond the flip
allowance; descriptor elements 1, at most 0.06 % not exact.  Set aside as close calls: at most 0.9 % of keypoint
locations and 0.7 % of orientation locations.
"""
import numpy as np

import sift_reference as ref

U = 2.0 ** -24
OFF_MARGIN = 1e-4
CONTR_MARGIN = 1e-4
EDGE_MARGIN = 1e-4
ATAN_ERR_DEG = 0.01
ANGLE_TOL = 0.02
PEAK_MARGIN = 2e-5
RADIUS_MARGIN = 1e-4
PT_TOL = 1e-3          # octave pixels: f32 rounding of c + xc (c < 4096: <= 2^-12) plus the offset difference
SIZE_RTOL = 1e-5       # size = 1.6 * 2^((l + xi)/3) ...: d size / size = ln2/3 * d xi
RESP_RTOL = 1e-4
MAX_EXCLUDED = 0.01


def pyr_tol(ks, level0=False):
    return 255 * U * (ks + ks // 2 + 4 + (4 if level0 else 0))


def check_pyramid(img, pyr):
    """pyr: the implementation's pyramid as a list of (6, h, w) f32 arrays.  Level 0 of octave 0 from the u8 image,
    level i from the implementation's level i - 1, the base of octave o from its level 3 of octave o - 1 (exact)."""
    H, W = img.shape
    assert [g.shape[1:][::-1] for g in pyr] == ref.octave_sizes(W, H)
    worst = {}
    for o, g in enumerate(pyr):
        if o == 0:
            m = ref.octave0_level0(img)
            err = np.abs(m - g[0]).max()
            worst[(0, 0)] = err
            assert err <= pyr_tol(ref.kernel_size(ref.initial_sigma()), True), ("level 0", err)
        else:
            assert np.array_equal(ref.octave_base(pyr[o - 1][ref.NOL]), g[0]), ("octave base", o)
        for i in range(1, ref.NOL + 3):
            m = ref.next_level(g[i - 1].astype(np.float64), i)
            err = np.abs(m - g[i]).max()
            worst[(o, i)] = err
            assert err <= pyr_tol(ref.kernel_size(ref.level_sigmas()[i])), ("level", o, i, err)
    return max(worst.values())


def model_extrema(pyr):
    """the model's refined extrema from the implementation's pyramid, per octave"""
    out = []
    for o, g in enumerate(pyr):
        D = ref.dog(g)                                  # f32 - f32: the implementation's DoG bit for bit
        seeds = ref.find_seeds(D)
        out.append(ref.adjust_local_extrema(D.astype(np.float64), seeds) if seeds.shape[1] else None)
    return out


def check_keypoints(pyr, kps, sample=None, rng=None):
    """refined keypoints: one-to-one on (octave, layer, r, c) modulo close calls; pt, size, response, packed octave.
    kps: the implementation's uncapped keypoints as reported (firstOctave rescale applied).
    sample: compare fields on at most this many matched locations of octave 0 (NumPy time on HD frames)."""
    o_i, l_i, r_i, c_i, xib_i = ref.locate(kps)
    impl = {}
    for k in range(len(kps)):
        impl.setdefault((int(o_i[k]), int(l_i[k]), int(r_i[k]), int(c_i[k])), k)
    ext = model_extrema(pyr)
    model, close, n_lost = {}, set(), 0
    for o, e in enumerate(ext):
        if e is None:
            continue
        near = (e["off_margin"] < OFF_MARGIN) | (e["contr_margin"] < CONTR_MARGIN) | (e["edge_margin"] < EDGE_MARGIN)
        f = ref.keypoint_fields(o, e)
        for k in range(len(e["l"])):
            key = (o, int(e["l"][k]), int(e["r"][k]), int(e["c"][k]))
            if key in model and not near[k]:
                continue                                 # same location from another seed: removeDuplicatedSorted
            model[key] = (k, o, f, e, bool(near[k]))
            if near[k]:
                close.add(key)
        # seeds the model drops by a close call, which the implementation may keep (at a location the model cannot name)
        n_lost += int(np.sum(e["dropped_margin"] < max(CONTR_MARGIN, EDGE_MARGIN, OFF_MARGIN))) + \
            int(np.sum(e["lost_margin"] < OFF_MARGIN))
    only_model = [k for k in model if k not in impl and k not in close]
    only_impl = [k for k in impl if k not in model]
    assert not only_model, ("model keypoints the implementation lacks", only_model[:10], len(only_model))
    assert len(only_impl) <= n_lost, ("implementation keypoints the model does not find", only_impl[:10], len(only_impl), n_lost)
    excluded = (len(close) + n_lost) / max(len(model), 1)
    assert excluded < MAX_EXCLUDED, excluded
    keys = [k for k in model if k in impl and k not in close]
    if sample is not None:
        rng = rng or np.random.default_rng(0)
        big = [k for k in keys if k[0] == 0]
        small = [k for k in keys if k[0] != 0]
        if len(big) > sample:
            big = [big[i] for i in rng.choice(len(big), sample, replace=False)]
        keys = big + small
    worst = {"pt": 0.0, "size": 0.0, "response": 0.0, "xi_byte": 0}
    for key in keys:
        k, o, f, e, _ = model[key]
        i = impl[key]
        s = 2.0 ** (o - 1)                                # reported = upsampled-octave value * 0.5
        dpt = max(abs(kps["x"][i] / s - (e["c"][k] + e["xc"][k])), abs(kps["y"][i] / s - (e["r"][k] + e["xr"][k])))
        dsz = abs(kps["size"][i] * 2 - f["size"][k]) / f["size"][k]
        drs = abs(kps["response"][i] - f["response"][k]) / f["response"][k]
        xib_m = (int(f["octave"][k]) >> 16) & 255
        dxb = abs(int(xib_i[i]) - xib_m)
        assert dpt <= PT_TOL and dsz <= SIZE_RTOL and drs <= RESP_RTOL and dxb <= 1, (key, dpt, dsz, drs, dxb)
        worst["pt"] = max(worst["pt"], dpt); worst["size"] = max(worst["size"], dsz)
        worst["response"] = max(worst["response"], drs); worst["xi_byte"] = max(worst["xi_byte"], dxb)
    worst.update(n_model=len(model), n_impl=len(impl), excluded=excluded, compared=len(keys))
    return worst


def check_orientations(pyr, kps, sample=None, rng=None):
    """the multiset of angles at every location of the implementation's keypoints, from its level image and size"""
    o_i, l_i, r_i, c_i, _ = ref.locate(kps)
    groups = {}
    for k in range(len(kps)):
        groups.setdefault((int(o_i[k]), int(l_i[k]), int(r_i[k]), int(c_i[k])), []).append(k)
    keys = list(groups)
    if sample is not None and len(keys) > sample:
        rng = rng or np.random.default_rng(1)
        keys = [keys[i] for i in rng.choice(len(keys), sample, replace=False)]
    n_excl, worst, n_ang = 0, 0.0, 0
    for key in keys:
        o, l, r, c = key
        ks = groups[key]
        s = float(kps["size"][ks[0]]) * 2 * 0.5 / 2.0 ** o       # scl_octv of the upsampled-octave keypoint
        if ref._half_distance(ref.ORI_RADIUS * s) < RADIUS_MARGIN:
            n_excl += 1
            continue
        ang, tol, margin = ref.orientations(pyr[o][l], c, r, s, ATAN_ERR_DEG)
        if tol is None or margin < PEAK_MARGIN:
            n_excl += 1
            continue
        got = np.sort(kps["angle"][ks].astype(np.float64))
        assert len(got) == len(ang), (key, got, ang)
        used = np.zeros(len(got), bool)
        for a, t in zip(ang, tol):
            d = np.abs((got - a + 180) % 360 - 180)
            d[used] = np.inf
            j = int(np.argmin(d))
            assert d[j] <= t + ANGLE_TOL, (key, a, got, d[j], t)
            used[j] = True
            worst = max(worst, d[j] - t)
            n_ang += 1
    excluded = n_excl / max(len(keys), 1)
    assert excluded < MAX_EXCLUDED, excluded
    return {"angle": worst, "excluded": excluded, "angles": n_ang}


def check_descriptors(pyr, kps, desc, sample=None, rng=None):
    """every descriptor from the implementation's level image and keypoint (x, y, size, angle, octave)"""
    idx = np.arange(len(kps))
    if sample is not None and len(idx) > sample:
        rng = rng or np.random.default_rng(2)
        idx = np.sort(rng.choice(len(idx), sample, replace=False))
    o_r, l, _ = ref.unpack_octave(kps["octave"])
    worst, nonexact, total = 0.0, 0, 0
    for k in idx:
        o = int(o_r[k])
        sc = np.float32(2.0 ** -o)
        ori = np.float32(360) - kps["angle"][k]
        if abs(float(ori) - 360.0) < ref.FLT_EPSILON:
            ori = np.float32(0)
        m = ref.descriptor(pyr[o + 1][int(l[k])], float(kps["x"][k] * sc), float(kps["y"][k] * sc), float(ori),
                           float(kps["size"][k] * sc * np.float32(0.5)))
        d = np.abs(m - desc[k].astype(np.float64))
        assert d.max() <= 1, (int(k), d.max(), np.nonzero(d > 1)[0][:8])
        worst = max(worst, d.max())
        nonexact += int(np.count_nonzero(d))
        total += d.size
    frac = nonexact / max(total, 1)
    assert frac < MAX_EXCLUDED, frac
    return {"desc": worst, "nonexact": frac, "compared": len(idx)}


def same_records(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8).reshape(len(a), -1), b.view(np.uint8).reshape(len(b), -1))


def record_set(a):
    return sorted(map(bytes, a.view(np.uint8).reshape(len(a), -1)))


def check_post(uncapped, capped, nfeatures):
    """removeDuplicatedSorted + retainBest + rescale applied by the model to the implementation's uncapped keypoints:
    without a cap, the same list in the same (KeyPoint_LessThan) order; with one, the same set -- the implementation's
    order is sorted, the model's is nth_element's (returned for order tests)."""
    pre = ref.unscale_first_octave(uncapped)
    m = ref.post_process(pre, nfeatures)
    if nfeatures <= 0 or len(uncapped) <= nfeatures:
        assert same_records(m, uncapped.astype(ref.KP_DTYPE)) and same_records(capped.astype(ref.KP_DTYPE), m)
        return m
    c = capped.astype(ref.KP_DTYPE)
    assert record_set(m) == record_set(c), (len(m), len(c))
    assert np.array_equal(ref.lessthan_order(c), np.arange(len(c))), "the implementation's capped list is not sorted"
    return m


# ------------------------------------------------------------------------------------------ drawn inputs
def _blob(W, H, cx, cy, sigma, amp):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))


def drawn_images(W=160, H=120):
    """inputs placed where SIFT kernels go wrong: name -> u8 image"""
    out = {}
    base = np.full((H, W), 110.0)
    # Gaussian blobs against the 5-px border of the upsampled octave and in the corners (clipped windows)
    im = base.copy()
    for cx, cy in ((3, 3), (W - 4, 3), (3, H - 4), (W - 4, H - 4), (W // 2, 2), (1, H // 2), (W - 2, H // 2), (W // 2, H - 3)):
        im += _blob(W, H, cx, cy, 2.0, 90.0)
    for cx, cy in ((9, 9), (W - 10, H - 10), (12, H - 8)):
        im -= _blob(W, H, cx, cy, 2.5, 80.0)
    out["border_blobs"] = im
    # blobs whose gradient points along 0 / 360 degrees: bright towards +x (the histogram peaks at the wrap)
    im = base.copy()
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    for cx, cy, s in ((W * 0.3, H * 0.5, 4.0), (W * 0.7, H * 0.3, 3.0), (W * 0.65, H * 0.75, 5.0)):
        env = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * (2 * s) ** 2))
        im += 70 * env * np.tanh((x - cx) / s)
    out["wrap_blobs"] = im
    # L-corners: two dominant gradient directions at one location
    im = base.copy()
    for x0, y0, a in ((W // 4, H // 4, 120), (W // 2 + 10, H // 2, -90), (W // 5, H * 2 // 3, 100)):
        im[y0:y0 + 25, x0:x0 + 6] += a
        im[y0 + 19:y0 + 25, x0:x0 + 25] += a
    out["l_corners"] = im
    # one blob large enough to be found only in the deepest octaves
    out["large_blob"] = base + _blob(W, H, W * 0.5, H * 0.5, min(W, H) * 0.07, 100.0)
    # a flat image: no keypoint at all
    out["flat"] = base.copy()
    # a saturated block (dx = dy = 0 inside) on a textured background
    rng = np.random.default_rng(7)
    im = blur_noise(rng, W, H)
    im[H // 4:H * 3 // 4, W // 4:W * 3 // 4] = 255
    out["saturated_block"] = im
    return {k: np.clip(np.rint(v), 0, 255).astype(np.uint8) for k, v in out.items()}


def blur_noise(rng, W, H):
    n = rng.normal(0, 1, (H // 4 + 1, W // 4 + 1))
    n = np.kron(n, np.ones((4, 4)))[:H, :W]
    return 110 + 40 * ref.blur(n, 1.5)
