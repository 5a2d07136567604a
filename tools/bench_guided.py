#!/usr/bin/env python3
"""What rpe_guided_matches costs next to the crossCheck matcher it extends: windowed matching over
a synthetic stream as ONE pair list (256 VGA frames, window 4: 1014 pairs, ORB-1000 / 500).

  match_stage      RPE_STAGE_MATCH of rpe_estimate_pairs over the list (rpe_get_stage_ms: hipEvents on the handle's stream)
  guided           rpe_guided_matches on the run's own poses, no output fetched: records kernel + tile kernel (+ select)

The guided call is timed on the host around a call that ends in a stream synchronise (the C-ABI does not hand out the
handle's stream); at 1014 pairs the launches and the synchronise are microseconds against milliseconds.  Warm-up runs
first; median and min / max of the repetitions, both in the same process.  Prints one JSON line.

--l2: the same workload on an ORB + NORM_L2 handle (rpe_guided_matches_l2 against the L2 crossCheck matcher), then a second
JSON line for a SIFT-2048 handle over a short pair list (--sift-frames frames of the stream the tests' PHYSICS set is
rendered from, window 2), with the guided, crossCheck and RANSAC inlier counts of its pairs.

    python tools/bench_guided.py [--l2] [--frames 256] [--window 4] [--reps 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the six-frame VGA stream of the SIFT line: the parameters of the tests' PHYSICS set (tests/scale_model.py), so that the
# counts recorded in DESIGN.md section 5 are those of frames the suite also sees; the tool itself needs only the package
PHYSICS_STREAM = dict(n_frames=6, seed=5_000_041, max_angle_deg=2.0, step=0.3)


def _stats(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4), "n": len(v)}


def window_pairs(F, k):
    return np.array([(i, i + d) for d in range(1, k + 1) for i in range(F - d)], np.int32)


def measure(e, frames, pairs, K, a, l2):
    """the pair list over the frames on engine e: the match stage and the guided call of its norm, per repetition"""
    F, P = len(frames), len(pairs)
    e.frames_reserve(F)
    for s in range(0, F, 2 * P):
        e.frames_put(frames[s:s + 2 * P], np.arange(s, min(s + 2 * P, F), dtype=np.int32))
    e.set_profiling(True)

    def guided_untimed():
        if l2:
            return e.lib.rpe_guided_matches_l2(e.h, P, None, None, a.gate_px, float("inf"), None, None, None, None, None, None)
        return e.lib.rpe_guided_matches(e.h, P, None, None, a.gate_px, 256, None, None, None, None, None, None)

    tm, tg = [], []
    for r in range(a.warmup + a.reps):
        res = e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)
        ms = e.stage_ms()["match"]
        e.synchronize()
        t0 = time.perf_counter()
        rc = guided_untimed()
        t1 = time.perf_counter()
        assert rc == 0
        if r >= a.warmup:
            tm.append(ms); tg.append((t1 - t0) * 1e3)
    nm = (e.guided_matches_l2 if l2 else e.guided_matches)(P, gate_px=a.gate_px)[5]
    rmask = e.fetch_structure(P)[0]
    ok = res[4] == 0
    out = {"n_pairs": P, "pairs_ok": int(ok.sum())}
    out["guided_median"] = float(np.median(nm[ok])); out["ransac_inliers_median"] = float(np.median(rmask.sum(1)[ok]))
    out["matches_median"] = float(np.median(res[3][ok]))
    out["match_stage"] = _stats(tm)
    out["guided"] = _stats(tg)
    out["ratio"] = round(out["guided"]["median_ms"] / out["match_stage"]["median_ms"], 3)
    return out, nm, rmask.sum(1), res[3], ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--gate-px", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--l2", action="store_true", help="ORB + NORM_L2 instead of Hamming, plus the SIFT-2048 line")
    ap.add_argument("--sift-frames", type=int, default=8)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    F, k = a.frames, a.window
    pairs = window_pairs(F, k)
    P = len(pairs)
    out = {"norm": "l2" if a.l2 else "hamming", "frames": F, "window": k, "nfeatures": a.nfeatures, "max_matches": a.max_matches, "gate_px": a.gate_px}
    frames = synthetic.make_stream(F, K, W, H, workers=a.workers)[0]
    e = _capi.Engine(W, H, max_batch=P, nfeatures=a.nfeatures, max_matches=a.max_matches,
                     norm_type=_capi.NORM_L2 if a.l2 else _capi.NORM_HAMMING)
    out.update(measure(e, frames, pairs, K, a, a.l2)[0])
    e.close()
    print(json.dumps(out))
    if not a.l2:
        return
    frames = synthetic.make_stream(PHYSICS_STREAM["n_frames"], K, seed=PHYSICS_STREAM["seed"], max_angle_deg=PHYSICS_STREAM["max_angle_deg"],
                                   step=PHYSICS_STREAM["step"])[0][:a.sift_frames]
    pairs = window_pairs(len(frames), 2)
    out = {"norm": "l2", "feature": "SIFT", "frames": len(frames), "window": 2, "nfeatures": 2048, "max_matches": a.max_matches, "gate_px": a.gate_px}
    e = _capi.Engine(W, H, max_batch=len(pairs), nfeatures=2048, max_matches=a.max_matches,
                     feature_method=_capi.FEATURE_SIFT, norm_type=_capi.NORM_L2)
    res, nm, inl, cc, ok = measure(e, frames, pairs, K, a, True)
    e.close()
    out.update(res)
    out["per_pair"] = {"guided": nm.tolist(), "crosscheck": cc.tolist(), "ransac_inliers": inl.tolist(), "ok": ok.astype(int).tolist()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
