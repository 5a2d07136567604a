#!/usr/bin/env python3
"""What rpe_guided_matches costs next to the crossCheck matcher it extends: windowed matching over
a synthetic stream as ONE pair list (256 VGA frames, window 4: 1014 pairs, ORB-1000 / 500).

  match_stage      RPE_STAGE_MATCH of rpe_estimate_pairs over the list (rpe_get_stage_ms: hipEvents on the handle's stream)
  guided           rpe_guided_matches on the run's own poses, no output fetched: records kernel + tile kernel (+ select)

The guided call is timed on the host around a call that ends in a stream synchronise (the C-ABI does not hand out the
handle's stream); at 1014 pairs the launches and the synchronise are microseconds against milliseconds.  Warm-up runs
first; median and min / max of the repetitions, both in the same process.  Prints one JSON line.

    python tools/bench_guided.py [--frames 256] [--window 4] [--reps 9]
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


def _stats(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--gate-px", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    F, k = a.frames, a.window
    pairs = np.array([(i, i + d) for d in range(1, k + 1) for i in range(F - d)], np.int32)
    P = len(pairs)
    out = {"frames": F, "window": k, "n_pairs": P, "nfeatures": a.nfeatures, "max_matches": a.max_matches, "gate_px": a.gate_px}
    frames = synthetic.make_stream(F, K, W, H, workers=a.workers)[0]
    e = _capi.Engine(W, H, max_batch=P, nfeatures=a.nfeatures, max_matches=a.max_matches)
    e.frames_reserve(F)
    for s in range(0, F, 2 * P):
        e.frames_put(frames[s:s + 2 * P], np.arange(s, min(s + 2 * P, F), dtype=np.int32))
    e.set_profiling(True)

    def guided_untimed():
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
    nm = e.guided_matches(P, gate_px=a.gate_px)[5]
    rmask = e.fetch_structure(P)[0]
    ok = res[4] == 0
    out["pairs_ok"] = int(ok.sum())
    out["guided_median"] = float(np.median(nm[ok])); out["ransac_inliers_median"] = float(np.median(rmask.sum(1)[ok]))
    out["matches_median"] = float(np.median(res[3][ok]))
    out["match_stage"] = _stats(tm)
    out["guided"] = _stats(tg)
    out["ratio"] = round(out["guided"]["median_ms"] / out["match_stage"]["median_ms"], 3)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
