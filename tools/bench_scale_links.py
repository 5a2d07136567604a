#!/usr/bin/env python3
"""What rpe_scale_links costs and what it replaces: windowed matching over a synthetic stream as
ONE pair list (256 VGA frames, window 4: 1014 pairs), and the links between each pair (i, i + d) and the next pair
(i, i + d + 1) of the same first frame (759 links, side 0).

  pairs            rpe_estimate_pairs over the list (the frames are put once, outside the timed window)
  links_first      rpe_scale_links right after a pair list: structure kernels + link kernel + fetch of the results
  links_again      the same call again: the per-match buffers already hold the structure
  host_path        what a caller without the call does: rpe_fetch_structure + rpe_fetch_match_indices + rpe_fetch_results,
                   then the NumPy model of tests/scale_model.py (host_fetch / host_model give the two parts)

Every timed window ends in a stream synchronise; warm-up runs first; median and min / max of the repetitions.  The
kernel's own device time comes from `rocprofv3 --kernel-trace --stats -- python tools/bench_scale_links.py`
(scale_links_kernel), in a run of its own.  The GPU result is asserted equal to the model.  Prints one JSON line.

    python tools/bench_scale_links.py [--frames 256] [--window 4] [--reps 5]
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
    v = np.asarray(v) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4), "n": len(v)}


def window_pairs_and_links(F, k):
    """pairs (i, i + d), d-major, and the links (index of (i, i + d), index of (i, i + d + 1), side 0)"""
    pairs = np.array([(i, i + d) for d in range(1, k + 1) for i in range(F - d)], np.int32)
    first = np.concatenate([[0], np.cumsum([F - d for d in range(1, k + 1)])])
    links = np.array([(first[d - 1] + i, first[d] + i, 0) for d in range(1, k) for i in range(F - d - 1)], np.int32).reshape(-1, 3)
    return pairs, links


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--min-shared", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
    from tests import scale_model as sc
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    F, k = a.frames, a.window
    pairs, links = window_pairs_and_links(F, k)
    P, L = len(pairs), len(links)
    out = {"frames": F, "window": k, "n_pairs": P, "n_links": L, "nfeatures": a.nfeatures, "max_matches": a.max_matches}
    frames = synthetic.make_stream(F, K, W, H, workers=a.workers)[0]
    e = _capi.Engine(W, H, max_batch=P, nfeatures=a.nfeatures, max_matches=a.max_matches)
    e.frames_reserve(F)
    for s in range(0, F, 2 * P):
        e.frames_put(frames[s:s + 2 * P], np.arange(s, min(s + 2 * P, F), dtype=np.int32))

    def run_pairs():
        return e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)

    def run_links():
        return e.scale_links(links[:, 0], links[:, 1], links[:, 2], a.min_shared)

    def host_fetch():
        R, t, _, nm, st = e.fetch_results(P)
        q, ti = e.fetch_match_indices(P)
        rm, pm, pts = e.fetch_structure(P)
        return sc.Run(q, ti, rm, pm, pts, R, t, st, nm)

    run_pairs()
    got = run_links()
    want = sc.scale_links(host_fetch(), links, a.min_shared)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.allclose(got[0], want[0], rtol=1e-12, atol=0)
    out["links_ok"] = int((got[2] == 0).sum())
    out["n_shared_median"] = float(np.median(got[1]))
    tp, t1, t2, tf, tm = [], [], [], [], []
    for r in range(a.warmup + a.reps):
        marks = [time.perf_counter()]
        run_pairs(); marks.append(time.perf_counter())
        run_links(); marks.append(time.perf_counter())
        run_links(); marks.append(time.perf_counter())
        run_pairs()                                   # the host path starts where the call starts: no structure held
        marks.append(time.perf_counter())
        run = host_fetch(); marks.append(time.perf_counter())
        sc.scale_links(run, links, a.min_shared); marks.append(time.perf_counter())
        if r >= a.warmup:
            d = np.diff(marks)
            tp.append(d[0]); t1.append(d[1]); t2.append(d[2]); tf.append(d[4]); tm.append(d[5])
    out["pairs"] = _stats(tp)
    out["links_first"] = _stats(t1)
    out["links_again"] = _stats(t2)
    out["host_fetch"] = _stats(tf)
    out["host_model"] = _stats(tm)
    out["host_path"] = _stats(np.asarray(tf) + np.asarray(tm))
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
