#!/usr/bin/env python3
"""What the pair proposals cost ("Pair proposals"): rpe_frames_similar over a resident synthetic stream,
all frames against all, on the GPU:

  step = 1 and step = 4, scores only; k = 3 candidates only; rectangular lists (no triangle); one query against the store;

next to the parent's only route to a ranking, rpe_estimate_pairs over the same pairs of distinct frames in chunks of
max_batch.  Every call is synchronous (it ends in the wait of its fetch), so the host clock around it is the call time;
warm-up calls run first; median and min / max of the repetitions are reported.  Prints one JSON document.

    python tools/bench_similarity.py [--frames 256] [--max-batch 512] [--reps 12] [--no-baseline] [--out FILE]
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


def _timed(fn, reps, warm=2):
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append((time.perf_counter() - t) * 1e3)
    ts = np.array(ts)
    return out, dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(ts.min()), 3), max_ms=round(float(ts.max()), 3), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--max-batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--max-distance", type=int, default=48)
    ap.add_argument("--no-baseline", action="store_true", help="skip rpe_estimate_pairs over all pairs (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from relative_pose_estimation_amd import _capi, geometry, synthetic
    N, MB, md = a.frames, a.max_batch, a.max_distance
    K = geometry.default_camera_matrix(640, 480)
    frames = synthetic.make_stream(N, K, workers=min(16, os.cpu_count() or 1))[0]          # the stream of tools/bench_pairs.py
    e = _capi.Engine(640, 480, max_batch=MB, nfeatures=1000, max_matches=500)
    e.frames_reserve(N)
    slots = np.arange(N, dtype=np.int32)
    for s in range(0, N, 2 * MB):
        e.frames_put(frames[s:s + 2 * MB], slots[s:s + 2 * MB])
    cnt, _ = e.frames_info(slots)
    res = {"frames": N, "pairs_scored": N * (N + 1) // 2, "keypoints_min": int(cnt.min()), "keypoints_median": int(np.median(cnt)),
           "max_distance": md}
    assert cnt.min() >= 900, "a frame with few keypoints makes its pairs cheap: the figures would flatter the kernel"
    s1, res["step1_scores_only"] = _timed(lambda: e.frames_similar(slots, slots, step=1, max_distance=md), a.reps)
    _, res["step4_scores_only"] = _timed(lambda: e.frames_similar(slots, slots, step=4, max_distance=md), a.reps)
    _, res["step1_k3_candidates_only"] = _timed(lambda: e.frames_similar(slots, slots, step=1, max_distance=md, k=3, exclude=3, want_scores=False), a.reps)
    _, res["step4_k3_candidates_only"] = _timed(lambda: e.frames_similar(slots, slots, step=4, max_distance=md, k=3, exclude=3, want_scores=False), a.reps)
    _, res["step1_rect_scores_only"] = _timed(lambda: e.frames_similar(slots, np.roll(slots, 1), step=1, max_distance=md), max(3, a.reps // 3))
    _, res["step1_one_query"] = _timed(lambda: e.frames_similar(slots[:1], slots, step=1, max_distance=md), a.reps)
    S = s1["scores"]
    assert np.array_equal(S, S.T) and (np.diag(S) >= cnt - 8).all()
    if not a.no_baseline:
        iu = np.triu_indices(N, 1)
        p1, p2 = iu[0].astype(np.int32), iu[1].astype(np.int32)

        def all_pairs():
            return np.concatenate([e.estimate_pairs(p1[s:s + MB], p2[s:s + MB], K)[3] for s in range(0, p1.size, MB)])

        nm, res["estimate_pairs_all"] = _timed(all_pairs, 3, warm=1)
        res["estimate_pairs_all"].update(pairs=int(p1.size), max_batch=MB)
        res["n_matches_capped_at_max_matches"] = float(np.mean(nm == 500))
    e.close()
    doc = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
