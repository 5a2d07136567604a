#!/usr/bin/env python3
"""What rpe_link_poses costs: a VGA stream of 1024 frames = 1023 pairs and the links of every two
consecutive pairs (1022 links, side 1), 256 samples, beside the two calls it stands next to on the same run.  The stream
is the 6-frame stream of the tests (scale_model.PHYSICS: consecutive pairs share a few hundred triangulated keypoints)
walked back and forth -- frames 0 1 .. 5 4 .. 0 1 .. -- because synthetic.make_stream's random walk turns away from its
scene over hundreds of frames (165 of 1023 pairs OK at this step), which leaves most links nothing to solve.

  stream           rpe_estimate_stream over the frames (host images in, poses out)
  scale_links      rpe_scale_links with the structure held (the first call after the stream launches the structure
                   kernels and is timed apart as scale_links_first)
  homographies     rpe_pair_homographies over all pairs, the same number of samples
  link_poses_min   rpe_link_poses, refine_iters = 0
  link_poses       rpe_link_poses, refine_iters = 10

Every timed window is a host clock around a call that ends in a stream synchronise and the fetch of its results;
warm-up runs first; median and min / max of the repetitions.  The kernels' own device times come from
`rocprofv3 --kernel-trace --stats -- python tools/bench_link_poses.py` (link_pose_kernel), in a run of its own.  Prints
one JSON line.

    python tools/bench_link_poses.py [--frames 1024] [--iters 256] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--iters", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=6)              # frames rendered; the stream walks them back and forth
    ap.add_argument("--seed", type=int, default=5_000_041)          # the stream of the tests (scale_model.PHYSICS)
    ap.add_argument("--step", type=float, default=0.3)              # a baseline that leaves shared structure: 2.5 .. 7.5 % of the depth
    ap.add_argument("--min-shared", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    F = a.frames
    P, L = F - 1, F - 2
    D = a.distinct
    walk = np.abs((np.arange(F) + D - 1) % (2 * D - 2) - (D - 1))          # 0 1 .. D-1 D-2 .. 1 0 1 ..
    frames = np.ascontiguousarray(synthetic.make_stream(D, K, W, H, seed=a.seed, step=a.step, workers=a.workers)[0][walk])
    e = _capi.Engine(W, H, max_batch=P, nfeatures=a.nfeatures, max_matches=a.max_matches)
    i = np.arange(L, dtype=np.int32)
    links = (i, i + 1, np.ones(L, np.int32))
    calls = {
        "scale_links": lambda: e.scale_links(*links, a.min_shared),
        "homographies": lambda: e.pair_homographies(P, a.iters),
        "link_poses_min": lambda: e.link_poses(*links, iters=a.iters, min_shared=a.min_shared, refine_iters=0),
        "link_poses": lambda: e.link_poses(*links, iters=a.iters, min_shared=a.min_shared, refine_iters=10),
    }
    t = {k: [] for k in ["stream", "scale_links_first"] + list(calls)}
    out = {"frames": F, "n_pairs": P, "n_links": L, "nfeatures": a.nfeatures, "max_matches": a.max_matches, "iters": a.iters,
           "distinct": D, "seed": a.seed, "step": a.step}
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        st = e.estimate_stream(frames, K)[4]
        t1 = time.perf_counter()
        e.scale_links(*links, a.min_shared)
        t2 = time.perf_counter()
        row = {"stream": t1 - t0, "scale_links_first": t2 - t1}
        for k, fn in calls.items():
            t3 = time.perf_counter()
            got = fn()
            row[k] = time.perf_counter() - t3
        if r >= a.warmup:
            for k, v in row.items():
                t[k].append(v)
    out["pairs_ok"] = int((st == 0).sum())
    out["links_ok"] = int((got[4][:, 0] == 0).sum())
    out["n_median"] = float(np.median(got[3][:, 0])); out["inliers_median"] = float(np.median(got[3][:, 1]))
    out["polish_rejected"] = int((got[4][:, 3] < 0).sum())
    for k, v in t.items():
        out[k] = _stats(v)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
