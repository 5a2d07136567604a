#!/usr/bin/env python3
"""What the frame store buys: windowed matching over a synthetic stream, two ways, on the GPU.

  (a) batch form     rpe_enqueue_batch_device on the gathered, duplicated image pairs in chunks of max_batch
                     (every pair extracts both of its images)
  (b) frame store    rpe_frames_put_device of the frames once + rpe_enqueue_pairs over the same list

and the online step: one new frame put into a ring + three pairs against the previous frames, next to
PoseEstimator.estimate of one pair.  Results of (a) and (b) are asserted bit-equal.  Every timed window ends in a
stream synchronise (fetch_results / frames_info); warm-up runs first; median and min / max of the repetitions are
reported.  Prints one JSON line.

    python tools/bench_pairs.py [--frames 256] [--window 4] [--max-batch 256] [--reps 7]
    python tools/bench_pairs.py --online-only            # estimate() alone (also runs on a library without the store)
"""
import argparse
import ctypes as C
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


def _timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def slot_bytes(kcap, desc_bytes, l2):
    """bytes of one store slot: descriptors + kp_pt (+ the norm words of NORM_L2 handles) per keypoint row, count and flags"""
    return kcap * (desc_bytes + 8 + (8 if l2 else 0)) + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--online-reps", type=int, default=200)
    ap.add_argument("--online-only", action="store_true")
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    from relative_pose_estimation_amd import PoseEstimator, _capi, geometry, synthetic
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    out = {"frames": a.frames, "window": a.window, "max_batch": a.max_batch, "nfeatures": a.nfeatures, "max_matches": a.max_matches}

    # ---- online step, through the Python front-end (host images in, poses out)
    fr = synthetic.make_stream(8, K, W, H, workers=min(8, a.workers))[0]
    pe = PoseEstimator(K, nfeatures=a.nfeatures, max_matches=a.max_matches, max_batch=4)
    state = {"i": 0}

    def one_estimate():
        i = state["i"] = (state["i"] + 1) % 7
        pe.estimate(fr[i], fr[i + 1])
    out["online_estimate_one_pair"] = _stats(_timed(one_estimate, 20, a.online_reps))
    if not a.online_only:
        ring = pe.frame_store(4)
        ring.put_many([0, 1, 2], fr[:3])
        state["i"] = 3

        def one_step():
            i = state["i"]
            ring.put(i % 4, fr[i % 8])
            ring.estimate([((i - d) % 4, i % 4) for d in (1, 2, 3)])
            state["i"] = i + 1
        out["online_put_plus_3_pairs"] = _stats(_timed(one_step, 20, a.online_reps))

        def put_only():
            i = state["i"]
            ring.put(i % 4, fr[i % 8])
            ring.info([i % 4])
            state["i"] = i + 1
        out["online_put_alone"] = _stats(_timed(put_only, 20, a.online_reps))
        ring.close()
    pe.close()
    if a.online_only:
        print(json.dumps(out))
        return

    # ---- windowed matching
    F, k, MB = a.frames, a.window, a.max_batch
    frames = synthetic.make_stream(F, K, W, H, workers=a.workers)[0]
    lst = np.array([(i, i + d) for d in range(1, k + 1) for i in range(F - d)], np.int32)
    P = len(lst)
    out["pairs"] = P
    e = _capi.Engine(W, H, max_batch=MB, nfeatures=a.nfeatures, max_matches=a.max_matches)
    img = W * H
    d_frames = e.upload(frames)
    d1 = e.upload(frames[lst[:, 0]]); d2 = e.upload(frames[lst[:, 1]])
    chunks = [(s, min(s + MB, P)) for s in range(0, P, MB)]

    def run_batches():
        res = []
        for s, t in chunks:
            res.append(e.estimate_batch_device(C.c_void_p(d1.value + s * img), C.c_void_p(d2.value + s * img), t - s, K))
        return [np.concatenate([r[f] for r in res]) for f in range(5)]

    e.frames_reserve(F)
    slots = np.arange(F, dtype=np.int32)

    def put_all():
        for s in range(0, F, 2 * MB):
            n = min(2 * MB, F - s)
            e.frames_put_device(C.c_void_p(d_frames.value + s * img), n, slots[s:s + n])

    def run_pairs():
        res = []
        for s, t in chunks:
            res.append(e.estimate_pairs(lst[s:t, 0], lst[s:t, 1], K))
        return [np.concatenate([r[f] for r in res]) for f in range(5)]

    def run_store():
        put_all()
        return run_pairs()

    def put_sync():
        put_all()
        e.synchronize()

    ra, rb = run_batches(), run_store()
    for f in range(5):
        x, y = ra[f], rb[f]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f"batch form and frame store differ in field {f}"
    out["bit_equal"] = True
    out["status_ok"] = int((ra[4] == 0).sum())
    # alternate the two forms so that both see the same machine
    ta, tb, tp, tq = [], [], [], []
    for r in range(a.warmup + a.reps):
        for fn, dst in ((run_batches, ta), (run_store, tb), (put_sync, tp), (run_pairs, tq)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                dst.append(dt)
    out["a_batches"] = _stats(ta)
    out["b_put_plus_pairs"] = _stats(tb)
    out["b_put_alone"] = _stats(tp)
    out["b_pairs_alone"] = _stats(tq)
    out["ratio_a_over_b"] = round(out["a_batches"]["median_ms"] / out["b_put_plus_pairs"]["median_ms"], 3)
    out["put_share_of_b"] = round(out["b_put_alone"]["median_ms"] / out["b_put_plus_pairs"]["median_ms"], 3)
    cnt, _ = e.frames_info(slots)
    rows = int(np.minimum(cnt, e.kcap).sum())
    out["scatter_bytes_read_plus_written"] = 2 * (rows * (32 + 8) + 8 * F)
    out["keypoints_mean"] = round(float(cnt.mean()), 1)
    try:
        out["hbm_stream_bytes_per_s"] = e.calibrate_hbm()
    except _capi.RpeError as err:
        out["hbm_stream_bytes_per_s"] = str(err)
    out["slot_bytes"] = {"orb1000_hamming": slot_bytes(1064, 32, False), "orb1000_l2": slot_bytes(1064, 32, True),
                         "sift2048_l2": slot_bytes(2112, 128, True), "sift_uncapped_l2": slot_bytes(16384, 128, True)}
    e.synchronize()
    for p in (d_frames, d1, d2):
        e.device_free(p)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
