#!/usr/bin/env python3
"""What rpe_build_tracks costs next to the run it follows: windowed matching over a synthetic stream
as ONE pair list (256 VGA frames, window 4: 1014 pairs, ORB-1000 / 500), then the tracks of the run under each edge rule.

  pairs            rpe_estimate_pairs over the list (the frames are put once, outside the timed window)
  tracks_<rule>    rpe_build_tracks with every output fetched into arrays allocated once (the structure of the run is held:
                   the call before the timed ones has launched the structure kernels)
  tracks_first     the first rpe_build_tracks after a pair list under RPE_TRACK_EDGES_USABLE: structure kernels included
  wrapper_usable   _capi.Engine.build_tracks: the same call plus the allocation and trimming of the dict

Every timed window ends in a stream synchronise (the call fetches); warm-up runs first; median and min / max of the
repetitions.  The counts, the length histogram and the conflict share of each rule are reported, and the result under
RPE_TRACK_EDGES_USABLE is asserted equal to the model of tests/track_model.py.  The kernels' own device times come from
`rocprofv3 --kernel-trace --stats -- python tools/bench_tracks.py`, in a run of its own.  Prints one JSON line.

    python tools/bench_tracks.py [--frames 256] [--window 4] [--reps 9]
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
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
    from tests import scale_model as sc
    from tests import track_model as tm
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    F, k = a.frames, a.window
    pairs = np.array([(i, i + d) for d in range(1, k + 1) for i in range(F - d)], np.int32)
    P, mm = len(pairs), a.max_matches
    out = {"frames": F, "window": k, "n_pairs": P, "nfeatures": a.nfeatures, "max_matches": mm}
    frames = synthetic.make_stream(F, K, W, H, workers=a.workers)[0]
    print("frames rendered", file=sys.stderr, flush=True)
    e = _capi.Engine(W, H, max_batch=P, nfeatures=a.nfeatures, max_matches=mm)
    e.frames_reserve(F)
    for s in range(0, F, 2 * P):
        e.frames_put(frames[s:s + 2 * P], np.arange(s, min(s + 2 * P, F), dtype=np.int32))
    n = P * mm
    bufs = [np.zeros(6, np.int32), np.zeros(n + 1, np.int32), np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32),
            np.zeros((2 * n, 2), np.float32), np.zeros((P, mm), np.int32)]
    ptrs = [b.ctypes.data for b in bufs]

    def run_pairs():
        return e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)

    def call(rule):
        rc = e.lib.rpe_build_tracks(e.h, None, rule, 2, *ptrs)
        assert rc == 0, e.lib.rpe_last_error(e.h)

    res = run_pairs()
    out["pairs_ok"] = int((res[4] == 0).sum())
    rules = (("usable", _capi.TRACK_EDGES_USABLE), ("ransac", _capi.TRACK_EDGES_RANSAC), ("all", _capi.TRACK_EDGES_ALL))
    for name, rule in rules:
        tr = e.build_tracks(edge_rule=rule)
        lengths = geometry.track_lengths(tr)
        comps = tr["n_tracks"] + tr["dropped_conflict"] + tr["dropped_short"]
        out["counts_" + name] = {c: tr[c] for c in _capi.TRACK_COUNTS}
        out["lengths_" + name] = np.bincount(lengths).tolist()
        out["conflict_share_" + name] = round(tr["dropped_conflict"] / max(comps, 1), 4)
        if rule == _capi.TRACK_EDGES_USABLE:
            R, t, _, nm, st = e.fetch_results(P)
            q, ti = e.fetch_match_indices(P)
            rm, pm, pts = e.fetch_structure(P)
            p1, p2 = e.fetch_matched_points(P)
            run = sc.Run(q, ti, rm, pm, pts, R, t, st, nm)
            want = tm.build_tracks(F, e.kcap, pairs[:, 0], pairs[:, 1], q, ti, tm.run_edges(run, tm.EDGES_USABLE), p1, p2, 2)
            tm.assert_equal(tr, want)
            out["equals_model"] = True
    tp, tf, tw = [], [], []
    tr_ = {name: [] for name, _ in rules}
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter(); run_pairs(); t1 = time.perf_counter()
        call(_capi.TRACK_EDGES_USABLE); t2 = time.perf_counter()
        d = {}
        for name, rule in rules:
            s0 = time.perf_counter(); call(rule); d[name] = time.perf_counter() - s0
        s0 = time.perf_counter(); e.build_tracks(); w = time.perf_counter() - s0
        if r >= a.warmup:
            tp.append(t1 - t0); tf.append(t2 - t1); tw.append(w)
            for name in d:
                tr_[name].append(d[name])
    out["pairs"] = _stats(tp)
    out["tracks_first"] = _stats(tf)
    for name, _ in rules:
        out["tracks_" + name] = _stats(tr_[name])
    out["wrapper_usable"] = _stats(tw)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
