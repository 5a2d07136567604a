#!/usr/bin/env python3
"""What rpe_triangulate_tracks costs next to rpe_build_tracks ("Track points"): the workload of
tools/bench_tracks.py -- windowed matching over a synthetic stream as ONE pair list (256 VGA frames, window 4: 1014 pairs,
ORB-1000 / 500) -- its tracks under RPE_TRACK_EDGES_USABLE, and the frames' absolute poses from the window-1 pairs of the
same run (their scale links, geometry.chain_trajectory, geometry.frame_groups).

  tracks        rpe_build_tracks, every output fetched into arrays allocated once (the structure of the run is held)
  points        rpe_triangulate_tracks over those tracks, every output fetched into arrays allocated once: the uploads of
                the tracks, poses and groups, the two kernels, six copies back
  wrapper       _capi.Engine.triangulate_tracks: the same call plus the allocation of the dict
  points_one    the same call with frame_group NULL: every frame in one group, so every observation is used.  The chain of
                this stream breaks into many short segments (its links share few keypoints), which leaves most tracks
                without two views in their group; under one group the poses across a break are on unrelated scales, so the
                points mean little, but the kernel does the work of a chain that holds: the load case of the call

Every timed window ends in a stream synchronise (the call fetches); warm-up calls first; median and min / max of the
repetitions.  The code histogram, the inlier share and the rms of the OK tracks are reported, and the result is asserted
equal to the model of tests/track_point_model.py, bit for bit.  The kernels' own device times come from
`rocprofv3 --kernel-trace --stats -- python tools/bench_track_points.py --no-model`, in a run of its own.  Prints one JSON
line.

    python tools/bench_track_points.py [--frames 256] [--window 4] [--reps 9] [--no-model]
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
    ap.add_argument("--no-model", action="store_true", help="skip the comparison with the Python model (profiling runs)")
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
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
    R, t, _, _, st = e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)
    out["pairs_ok"] = int((st == 0).sum())
    # the chain of the window-1 pairs: pair i joins frames i and i + 1 for i < F - 1
    i = np.arange(F - 2, dtype=np.int32)
    stats, _, code = e.scale_links(i, i + 1, np.ones(F - 2, np.int32))
    R_abs, T_abs, _, _, segment = geometry.chain_trajectory(R[:F - 1], t[:F - 1], st[:F - 1], stats[:, 1], code)
    group = geometry.frame_groups(st[:F - 1], segment)
    out["segments"] = int(segment.max()) + 1
    tracks = e.build_tracks()
    n_t, n_o = tracks["n_tracks"], tracks["n_obs"]
    out["n_tracks"], out["n_obs"] = n_t, n_o
    out["lengths"] = np.bincount(geometry.track_lengths(tracks)).tolist()

    res = e.triangulate_tracks(tracks, R_abs, T_abs, K=K, frame_group=group)
    used = res["obs_flag"] > 0
    ok = res["code"] == _capi.TRACKPT_OK
    out["codes"] = dict(zip(_capi.TRACKPT_NAMES, np.bincount(res["code"], minlength=6).tolist()))
    out["used_share"] = round(float(used.mean()), 4)
    out["inlier_share_of_used"] = round(float((res["obs_flag"] == 1).sum() / max(int(used.sum()), 1)), 4)
    out["median_rms_ok_px"] = round(float(np.median(res["rms"][ok])), 4) if ok.any() else None
    out["iterations_mean"] = round(float(res["iterations"].mean()), 3)
    out["iterations_max"] = int(res["iterations"].max())
    one = e.triangulate_tracks(tracks, R_abs, T_abs, K=K)
    out["one_group"] = {"codes": dict(zip(_capi.TRACKPT_NAMES, np.bincount(one["code"], minlength=6).tolist())),
                        "inlier_share_of_used": round(float((one["obs_flag"] == 1).mean()), 4),
                        "iterations_mean": round(float(one["iterations"].mean()), 3), "iterations_max": int(one["iterations"].max())}
    if not a.no_model:
        from tests import camera_model as cm
        from tests import track_point_model as tm
        t0 = time.perf_counter()
        tm.assert_equal(res, tm.triangulate_tracks(tracks, R_abs, T_abs, cm.Cam(K), group))
        out["equals_model"] = True
        out["model_s"] = round(time.perf_counter() - t0, 2)

    n = P * mm
    tb = [np.zeros(6, np.int32), np.zeros(n + 1, np.int32), np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32),
          np.zeros((2 * n, 2), np.float32), np.zeros((P, mm), np.int32)]
    tptr = [b.ctypes.data for b in tb]
    ins = [np.ascontiguousarray(tracks["track_start"], np.int32), np.ascontiguousarray(tracks["obs_frame"], np.int32),
           np.ascontiguousarray(tracks["obs_xy"], np.float32), np.ascontiguousarray(R_abs), np.ascontiguousarray(T_abs),
           np.ascontiguousarray(group, np.int32), np.ascontiguousarray(K, np.float64)]
    ts, of, xy, Ra, Ta, g, Kc = [b.ctypes.data for b in ins]
    ob = [np.zeros((n_t, 3)), np.zeros((n_t, 4), np.int32), np.zeros(n_t), np.zeros(n_t), np.zeros(n_o, np.uint8), np.zeros(n_o)]
    optr = [b.ctypes.data for b in ob]

    def call_tracks():
        rc = e.lib.rpe_build_tracks(e.h, None, _capi.TRACK_EDGES_USABLE, 2, *tptr)
        assert rc == 0, e.lib.rpe_last_error(e.h)

    def call_points(groups):
        rc = e.lib.rpe_triangulate_tracks(e.h, n_t, ts, of, xy, F, Ra, Ta, groups, Kc, None, 2.0, 2, 1.0, 10, *optr)
        assert rc == 0, e.lib.rpe_last_error(e.h)

    # tp_solve launches in order: two above, then three per round (points, wrapper, points_one)
    tt, tp, tw, to = [], [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter(); call_tracks(); t1 = time.perf_counter()
        call_points(g); t2 = time.perf_counter()
        e.triangulate_tracks(tracks, R_abs, T_abs, K=K, frame_group=group); t3 = time.perf_counter()
        if r == 0:
            assert np.array_equal(ob[0], res["points"]) and np.array_equal(ob[4], res["obs_flag"])
        t4 = time.perf_counter(); call_points(None); t5 = time.perf_counter()
        if r >= a.warmup:
            tt.append(t1 - t0); tp.append(t2 - t1); tw.append(t3 - t2); to.append(t5 - t4)
    assert np.array_equal(ob[0], one["points"]) and np.array_equal(ob[4], one["obs_flag"])
    out["tracks"] = _stats(tt)
    out["points"] = _stats(tp)
    out["wrapper"] = _stats(tw)
    out["points_one"] = _stats(to)
    out["bytes_up"] = int(sum(b.nbytes for b in ins[:6]) + 96)
    out["bytes_down"] = int(sum(b.nbytes for b in ob))
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
