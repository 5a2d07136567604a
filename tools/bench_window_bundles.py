#!/usr/bin/env python3
"""What rpe_bundle_windows costs next to rpe_triangulate_tracks ("Window bundles"): the workload of
tools/bench_track_points.py -- windowed matching over a synthetic stream as ONE pair list (256 VGA frames, window 4: 1014
pairs, ORB-1000 / 500), its USABLE tracks, the chain of the window-1 pairs and its frame groups -- the track points under
that chain, and windows of 8 frames with overlap 2 (geometry.windows_of_groups) bundled over them.

  points        rpe_triangulate_tracks, every output fetched into arrays allocated once
  windows       rpe_bundle_windows over the chain's groups, every output fetched into arrays allocated once: the uploads, the
                three kernels, seven copies back
  windows_one   the same with every frame in one group (points and windows of one group): the load case, as in
                bench_track_points -- the poses across a broken link are on unrelated scales, so the result means little

Every timed window ends in a stream synchronise (the call fetches); warm-up calls first; median and min / max of the
repetitions.  The codes, point counts and iterations are reported, two calls are asserted equal bit for bit, and the same
job is run through the model of tests/window_bundle_model.py as the CPU baseline (and compared: integers).  The kernels'
own device times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_window_bundles.py --no-model`, in a run
of its own.  Prints one JSON line.

    python tools/bench_window_bundles.py [--frames 256] [--window 4] [--size 8] [--overlap 2] [--reps 9] [--no-model]
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
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--max-points", type=int, default=4096)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--max-matches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    ap.add_argument("--no-model", action="store_true", help="skip the Python model (profiling runs)")
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi, geometry, synthetic
    W, H = 640, 480
    K = geometry.default_camera_matrix(W, H)
    F, k = a.frames, a.window
    pairs = np.array([(i, i + d) for d in range(1, k + 1) for i in range(F - d)], np.int32)
    P, mm = len(pairs), a.max_matches
    out = {"frames": F, "window": k, "n_pairs": P, "size": a.size, "overlap": a.overlap, "max_points": a.max_points}
    frames = synthetic.make_stream(F, K, W, H, workers=a.workers)[0]
    print("frames rendered", file=sys.stderr, flush=True)
    e = _capi.Engine(W, H, max_batch=P, nfeatures=a.nfeatures, max_matches=mm)
    e.frames_reserve(F)
    for s in range(0, F, 2 * P):
        e.frames_put(frames[s:s + 2 * P], np.arange(s, min(s + 2 * P, F), dtype=np.int32))
    R, t, _, _, st = e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)
    i = np.arange(F - 2, dtype=np.int32)
    stats, _, code = e.scale_links(i, i + 1, np.ones(F - 2, np.int32))
    R_abs, T_abs, _, _, segment = geometry.chain_trajectory(R[:F - 1], t[:F - 1], st[:F - 1], stats[:, 1], code)
    group = geometry.frame_groups(st[:F - 1], segment)
    tracks = e.build_tracks()
    n_t, n_o = tracks["n_tracks"], tracks["n_obs"]
    out["n_tracks"], out["n_obs"], out["segments"] = n_t, n_o, int(segment.max()) + 1

    jobs = {}
    for name, g in (("windows", group), ("windows_one", None)):
        pts = e.triangulate_tracks(tracks, R_abs, T_abs, K=K, frame_group=g)
        wins = geometry.windows_of_groups(np.zeros(F, np.int32) if g is None else g, a.size, a.overlap)
        use = (pts["code"] == _capi.TRACKPT_OK).astype(np.uint8)
        res = e.bundle_windows(tracks, pts["points"], R_abs, T_abs, wins, K=K, obs_use=pts["obs_flag"], point_use=use, max_points=a.max_points)
        again = e.bundle_windows(tracks, pts["points"], R_abs, T_abs, wins, K=K, obs_use=pts["obs_flag"], point_use=use, max_points=a.max_points)
        for key in ("code", "n_points", "n_obs", "iterations", "accepted", "rms"):
            assert np.array_equal(res[key].view(np.uint8), again[key].view(np.uint8)), key
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(res["R"] + res["T"] + res["points"], again["R"] + again["T"] + again["points"]))
        ok = res["code"] == _capi.WINDOW_OK
        out[name + "_job"] = {"n_win": len(wins), "sizes": np.bincount([len(w) for w in wins], minlength=9).tolist(),
                              "codes": dict(zip(_capi.WINDOW_NAMES, np.bincount(res["code"], minlength=4).tolist())),
                              "points_sum": int(res["n_points"].sum()), "points_max": int(res["n_points"].max()) if len(wins) else 0,
                              "obs_sum": int(res["n_obs"].sum()), "dropped": int(res["dropped"].sum()),
                              "iterations_sum": int(res["iterations"].sum()), "iterations_max": int(res["iterations"].max()) if len(wins) else 0,
                              "rms_ok_before_px": round(float(np.median(res["rms"][ok, 0])), 4) if ok.any() else None,
                              "rms_ok_after_px": round(float(np.median(res["rms"][ok, 1])), 4) if ok.any() else None}
        jobs[name] = (pts, wins, use, res, g)
        if not a.no_model:
            from tests import camera_model as cm
            from tests import window_bundle_model as wm
            t0 = time.perf_counter()
            want = wm.bundle_windows(tracks, pts["points"], R_abs, T_abs, wins, cm.Cam(K), pts["obs_flag"], use, a.max_points, 8, 10)
            out[name + "_job"]["model_s"] = round(time.perf_counter() - t0, 2)
            same = sum(int(res["code"][w] == r["code"] and res["n_points"][w] == r["counts"][1] and res["iterations"][w] == r["info"][1])
                       for w, r in enumerate(want))
            out[name + "_job"]["windows_equal_model_integers"] = same
            assert same == len(want), (name, same, len(want))

    ins = [np.ascontiguousarray(tracks["track_start"], np.int32), np.ascontiguousarray(tracks["obs_frame"], np.int32),
           np.ascontiguousarray(tracks["obs_xy"], np.float32), np.ascontiguousarray(R_abs), np.ascontiguousarray(T_abs),
           np.ascontiguousarray(K, np.float64)]
    ts, of, xy, Ra, Ta, Kc = [b.ctypes.data for b in ins]
    tp_out = [np.zeros((n_t, 3)), np.zeros((n_t, 4), np.int32), np.zeros(n_t), np.zeros(n_t), np.zeros(n_o, np.uint8), np.zeros(n_o)]
    gk = np.ascontiguousarray(group, np.int32)

    def call_points():
        rc = e.lib.rpe_triangulate_tracks(e.h, n_t, ts, of, xy, F, Ra, Ta, gk.ctypes.data, Kc, None, 2.0, 2, 1.0, 10, *[b.ctypes.data for b in tp_out])
        assert rc == 0, e.lib.rpe_last_error(e.h)

    calls = {}
    for name, (pts, wins, use, res, g) in jobs.items():
        nw = len(wins)
        ws = np.zeros(nw + 1, np.int32); ws[1:] = np.cumsum([len(w) for w in wins])
        wf = np.ascontiguousarray(np.concatenate(wins), np.int32)
        p0 = np.ascontiguousarray(pts["points"]); ou = np.ascontiguousarray(pts["obs_flag"]); pu = np.ascontiguousarray(use)
        slots = nw * a.max_points
        ob = [np.zeros((int(ws[-1]), 9)), np.zeros((int(ws[-1]), 3)), np.zeros((slots, 3)), np.zeros(slots, np.int32), np.zeros((nw, 4), np.int32),
              np.zeros((nw, 4), np.int32), np.zeros((nw, 2))]
        keep = (ws, wf, p0, ou, pu, ob)

        def call(keep=keep, nw=nw):
            ws, wf, p0, ou, pu, ob = keep
            rc = e.lib.rpe_bundle_windows(e.h, n_t, ts, of, xy, p0.ctypes.data, pu.ctypes.data, ou.ctypes.data, F, Ra, Ta, Kc, None, nw,
                                          ws.ctypes.data, wf.ctypes.data, a.max_points, 8, 10, *[b.ctypes.data for b in ob])
            assert rc == 0, e.lib.rpe_last_error(e.h)
        calls[name] = call
        out[name + "_job"]["bytes_up"] = int(sum(b.nbytes for b in ins[:5]) + p0.nbytes + ou.nbytes + pu.nbytes + ws.nbytes + wf.nbytes + 96)
        out[name + "_job"]["bytes_down"] = int(sum(b.nbytes for b in ob))

    tp, tw, to = [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter(); call_points(); t1 = time.perf_counter()
        calls["windows"](); t2 = time.perf_counter()
        calls["windows_one"](); t3 = time.perf_counter()
        if r >= a.warmup:
            tp.append(t1 - t0); tw.append(t2 - t1); to.append(t3 - t2)
    out["points"] = _stats(tp)
    out["windows"] = _stats(tw)
    out["windows_one"] = _stats(to)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
