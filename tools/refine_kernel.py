"""Kernel time of rpe_refine_poses' two launches (ransac_mask_kernel, pose_refine_kernel) at the bench's batch: 1024 VGA
pairs, ORB(1000) + Hamming, max_matches 500 -- 128 synthetic pairs tiled.  One device-resident batch, then --calls
refinements of --iters iterations.  Run under the profiler from the repo root:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/refine_kernel.py
--calibrate prints the measured v_fma_f64 issue rate (rpe_calibrate_valu kind 7) instead."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from relative_pose_estimation_amd import _capi, synthetic, geometry
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calibrate", action="store_true")
    args = ap.parse_args()
    K = geometry.default_camera_matrix(640, 480)
    e = _capi.Engine(640, 480, max_batch=args.batch, nfeatures=1000, max_matches=500)
    if args.calibrate:
        for w in (1, 2, 4):
            name, rate = e.calibrate_valu(7, w)
            print(f"kind 7 ({name}), {w} waves per SIMD: {rate:.4g} wave-instructions/s")
        e.close()
        return
    i1, i2, _, _ = synthetic.make_batch(128, K, cfg=2, workers=16)
    idx = np.arange(args.batch) % 128
    da, db = e.upload(i1[idx]), e.upload(i2[idx])
    R, t, inl, nm, st = e.estimate_batch_device(da, db, args.batch, K)
    for _ in range(args.calls):
        Rr, tr, inr, info, rms = e.refine_poses(args.batch, args.iters)
    print(f"pairs {args.batch}, codes {np.bincount(info[:, 0], minlength=3).tolist()}, mean iterations {info[:, 1].mean():.2f}, "
          f"mean residuals {info[:, 2].mean():.1f}, mean matches {nm.mean():.1f}, rms {rms[:, 0].mean():.4f} -> {rms[:, 1].mean():.4f}")
    e.close()


if __name__ == "__main__":
    main()
