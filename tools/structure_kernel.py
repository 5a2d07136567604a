"""Kernel time of rpe_fetch_structure's two launches (ransac_mask_kernel, pose_structure_kernel) at the bench's batch:
1024 VGA pairs, ORB(1000) + Hamming, max_matches 500 -- 8 synthetic pairs tiled (the per-pair work is that of a real
pair; generating 1024 distinct scenes would take minutes of host time).  One device-resident batch, then --fetches
fetches.  Run under the profiler from the repo root:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/structure_kernel.py"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from relative_pose_estimation_amd import _capi, synthetic, geometry
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fetches", type=int, default=10)
    args = ap.parse_args()
    K = geometry.default_camera_matrix(640, 480)
    i1, i2, _, _ = synthetic.make_batch(8, K, cfg=2)
    idx = np.arange(args.batch) % 8
    e = _capi.Engine(640, 480, max_batch=args.batch, nfeatures=1000, max_matches=500)
    da, db = e.upload(i1[idx]), e.upload(i2[idx])
    R, t, inl, nm, st = e.estimate_batch_device(da, db, args.batch, K)
    for _ in range(args.fetches):
        rm, pm, pts = e.fetch_structure(args.batch)
    assert np.array_equal(pm.sum(1), inl)
    print(f"pairs {args.batch}, status OK {int((st == 0).sum())}, mean inliers {inl.mean():.1f}, "
          f"mean RANSAC inliers {rm.sum(1).mean():.1f}, mean matches {nm.mean():.1f}")
    e.close()


if __name__ == "__main__":
    main()
