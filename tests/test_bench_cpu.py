"""bench.py's byte accounting and workload arithmetic (no GPU): level sizes against the oracle's pyramid
layout, algorithmic bytes against SURVEY 8(d)'s per-unit figures."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.parametrize("W,H", [(640, 480), (1920, 1080), (848, 478), (96, 96), (333, 257)])
def test_level_sizes_match_the_pyramid_layout(oracle, W, H):
    import bench
    L = oracle.orb_layout(W, H, 1000)
    assert bench.orb_levels(W, H) == [(L.w[l], L.h[l]) for l in range(12)]


def test_algorithmic_bytes():
    import bench
    P = 1590354                                               # VGA pyramid pixels
    assert sum(w * h for w, h in bench.orb_levels(640, 480)) == P
    assert bench.stage_bytes("match", 640, 480, P, 1000, 500) == 72000            # (N1+N2)*32 + N1*8
    assert bench.stage_bytes("pyramid", 640, 480, P, 1000, 500) == 2 * (307200 + P)
    fast = bench.stage_bytes("fast", 640, 480, P, 1000, 500)
    # list-emitting FAST: the border-filtered pyramid region of two images read ONCE (less than 2 P) + a few KB of
    # keypoint list entries and histograms; no dense NMS map is written any more
    assert 1.2 * P < fast < 2 * P
    assert bench.stage_bytes("select", 640, 480, P, 1000, 500) < 0.1 * P
    assert bench.stage_bytes("ransac", 640, 480, P, 1000, 500) == 8500
    oc = bench.sift_octaves(1920, 1080)
    assert oc[0] == (3840, 2160) and len(oc) == 10             # base 3840x2160, 10 octaves
    assert bench.stage_bytes("match", 1920, 1080, 0, 2048, 500, "SIFT") == 2 * 2048 * 128 + 2048 * 8
    px = sum(w * h for w, h in oc)
    assert bench.stage_bytes("pyramid", 1920, 1080, 0, 2048, 500, "SIFT") == 2 * (1920 * 1080 + 24 * px)
    with pytest.raises(KeyError):
        bench.stage_bytes("nope", 640, 480, P, 1000, 500)


def test_plain_run_options(monkeypatch):
    """a plain run is the headline alone; --full and --dump-outputs are opt-in; --steps below 1 is refused before any work"""
    import subprocess
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, "")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], env=env, capture_output=True, text=True)
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr and p.stdout == ""


def test_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs writes every pair's pose record in pair order as float64, and a fixed sample above the size limit"""
    import numpy as np
    import bench
    from relative_pose_estimation_amd import sharding
    rng = np.random.default_rng(1)
    n = 40
    R, t = rng.standard_normal((n, 3, 3)), rng.standard_normal((n, 3, 1))
    inl, st, nm = rng.integers(0, 500, n), rng.integers(0, 5, n), rng.integers(0, 500, n)
    rec = sharding.pack_records(R, t, inl, st, nm)
    names = ("R", "t", "inliers", "n_matches", "status", "pair")

    def load(d):
        return {k: np.load(os.path.join(d, f"{k}.npy")) for k in names}

    bench.dump_outputs(str(tmp_path / "all"), rec[::-1])          # gathered records need not arrive in pair order
    got = load(tmp_path / "all")
    assert all(v.dtype == np.float64 for v in got.values())
    for k, v in zip(names, (R, t, inl, nm, st, np.arange(n))):
        assert np.array_equal(got[k], v), k
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 128)
    bench.dump_outputs(str(tmp_path / "s1"), rec)
    bench.dump_outputs(str(tmp_path / "s2"), rec[::-1])
    s1, s2 = load(tmp_path / "s1"), load(tmp_path / "s2")
    assert sum(v.nbytes for v in s1.values()) <= 10 * 128
    assert all(np.array_equal(s1[k], s2[k]) for k in names)
    pair = s1["pair"].astype(int)
    assert len(pair) == 10 and np.all(np.diff(pair) > 0) and np.array_equal(s1["R"], R[pair]) and np.array_equal(s1["status"], st[pair])
