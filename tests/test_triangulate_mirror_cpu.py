"""relative_pose_estimation_amd/csrc/pose_triangulate.h on the host: triangulate_pm takes the cheirality verdicts of
(R, t) and (R, -t) from ONE Jacobi SVD (the -t system is the +t one with its last column negated, and every quantity of the
SVD is then the same or exactly negated), and falls back on a direct triangulation when a rotation with that column meets
zeta == +-0 (the one asymmetric statement, `zeta >= 0. ? 1. : -1.`).  tests/native/triangulate_mirror_host.cpp runs it
against triangulate_one called for t and for -t; it is built without floating-point contraction (the device build's
setting), with contraction and FMA (the identity does not depend on it), and once with the host sanitizers.

Every comparison is bit for bit (memcmp in the program), no tolerance anywhere.

The crafted case R = I, t = (-1, -1, 0), x1 = y1 = x2 = 0, y2 = 0.3: columns 0 and 3 of the system are (-1, 0, -1, 0) and
(0, 0, 1, 1), the rotations (0, 1) and (0, 2) are skipped (ga = 0 and ga = -x1 = 0), and (0, 3) meets al = be = 2, ga = -1.
That holds for every y1 and y2, so the tie is required of every variant with x1 = 0.  With x1 != 0 the rotation (0, 2) runs
first and unbalances column 0; the tie then does not occur (and need not): those variants must still agree with the direct
triangulation, by the mirror if no tie is flagged."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "triangulate_mirror_host.cpp")
BUILD = os.path.join(HERE, "native", "build")

FLAVOURS = {
    "nocontract": ["-O2", "-ffp-contract=off"],
    "contract": ["-O2", "-ffp-contract=fast", "-march=native"],
    "sanitized": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
N_RANDOM = {"nocontract": 200000, "contract": 200000, "sanitized": 20000}


@pytest.fixture(scope="module", params=list(FLAVOURS))
def prog(request):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "triangulate_mirror_host_" + request.param)
    subprocess.check_call(["g++", "-std=c++17"] + FLAVOURS[request.param] + ["-o", out, SRC])
    return request.param, out


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split())}


def test_mirror_equals_direct_on_random_cases(prog):
    flavour, exe = prog
    r = _run(exe, "random", N_RANDOM[flavour], 20240919)
    print(r)
    assert r["cases"] == N_RANDOM[flavour]
    assert r["bad_plus"] == 0                    # good_plus and P_plus are triangulate_one(R, t)'s
    assert r["bad_verdict"] == 0                 # good_minus is triangulate_one(R, -t)'s
    assert r["bad_point"] == 0                   # the direct point of -t is -P_plus, bit for bit
    assert r["ties"] == 0                        # random scenes do not raise the tie
    assert r["plus_good"] > r["cases"] // 10 and r["minus_good"] > r["cases"] // 10        # both verdicts are exercised


def test_crafted_tie_takes_the_fallback(prog):
    _, exe = prog
    base = _run(exe, "crafted", 0, 0, 0.3)
    print(base)
    assert base["tie"] == 1 and base["verdicts_equal"] == 1 and base["plus_equal"] == 1
    assert base["point_mirrors"] == 0            # the identity is really broken here: the fallback is needed
    rng = np.random.default_rng(31)
    for _ in range(12):                          # x1 = 0: the tie for every y1, y2
        y1, y2 = rng.uniform(-0.5, 0.5, 2).round(4)
        r = _run(exe, "crafted", 0, y1, y2)
        assert r["tie"] == 1 and r["verdicts_equal"] == 1 and r["plus_equal"] == 1, (y1, y2, r)
    for _ in range(12):                          # x1 != 0 (see the module docstring)
        x1, y1, y2 = rng.uniform(-0.5, 0.5, 3).round(4)
        r = _run(exe, "crafted", x1, y1, y2)
        assert r["verdicts_equal"] == 1 and r["plus_equal"] == 1 and (r["tie"] == 1 or r["point_mirrors"] == 1), (x1, y1, y2, r)
