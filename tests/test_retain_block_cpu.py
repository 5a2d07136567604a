"""The workgroup form of the retainBest replay (retain_best_emul.h) on the host.  rb::block_pair_swap_model performs the
device routine's arithmetic per wave slice -- slice totals, offsets, ranks from the original contents, per-slice K --
lane by lane; it must leave the array and the return value of the sequential scans it replaces (libstdc++'s
__unguarded_partition after __move_median_to_first, and std::partition), for 1, 2 and 4 waves.  The whole procedure
(rb::retain_best_gnu_by_passes, the body the device runs, over the model) must leave the ids in the order of the REAL
std::nth_element + std::partition.  The same checks run once more in a stand-alone program built with the address and
undefined-behaviour sanitizers.  Lengths and contents: tests/retain_block_cases.py."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

from tests import retain_block_cases as rc


@pytest.fixture(scope="module")
def lib():
    return rc.build_lib()


def _records():
    """(kind, elements, [(op, a1, a2, nwaves, want)]): every check of this file, also the case file of the sanitizer run"""
    recs = []
    for kind in (rc.FAST, rc.HARRIS):
        for m in rc.LENGTHS:
            for name, resp in rc.contents(m, kind):
                # pass level: the range is [1, m + 1), the element in front of it is the pivot / the boundary element
                ops = []
                for nw in rc.NWAVES:
                    if m >= 3:                                  # __unguarded_partition has its sentinels from four elements on
                        ops.append((0, 0, 0, nw, 1))
                    ops.append((1, 1, 0, nw, 1))
                recs.append((kind, rc.elements(resp, kind), ops, (m, name)))
                # whole procedure on the m elements
                ops = []
                for nw in rc.NWAVES:
                    for npts in rc.n_points_of(m):
                        ops.append((2, npts, -1, nw, 1))
                        if m >= 4 and name in ("equal", "ascending", "eight-valued", "signed zeros"):
                            ops.append((2, npts, 0, nw, 1))    # depth limit 0: the heap fallback from the first round
                for npts in rc.n_points_of(m):
                    ops.append((3, npts, rc.MSVC, 0, 1))
                recs.append((kind, rc.elements(resp[1:], kind), ops, (m, name)))
    return recs


def test_block_model_equals_the_sequential_passes_and_the_real_library(lib):
    n_pass = n_whole = n_heap = 0
    for kind, e, ops, label in _records():
        for op, a1, a2, nw, want in ops:
            if op == 3:
                continue
            got = lib.rbk_check(kind, e.ctypes.data_as(C.c_void_p), len(e), op, a1, a2, nw)
            assert got == want, (kind, label, op, a1, a2, nw)
            n_pass += op < 2
            n_whole += op == 2 and a2 < 0
            n_heap += op == 2 and a2 == 0
    assert n_pass > 1200 and n_whole > 1500 and n_heap > 300, (n_pass, n_whole, n_heap)


def test_msvc_runtime_keeps_cv2s_set(lib):
    """the MSVC branch stays the sequential procedure on one lane; whatever the runtime, retainBest keeps the n best and
    every element tied with the n-th"""
    for kind in (rc.FAST, rc.HARRIS):
        for m in rc.LENGTHS:
            for name, resp in rc.contents(m, kind):
                e = rc.elements(resp[1:], kind)
                key = (e >> np.uint32(24)).astype(np.float64) if kind == rc.FAST else (e >> np.uint64(32)).astype(np.uint32).view(np.float32)
                for npts in rc.n_points_of(m):
                    a, n1 = rc.retain_host(lib, e, npts, rc.MSVC, kind)
                    if m > npts:
                        thr = np.sort(key)[::-1][npts - 1]
                        assert sorted(a[:n1].tolist()) == sorted(e[key >= thr].tolist()), (kind, m, name, npts)
                    else:
                        assert n1 == m and np.array_equal(a, e)


def test_same_cases_under_the_sanitizers(tmp_path):
    prog = rc.build_sanitized_program()
    path = tmp_path / "cases.bin"
    n = 0
    with open(path, "wb") as f:
        for kind, e, ops, _ in _records():
            f.write(struct.pack("<3i", kind, len(e), len(ops)))
            f.write(np.asarray(ops, np.int32).tobytes())
            f.write(np.ascontiguousarray(e).tobytes())
            n += len(ops)
    r = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{n} cases, 0 bad", r.stdout
