"""Cases of the workgroup retainBest replay (retain_best_emul.h block_pair_swap / block_retain_best_gnu), shared by
tests/test_retain_block_cpu.py and tests/test_gpu_orb_retain_block.py, and the host library both go through
(tests/native/retain_block_host.cpp).

A range of m elements is cut into 64-element chunks and the chunks into one contiguous slice per wave; LENGTHS are the
smallest m at which a slice boundary, an empty slice (fewer chunks than waves) or a partial last chunk occurs for 1, 2
and 4 waves, around the 2048 tier of the two launches, and the longest VGA list (4800)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "retain_block_host.cpp")
BUILD = os.path.join(HERE, "native", "build")

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4800]
NWAVES = (1, 2, 4)
FAST, HARRIS = 0, 1                      # element kinds: u32 compared on >> 24, u64 compared on the f32 in the high word
LIBSTDCXX, MSVC = 0, 1


def build_lib():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libretain_block_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-o", out, SRC])
    lib = C.CDLL(out)
    lib.rbk_check.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.rbk_retain.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def build_sanitized_program():
    """the same source with its main, as a stand-alone program under the address and undefined-behaviour sanitizers"""
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "retain_block_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-DRBK_MAIN", "-o", out, SRC])
    return out


def contents(m, kind):
    """(name, m + 1 responses): index 0 is the slot in front of the range (the pivot of a partition round, the boundary
    element of std::partition), indices 1 .. m the range.  Drawn afresh but reproducibly per (m, kind)."""
    rng = np.random.default_rng(1000 * m + kind)
    n = m + 1
    k_first = max(1, min(m // 8, 64))                       # inside the first chunk, so inside every first slice
    k_last = max(1, min(m // 8, (m - 1) % 64 + 1))          # inside the last chunk, so inside the last non-empty slice
    out = [("equal", np.full(n, 20.0)),                      # every element stops both scans: K = floor(m / 2)
           ("descending", np.arange(n, 0, -1.0)),            # K = 0 for std::partition
           ("ascending", np.arange(1.0, n + 1)),
           ("two-valued", rng.integers(15, 17, n).astype(np.float64)),
           ("eight-valued", rng.integers(15, 23, n).astype(np.float64))]
    for name, base, other, where in (("left stoppers in the first slice", 2.0, 0.0, slice(1, 1 + k_first)),
                                     ("left stoppers in the last slice", 2.0, 0.0, slice(n - k_last, n)),
                                     ("right stoppers in the first slice", 0.0, 2.0, slice(1, 1 + k_first)),
                                     ("right stoppers in the last slice", 0.0, 2.0, slice(n - k_last, n))):
        r = np.full(n, base)
        r[where] = other
        r[0] = 1.0                                           # between the two: e >= r[0] holds for the 2.0 only
        out.append((name, r))
    if kind == HARRIS:
        out.append(("negative", -rng.random(n) - 0.5))
        out.append(("negative, tied", -rng.integers(1, 4, n).astype(np.float64)))
        out.append(("signed zeros", rng.choice(np.array([-0.0, 0.0, -1.0, 1.0]), n)))
    return out


def elements(resp, kind):
    """responses -> elements with the position as the payload (so that an element identifies itself).  FAST scores are
    8 bits: the responses keep their order and their ties, and where more than 255 values are distinct, neighbouring
    ranks share a score."""
    resp = np.asarray(resp, np.float64)
    ids = np.arange(len(resp), dtype=np.uint64)
    if kind == HARRIS:
        return (resp.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids
    vals, rank = np.unique(resp, return_inverse=True)
    score = rank + 1 if len(vals) <= 255 else rank * 254 // (len(vals) - 1) + 1
    return ((score.astype(np.uint64) << np.uint64(24)) | ids).astype(np.uint32)


def n_points_of(n):
    return sorted({1, n // 2, n - 1} - {0}) if n > 1 else [1]


def retain_host(lib, elems, n_points, runtime, kind):
    """the sequential rb::retain_best on a copy: (list as left behind, new size)"""
    a = np.ascontiguousarray(elems).copy()
    n1 = lib.rbk_retain(kind, a.ctypes.data_as(C.c_void_p), len(a), int(n_points), runtime)
    return a, n1


def retain_lists():
    """the lists of the GPU test: (kind, runtime) -> [(elements, n_points, label)], every length, content and n_points"""
    out = {}
    for kind in (FAST, HARRIS):
        lists = []
        for m in LENGTHS:
            for name, resp in contents(m, kind):
                e = elements(resp[1:], kind)
                for npts in n_points_of(m):
                    lists.append((e, npts, (m, name, npts)))
        for runtime in (LIBSTDCXX, MSVC):
            out[kind, runtime] = lists
    return out
