"""The workgroup retainBest replay on the GPU, through the stage entry rpe_orb_debug_retain (the device routine of
retain_fast_kernel and retain_harris_kernel, one workgroup per list, all lists of a kind and runtime in one launch)
against the sequential rb::retain_best on the host (tests/native/retain_block_host.cpp): every list must come back in
the same order element for element, with the same new size.  Lengths, contents and n_points are the CPU test's
(tests/retain_block_cases.py), for the u32 FAST entries and the u64 Harris entries, for libstdc++ and MSVC."""
import numpy as np
import pytest

from tests import retain_block_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return rc.build_lib()


@pytest.fixture(scope="module")
def engine():
    from relative_pose_estimation_amd import _capi
    e = _capi.Engine(640, 480, max_batch=1, nfeatures=1000, max_matches=500)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lists():
    return rc.retain_lists()


@pytest.mark.parametrize("kind", [rc.FAST, rc.HARRIS])
@pytest.mark.parametrize("runtime", [rc.LIBSTDCXX, rc.MSVC])
def test_every_list_is_left_as_the_sequential_procedure_leaves_it(engine, lib, lists, kind, runtime):
    todo = lists[kind, runtime]
    assert len(todo) >= 21 * 9 * 2
    got, got_n = engine.orb_debug_retain(kind, runtime, [e for e, _, _ in todo], [npts for _, npts, _ in todo])
    assert len(got) == len(todo)
    for (e, npts, label), a, n1 in zip(todo, got, got_n):
        want, want_n = rc.retain_host(lib, e, npts, runtime, kind)
        assert n1 == want_n, (label, n1, want_n)
        assert np.array_equal(a, want), label


def test_workgroups_keep_their_lds_to_themselves(engine, lib):
    """64 copies of one 2049-element list in one launch: every workgroup must leave the same list"""
    resp = dict(rc.contents(2049, rc.FAST))["eight-valued"][1:]
    e = rc.elements(resp, rc.FAST)
    want, want_n = rc.retain_host(lib, e, 500, rc.LIBSTDCXX, rc.FAST)
    got, got_n = engine.orb_debug_retain(rc.FAST, rc.LIBSTDCXX, [e] * 64, [500] * 64)
    for a, n1 in zip(got, got_n):
        assert n1 == want_n and np.array_equal(a, want)


def test_lists_beyond_the_capacity_are_refused(engine):
    from relative_pose_estimation_amd import _capi
    e = rc.elements(np.arange(100.0), rc.FAST)
    with pytest.raises(_capi.RpeError, match="longer than the capacity"):
        engine.orb_debug_retain(rc.FAST, rc.LIBSTDCXX, [e, e[:10]], [5, 5], cap=64)
    with pytest.raises(_capi.RpeError, match="cap too large"):
        engine.orb_debug_retain(rc.HARRIS, rc.LIBSTDCXX, [rc.elements(np.arange(10.0), rc.HARRIS)], [5], cap=8000)
