"""The premises of tests/test_gpu_sift_ties.py, checked on the CPU oracle: what the tie images of tests/sift_tie_cases.py
hold, and what retainBest keeps of them at each cap."""
import numpy as np
import pytest

import sift_tie_cases as tie


@pytest.fixture(scope="module")
def uncapped(oracle):
    return {amps: oracle.sift_detect_and_compute(tie.blob_grid(amps), 0, return_flags=True)
            for amps in (tie.TWO_AMPLITUDES, tie.ONE_AMPLITUDE)}


def test_two_amplitude_grid_has_two_responses(uncapped):
    k, _, flags = uncapped[tie.TWO_AMPLITUDES]
    resp, cnt = np.unique(k["response"], return_counts=True)
    assert len(k) == 80 and flags == 0
    assert len(resp) == 2 and cnt[1] == 48 and cnt[0] == 32           # ascending: the weak ones first


def test_single_amplitude_grid_has_one_response(uncapped):
    k, _, flags = uncapped[tie.ONE_AMPLITUDE]
    assert len(k) == 80 and flags == 0 and len(np.unique(k["response"])) == 1


@pytest.mark.parametrize("amps,nfeatures", list(tie.EXPECTED))
def test_capped_counts_and_flags(oracle, uncapped, amps, nfeatures):
    """ties of the nfeatures-th response are kept; over the capacity nfeatures + 64 the list is cut in sorted order"""
    count, flags = tie.EXPECTED[(amps, nfeatures)]
    k, d, f = oracle.sift_detect_and_compute(tie.blob_grid(amps), nfeatures, cap=nfeatures + 64, return_flags=True)
    assert len(k) == count and f == flags, (len(k), f)
    assert count <= nfeatures + 64
    ku, du, _ = uncapped[amps]
    if amps == tie.TWO_AMPLITUDES and count == 48:
        keep = ku["response"] == ku["response"].max()
        assert np.array_equal(k, ku[keep]) and np.array_equal(d, du[keep])
    else:
        assert np.array_equal(k, ku[:count]) and np.array_equal(d, du[:count])


def test_prefilter_frame_exceeds_the_prefilter_bound(oracle):
    f = tie.PREFILTER_FRAME
    k, _ = oracle.sift_detect_and_compute(tie.prefilter_frame(), 0)
    assert len(k) == f["uncapped"] > 2 * f["nfeatures"] + 1024
