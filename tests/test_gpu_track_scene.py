"""The track scene that rpe_triangulate_tracks and rpe_bundle_windows share (csrc/track_scene.h, scene_upload), on the GPU:
every single fault of the shared arguments is refused by both raw entry points with RPE_ERR_INVALID and the same text
behind the entry point's name; and track points and window bundles over a larger and a smaller scene, alternating on one
handle, return for every repeated call the bits of its first occurrence, which are the bits of that call on a fresh handle
-- the one scene set serves both, grows once and is carved anew by every call.  Existing cases only: the smallest of
tests/track_point_cases.py, noisy_w5 and count_257 (more tracks than a 256-thread workgroup) of tests/window_bundle_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import track_point_cases as tc
from tests import window_bundle_cases as wc

pytestmark = pytest.mark.gpu

INVALID = -1


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


def _engine(capi):
    """a small handle: its images are never touched"""
    return capi.Engine(640, 480, max_batch=1, nfeatures=64, max_matches=32)


def _same_bits(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _equal_results(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert _same_bits(a[k], b[k]), (what, k)


# ------------------------------------------------------------------ 1. the shared refusals
def _raw_both(e, scene):
    """both entry points over one scene (a dict of the shared arguments; None = NULL), each with valid arguments of its own:
    [(return code, the text of rpe_last_error behind '<name>: ')] for the track points, then for the window bundles"""
    keep = []

    def ptr(x, dt):
        if x is None:
            return None
        keep.append(np.ascontiguousarray(x, dt))
        return keep[-1].ctypes.data_as(C.c_void_p)

    def shared():
        cams = scene['cams']
        return dict(n_tracks=scene['n_tracks'], ts=ptr(scene['track_start'], np.int32), of=ptr(scene['obs_frame'], np.int32),
                    xy=ptr(scene['obs_xy'], np.float32), n_frames=scene['n_frames'], R=ptr(scene['R'], np.float64),
                    T=ptr(scene['T'], np.float64), K=ptr(scene['K'], np.float64), cams=None if cams is None else ptr(cams, cams.dtype))
    n, no = 4, 16                                   # room for the outputs of the valid call
    out = lambda count, dt=np.float64: ptr(np.zeros(count, dt), dt)
    s = shared()
    rc_tp = e.lib.rpe_triangulate_tracks(e.h, s['n_tracks'], s['ts'], s['of'], s['xy'], s['n_frames'], s['R'], s['T'], None, s['K'], s['cams'],
                                         2.0, 2, 1.0, 10, out(3 * n), out(4 * n, np.int32), out(n), out(n), out(no, np.uint8), out(no))
    err_tp = e.lib.rpe_last_error(e.h) if rc_tp else b""
    s = shared()
    rc_wb = e.lib.rpe_bundle_windows(e.h, s['n_tracks'], s['ts'], s['of'], s['xy'], ptr(np.ones(3 * n), np.float64), None, None, s['n_frames'],
                                     s['R'], s['T'], s['K'], s['cams'], 1, ptr([0, 2], np.int32), ptr([0, 1], np.int32), 16, 0, 1,
                                     out(18), out(6), out(48), out(16, np.int32), out(4, np.int32), out(4, np.int32), out(2))
    err_wb = e.lib.rpe_last_error(e.h) if rc_wb else b""
    res = []
    for rc, err, name in ((rc_tp, err_tp, b"rpe_triangulate_tracks: "), (rc_wb, err_wb, b"rpe_bundle_windows: ")):
        assert not rc or err.startswith(name), (rc, err)
        res.append((rc, err[len(name):]))
    return res


def test_shared_faults_are_refused_alike(capi):
    case = min(tc.cases(), key=lambda c: len(c['tracks']['obs_frame']))
    tr = case['tracks']
    F = len(case['R_abs'])
    assert len(tr['obs_frame']) == 2 and F == 2                              # one track of two views: the outputs above hold it
    good = dict(n_tracks=len(tr['track_start']) - 1, track_start=tr['track_start'], obs_frame=tr['obs_frame'], obs_xy=tr['obs_xy'],
                n_frames=F, R=case['R_abs'], T=case['T_abs'], K=case['cams'].K, cams=None)
    pin = np.zeros(F, capi.CAMERA_DTYPE)
    for i in range(F):
        pin[i] = (tc.K0[0, 0], tc.K0[1, 1], tc.K0[0, 2], tc.K0[1, 2], np.zeros(8))
    no_fx = pin.copy(); no_fx['fx'][1] = 0.0
    nan_cy = pin.copy(); nan_cy['cy'][0] = np.nan
    bad_K = tc.K0.copy(); bad_K[1, 1] = -1.0
    faults = [(dict(n_tracks=-1), b"n_tracks must be >= 0"), (dict(n_frames=0), b"n_frames must be >= 1"),
              (dict(cams=pin), b"exactly one of K and cams must be given"), (dict(K=None), b"exactly one of K and cams must be given"),
              (dict(track_start=[1, 2]), b"track_start[0] must be 0"), (dict(track_start=[0, -1]), b"track_start must not decrease"),
              (dict(track_start=None), None), (dict(R=None), None), (dict(T=None), None), (dict(obs_frame=None), None),
              (dict(obs_xy=None), None),
              (dict(obs_frame=[0, F]), b"a frame index outside 0 ... n_frames - 1"), (dict(obs_frame=[-1, 1]), b"a frame index outside 0 ... n_frames - 1"),
              (dict(K=None, cams=no_fx), b"a camera has fx <= 0 or fy <= 0"), (dict(K=None, cams=nan_cy), b"a camera has a non-finite field"),
              (dict(K=bad_K), b"a camera has fx <= 0 or fy <= 0")]
    e = _engine(capi)
    try:
        assert [rc for rc, _ in _raw_both(e, good)] == [0, 0]
        assert [rc for rc, _ in _raw_both(e, dict(good, K=None, cams=pin))] == [0, 0]
        for kw, text in faults:
            (rc_tp, err_tp), (rc_wb, err_wb) = _raw_both(e, dict(good, **kw))
            assert rc_tp == INVALID and rc_wb == INVALID, (kw, rc_tp, rc_wb)
            assert err_tp == err_wb and err_tp, (kw, err_tp, err_wb)
            assert text is None or err_tp == text, (kw, err_tp)
        null_texts = {_raw_both(e, dict(good, **kw))[0][1] for kw, text in faults if text is None}
        assert len(null_texts) == 1, null_texts                              # the one text that names no argument
        assert [rc for rc, _ in _raw_both(e, good)] == [0, 0]                # the handle stays usable
    finally:
        e.close()


# ------------------------------------------------------------------ 2. one scene set under alternating calls
def _points(e, case):
    """the track points of a window case: its poses are the perturbed ones, so under the gate its start points were made with"""
    return e.triangulate_tracks(case['tracks'], case['R_abs'], case['T_abs'], K=case['cams'].K,
                                **dict(tc.DEFAULT_GATES, threshold_px=wc.START_GATE_PX))


def _windows(e, case):
    return e.bundle_windows(case['tracks'], case['points0'], case['R_abs'], case['T_abs'], case['windows'], K=case['cams'].K,
                            obs_use=case['obs_use'], point_use=case['point_use'], max_points=case['max_points'], min_obs=case['min_obs'],
                            max_iters=case['max_iters'])


def test_alternating_calls_share_the_scene_set(capi):
    small, large = wc.noisy(5), wc.counted(257)
    assert (small['name'], large['name']) == ("noisy_w5", "count_257")
    assert len(large['tracks']['obs_frame']) > len(small['tracks']['obs_frame']) and len(large['tracks']['track_start']) - 1 > 256
    sequence = [("points, larger", _points, large), ("windows, smaller", _windows, small), ("points, larger", _points, large),
                ("windows, larger", _windows, large), ("windows, smaller", _windows, small)]
    fresh = {}
    for what, call, case in sequence:
        if what not in fresh:
            e = _engine(capi)
            try:
                fresh[what] = call(e, case)
            finally:
                e.close()
    # the calls did solve something (what they solve is the business of test_gpu_track_points / test_gpu_window_bundle)
    assert (fresh["points, larger"]['code'] == capi.TRACKPT_OK).sum() * 2 > 257
    assert fresh["windows, larger"]['code'].tolist() == [capi.WINDOW_OK] and fresh["windows, smaller"]['code'].tolist() == [capi.WINDOW_OK]
    e = _engine(capi)
    try:
        first = {}
        for step, (what, call, case) in enumerate(sequence):
            got = call(e, case)
            _equal_results(got, first.setdefault(what, got), (step, what, "its first occurrence"))
            _equal_results(got, fresh[what], (step, what, "a fresh handle"))
    finally:
        e.close()
