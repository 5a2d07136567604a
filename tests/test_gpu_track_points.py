"""Track points on the GPU (rpe_triangulate_tracks, through the C-ABI) against the scalar float64 model
(tests/track_point_model.py): integers exactly and every floating output bit for bit -- the rule has no reduction tree and
no libm call but sqrt, and the build has no contraction.  The hand-built scenes of tests/track_point_cases.py, the
workgroup-tail shapes, the two camera forms and the two group forms, every refusal, and the run form over a stream."""
import ctypes as C

import numpy as np
import pytest

from tests import camera_model as cm
from tests import scale_model as sc
from tests import track_point_cases as tc
from tests import track_point_model as tm

pytestmark = pytest.mark.gpu

INVALID = -1


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def eng(capi):
    """a small handle: its images are never touched"""
    e = capi.Engine(640, 480, max_batch=1, nfeatures=64, max_matches=32)
    yield e
    e.close()


def _records(capi, cams):
    rec = np.zeros(len(cams), capi.CAMERA_DTYPE)
    for i, c in enumerate(cams):
        rec[i] = (c.fx, c.fy, c.cx, c.cy, c.dist)
    return rec


def _call(capi, e, case, as_cams=False, **kw):
    """the library's dict of a case; as_cams: a one-K case through per-frame records of that pinhole"""
    cams = case['cams']
    F = len(case['R_abs'])
    if isinstance(cams, cm.Cam) and not as_cams:
        cam = dict(K=cams.K)
    else:
        cam = dict(cameras=_records(capi, [cams] * F if isinstance(cams, cm.Cam) else cams))
    args = dict(frame_group=case['frame_group'], **case['gates'])
    args.update(kw)
    return e.triangulate_tracks(case['tracks'], case['R_abs'], case['T_abs'], **cam, **args)


@pytest.fixture(scope="module")
def models():
    return {c['name']: (c, tm.model_case(c)) for c in tc.cases()}


@pytest.mark.parametrize("name", [c['name'] for c in tc.cases()])
def test_hand_built_cases(capi, eng, models, name):
    case, want = models[name]
    got = _call(capi, eng, case)
    print(name, "codes", np.bincount(want['code'], minlength=6).tolist(), "iterations up to", int(want['iterations'].max()))
    tm.assert_equal(got, want, name)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_workgroup_tails(capi, eng, n):
    case = tc.two_view_tracks(n)
    want = tm.model_case(case)
    assert (want['code'] == tm.OK).all()
    tm.assert_equal(_call(capi, eng, case), want, n)


def test_group_null_equals_all_zero_and_K_equals_pinhole_records(capi, eng, models):
    case, want = models["noisy_5"]
    tm.assert_equal(_call(capi, eng, case, frame_group=np.zeros(8, np.int32)), want, "zero groups")
    tm.assert_equal(_call(capi, eng, case, as_cams=True), want, "pinhole records")
    case, want = models["outlier"]
    tm.assert_equal(_call(capi, eng, case, as_cams=True, frame_group=np.full(8, 7, np.int32)), want, "one group of another name")


def test_same_call_twice_and_after_a_larger_and_a_smaller_call(capi, eng, models):
    case, want = models["clean_lens"]
    a = _call(capi, eng, case)
    b = _call(capi, eng, case)
    tm.assert_equal(a, b)
    tm.assert_equal(_call(capi, eng, tc.two_view_tracks(300)), tm.model_case(tc.two_view_tracks(300)))      # the buffers grow
    tm.assert_equal(_call(capi, eng, models["behind"][0]), models["behind"][1])
    tm.assert_equal(_call(capi, eng, case), want)


def test_no_tracks_and_empty_tracks(capi, eng):
    case = tc.clean(False)
    none = {'track_start': np.zeros(1, np.int32), 'obs_frame': np.zeros(0, np.int32), 'obs_xy': np.zeros((0, 2), np.float32)}
    got = eng.triangulate_tracks(none, case['R_abs'], case['T_abs'], K=tc.K0)
    assert got['points'].shape == (0, 3) and got['obs_flag'].shape == (0,)
    empty = dict(none, track_start=np.zeros(4, np.int32))                     # three tracks without an observation
    got = eng.triangulate_tracks(empty, case['R_abs'], case['T_abs'], K=tc.K0)
    assert (got['code'] == tm.TOO_FEW).all() and not got['n_used'].any() and not got['points'].any()


def _raw(e, case, **kw):
    """rpe_triangulate_tracks itself (the wrapper checks some arguments before the library sees them): the return code"""
    tr = case['tracks']
    a = dict(n_tracks=len(tr['track_start']) - 1, track_start=tr['track_start'], obs_frame=tr['obs_frame'], obs_xy=tr['obs_xy'],
             n_frames=len(case['R_abs']), R=case['R_abs'], T=case['T_abs'], group=None, K=tc.K0, cams=None, **case['gates'])
    a.update(kw)
    keep = []

    def ptr(x, dt):
        if x is None:
            return None
        keep.append(np.ascontiguousarray(x, dt))
        return keep[-1].ctypes.data_as(C.c_void_p)
    n, no = max(a['n_tracks'], 1), max(len(tr['obs_frame']), 1)
    outs = [np.zeros(3 * n), np.zeros(4 * n, np.int32), np.zeros(n), np.zeros(n), np.zeros(no, np.uint8), np.zeros(no)]
    cams = a['cams']
    return e.lib.rpe_triangulate_tracks(e.h, a['n_tracks'], ptr(a['track_start'], np.int32), ptr(a['obs_frame'], np.int32),
                                        ptr(a['obs_xy'], np.float32), a['n_frames'], ptr(a['R'], np.float64), ptr(a['T'], np.float64),
                                        ptr(a['group'], np.int32), ptr(a['K'], np.float64), None if cams is None else ptr(cams, cams.dtype),
                                        float(a['threshold_px']), int(a['min_views']), float(a['max_cos']), int(a['max_iters']),
                                        *[o.ctypes.data_as(C.c_void_p) for o in outs])


def test_refusals_leave_the_handle_usable(capi, eng, models):
    case, want = models["noisy_3"]
    good = _call(capi, eng, case)
    tm.assert_equal(good, want)
    assert _raw(eng, case) == 0
    F = len(case['R_abs'])
    pin = _records(capi, [case['cams']] * F)

    def bad(**kw):
        assert _raw(eng, case, **kw) == INVALID, kw
        assert b"rpe_triangulate_tracks" in eng.lib.rpe_last_error(eng.h), kw
    ts = case['tracks']['track_start']
    bad(n_tracks=-1)
    s = ts.copy(); s[0] = 1
    bad(track_start=s)
    s = ts.copy(); s[3] = s[2] - 1
    bad(track_start=s)
    bad(n_frames=0)
    f = case['tracks']['obs_frame'].copy(); f[5] = F
    bad(obs_frame=f)
    f = case['tracks']['obs_frame'].copy(); f[0] = -1
    bad(obs_frame=f)
    bad(cams=pin)                                        # both K and cams
    bad(K=None)                                          # neither
    c = pin.copy(); c['fx'][2] = 0.0
    bad(K=None, cams=c)
    c = pin.copy(); c['dist'][1, 3] = np.nan
    bad(K=None, cams=c)
    k = tc.K0.copy(); k[1, 1] = -1.0
    bad(K=k)
    for v in (0.0, -1.0, np.nan, np.inf):
        bad(threshold_px=v)
    bad(min_views=1)
    for v in (-1.0, 1.0000001, np.nan):
        bad(max_cos=v)
    bad(max_iters=-1)
    bad(max_iters=101)
    R = case['R_abs'].copy(); R[4, 1, 1] = np.inf
    bad(R=R)
    T = case['T_abs'].copy(); T[7, 2] = np.nan
    bad(T=T)
    g = np.zeros(F, np.int32); g[7] = -1
    bad(T=T, group=np.zeros(F, np.int32))
    assert _raw(eng, case, T=T, group=g) == 0            # a frame without a group may hold anything
    assert _raw(eng, case, K=None, cams=pin) == 0
    assert _raw(eng, case, n_tracks=0) == 0
    assert _raw(eng, case, n_tracks=0, threshold_px=0.0) == INVALID
    tm.assert_equal(_call(capi, eng, case), good)         # the next valid call returns the earlier bytes


# ------------------------------------------------------------------ run form
def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrs]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def physics():
    return sc.physics_frames()


@pytest.mark.parametrize("flags", [dict(), dict(register=True), dict(bundle=True)])
def test_estimate_trajectory_points_equal_the_model(capi, physics, flags):
    """the PHYSICS stream, ORB-1000 / 500: estimate_trajectory(points=True) equals the model fed with the returned tracks,
    chain and groups; without the flag every other key keeps its bits"""
    from relative_pose_estimation_amd import PoseEstimator, geometry
    frames, K = physics
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    plain = pe.estimate_trajectory(frames, tracks=True, **flags)
    d = pe.estimate_trajectory(frames, points=True, **flags)
    assert set(d) == set(plain) | {'points'}
    for k in plain:
        if k != 'tracks':
            assert _same_bits(d[k], plain[k]), k
    for k in ('track_start', 'obs_frame', 'obs_kp', 'obs_xy', 'match_track'):
        assert _same_bits(d['tracks'][k], plain['tracks'][k]), k
    pts = d['points']
    assert pts['chain'] == ('R_abs_ba' if flags.get('bundle') else 'R_abs_reg' if flags.get('register') else 'R_abs')
    if not flags:
        assert _same_bits(pts['T_abs'], d['T_abs']) and pts['frame_group'].tolist() == geometry.frame_groups(d['status'], d['segment']).tolist()
    want = tm.triangulate_tracks(d['tracks'], d[pts['chain']], pts['T_abs'], cm.Cam(K), pts['frame_group'])
    tm.assert_equal(pts, want, flags)
    ok = pts['code'] == capi.TRACKPT_OK
    hist = dict(zip(capi.TRACKPT_NAMES, np.bincount(pts['code'], minlength=6).tolist()))
    print("run form", flags, "tracks", len(ok), hist, "lengths", np.bincount(np.diff(d['tracks']['track_start'])).tolist(),
          "median rms of OK %.4f px" % float(np.median(pts['rms'][ok])), "inlier share %.4f" % float((pts['obs_flag'] == 1).mean()))
    assert 2 * int(ok.sum()) >= len(ok)
    assert (pts['rms'][ok] <= 2.0).all()
    # last_track_points over the same chain: the same bits, and its gates reach the library
    again = pe.last_track_points(d[pts['chain']], pts['T_abs'], pts['frame_group'])
    tm.assert_equal(again, pts)
    strict = pe.last_track_points(d[pts['chain']], pts['T_abs'], pts['frame_group'], min_views=3)
    assert (strict['code'][np.diff(d['tracks']['track_start']) == 2] == capi.TRACKPT_TOO_FEW).all()
    pe.close()


def test_the_run_stays_fetchable(capi, physics, models):
    frames, K = physics
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(frames[:4], K)
    assert not res[4].any()

    def fetches():
        return _bits(e.fetch_results(3)) + _bits(e.fetch_structure(3)) + _bits(e.fetch_match_indices(3)) + _bits(e.fetch_matched_points(3))
    before = fetches()
    tracks = e.build_tracks()
    case, want = models["outlier"]
    tm.assert_equal(_call(capi, e, case), want)
    R = np.stack([np.eye(3)] * 4); T = np.array([[-0.3 * i, 0.0, 0.0] for i in range(4)])
    first = e.triangulate_tracks(tracks, R, T, K=K)
    again = e.build_tracks()
    for k in ('track_start', 'obs_frame', 'obs_kp', 'obs_xy', 'match_track'):
        assert _same_bits(tracks[k], again[k]), k
    for x, y in zip(before, fetches()):
        assert np.array_equal(x, y)
    tm.assert_equal(e.triangulate_tracks(again, R, T, K=K), first)
    e.close()
