"""Window bundles on the GPU (rpe_bundle_windows, through the C-ABI) against the float64 model
(tests/window_bundle_model.py): codes, counts, point lists and the anchor exactly, poses, points and rms within the model's
own reduction-order margin -- over the hand-built scenes of tests/window_bundle_cases.py (windows of 2 to 8 frames, the
lane-stride and wave-total edges, the cap, masks, lens cameras, every code), the two camera forms, every refusal, the empty
call, determinism, the run it must not touch, and the run form over the PHYSICS stream."""
import ctypes as C

import numpy as np
import pytest

from tests import camera_model as cm
from tests import scale_model as sc
from tests import window_bundle_cases as wc
from tests import window_bundle_model as wm

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -3


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


@pytest.fixture(scope="module")
def models():
    """every case with the model's results, forward and reversed, computed once"""
    return {c['name']: (c, wm.model_case(c), wm.model_case(c, "reversed")) for c in wc.cases()}


@pytest.fixture(scope="module")
def margin(models):
    """ten times the largest forward / reversed difference of the model over the cases: (rms_after px, R degrees, T, point
    coordinate, rms_before px).  Recomputed here, never hard-coded."""
    fwd = [r for _, f, _ in models.values() for r in f]; rev = [r for _, _, v in models.values() for r in v]
    ties, d = wm.reduction_margin(fwd, rev)
    print("forward / reversed over %d windows: %s, ties %s" % (len(fwd), d, ties))
    assert (d > 0).all() and len(ties) * 4 <= len(fwd), (d, ties)
    print("window margin (10 x forward / reversed): rms %.3e px, R %.3e deg, T %.3e, point %.3e, rms_before %.3e px" % tuple(10 * d))
    return 10 * d


def _records(capi, cams):
    rec = np.zeros(len(cams), capi.CAMERA_DTYPE)
    for i, c in enumerate(cams):
        rec[i] = (c.fx, c.fy, c.cx, c.cy, c.dist)
    return rec


def _call(capi, e, case, as_cams=False, **kw):
    cams = case['cams']
    F = len(case['R_abs'])
    if isinstance(cams, cm.Cam) and not as_cams:
        cam = dict(K=cams.K)
    else:
        cam = dict(cameras=_records(capi, [cams] * F if isinstance(cams, cm.Cam) else cams))
    args = dict(obs_use=case['obs_use'], point_use=case['point_use'], max_points=case['max_points'], min_obs=case['min_obs'],
                max_iters=case['max_iters'])
    args.update(kw)
    return e.bundle_windows(case['tracks'], case['points0'], case['R_abs'], case['T_abs'], case['windows'], **cam, **args)


def _same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _equal_results(a, b):
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all(_same_bits(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert _same_bits(a[k], b[k]), k


def _window(got, w):
    return dict(R=got['R'][w], T=got['T'][w], points=got['points'][w], rms=tuple(got['rms'][w]))


def _compare(got, w, f, r, margin, worst):
    """window w of a call against the forward model f (r: the reversed one); True when the window is tied"""
    if wm.tied(f, r):
        return True
    info = (int(got['code'][w]), int(got['iterations'][w]), int(got['accepted'][w]), int(got['anchor'][w]))
    counts = (int(got['views'][w]), int(got['n_points'][w]), int(got['n_obs'][w]), int(got['dropped'][w]))
    assert info == tuple(f['info']), (w, info, f['info'])
    assert counts == tuple(f['counts']), (w, counts, f['counts'])
    assert np.array_equal(got['point_track'][w], f['point_track']), w
    g = _window(got, w)
    if f['code'] != wm.WINDOW_OK:                                        # the input state, bit for bit
        assert _same_bits(g['R'], f['R']) and _same_bits(g['T'], f['T']) and _same_bits(g['points'], f['points']), w
        assert _same_bits(got['rms'][w, 0], got['rms'][w, 1])
        if f['code'] != wm.WINDOW_REJECTED:
            assert not got['rms'][w].any()
        elif np.isfinite(f['rms'][0]):
            assert abs(g['rms'][0] - f['rms'][0]) <= margin[4]
        else:
            assert not np.isfinite(g['rms'][0])
        return False
    worst[:] = np.maximum(worst, wm.differences(g, f))
    assert g['rms'][1] <= g['rms'][0]
    assert _same_bits(g['R'][0], f['R'][0]) and _same_bits(g['T'][0], f['T'][0])     # the gauge frame's input bits
    return False


# ------------------------------------------------------------------ 1. every case against the model
def test_cases_equal_the_model(capi, eng, models, margin):
    worst, ties, n, codes = np.zeros(5), [], 0, set()
    for name, (case, fw, rv) in models.items():
        got = _call(capi, eng, case)
        codes |= set(got['code'].tolist())
        w1 = np.zeros(5)
        for w in range(len(fw)):
            n += 1
            if _compare(got, w, fw[w], rv[w], margin, w1):
                ties.append((name, w))
        print("%-16s codes %s points %s iterations %s accepted %s: d_rms %.3e d_R %.3e d_T %.3e d_X %.3e d_rms0 %.3e" %
              (name, got['code'].tolist(), got['n_points'].tolist(), got['iterations'].tolist(), got['accepted'].tolist(), *w1))
        worst = np.maximum(worst, w1)
    print("windows %d ties %s worst %s margin %s" % (n, ties, worst, margin))
    assert len(ties) * 4 <= n, ties
    assert (worst <= margin).all(), (worst, margin)
    assert codes == {capi.WINDOW_OK, capi.WINDOW_NO_BASELINE, capi.WINDOW_TOO_FEW, capi.WINDOW_REJECTED}    # every code came back


# ------------------------------------------------------------------ 2. the camera forms
def test_K_and_pinhole_records_give_the_same_bits(capi, eng, models):
    for name in ("noisy_w5", "overlapping", "capped"):
        case = models[name][0]
        _equal_results(_call(capi, eng, case), _call(capi, eng, case, as_cams=True))


# ------------------------------------------------------------------ 3. refusals, the empty call
def _raw(e, case, outs=True, **kw):
    """rpe_bundle_windows itself (the wrapper checks some arguments before the library sees them): the return code"""
    tr = case['tracks']
    ws = np.concatenate([[0], np.cumsum([len(w) for w in case['windows']])]).astype(np.int32)
    a = dict(n_tracks=len(tr['track_start']) - 1, track_start=tr['track_start'], obs_frame=tr['obs_frame'], obs_xy=tr['obs_xy'],
             points0=case['points0'], point_use=case['point_use'], obs_use=case['obs_use'], n_frames=len(case['R_abs']),
             R=case['R_abs'], T=case['T_abs'], K=wc.tc.K0, cams=None, n_win=len(case['windows']), win_start=ws,
             win_frame=np.concatenate(case['windows']).astype(np.int32), max_points=case['max_points'], min_obs=case['min_obs'],
             max_iters=case['max_iters'])
    a.update(kw)
    keep = []

    def ptr(x, dt):
        if x is None:
            return None
        keep.append(np.ascontiguousarray(x, dt))
        return keep[-1].ctypes.data_as(C.c_void_p)
    nw, nwf = max(a['n_win'], 1), max(0 if a['win_frame'] is None else len(a['win_frame']), 1)
    slots = nw * min(max(a['max_points'], 1), 16384)
    o = [np.full(9 * nwf, 7.0), np.full(3 * nwf, 7.0), np.full(3 * slots, 7.0), np.full(slots, 7, np.int32), np.full(4 * nw, 7, np.int32),
         np.full(4 * nw, 7, np.int32), np.full(2 * nw, 7.0)]
    cams = a['cams']
    rc = e.lib.rpe_bundle_windows(e.h, a['n_tracks'], ptr(a['track_start'], np.int32), ptr(a['obs_frame'], np.int32),
                                  ptr(a['obs_xy'], np.float32), ptr(a['points0'], np.float64), ptr(a['point_use'], np.uint8),
                                  ptr(a['obs_use'], np.uint8), a['n_frames'], ptr(a['R'], np.float64), ptr(a['T'], np.float64),
                                  ptr(a['K'], np.float64), None if cams is None else ptr(cams, cams.dtype), a['n_win'],
                                  ptr(a['win_start'], np.int32), ptr(a['win_frame'], np.int32), int(a['max_points']), int(a['min_obs']),
                                  int(a['max_iters']), *[(x.ctypes.data_as(C.c_void_p) if outs else None) for x in o])
    return rc, o


def test_refusals_leave_the_handle_usable(capi, eng, models):
    case = models["noisy_w5"][0]
    good = _call(capi, eng, case)
    assert _raw(eng, case)[0] == 0
    F = len(case['R_abs'])
    pin = _records(capi, [case['cams']] * F)

    def bad(code=INVALID, **kw):
        rc, o = _raw(eng, case, **kw)
        assert rc == code, (kw, rc)
        assert b"rpe_bundle_windows" in eng.lib.rpe_last_error(eng.h), kw
        assert all((x == 7).all() for x in o), kw                            # nothing was written
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
    bad(track_start=None); bad(obs_frame=None); bad(obs_xy=None); bad(points0=None); bad(R=None); bad(T=None)
    bad(cams=pin)                                                            # both K and cams
    bad(K=None)                                                              # neither
    c = pin.copy(); c['fx'][2] = 0.0
    bad(K=None, cams=c)
    k = wc.tc.K0.copy(); k[1, 1] = -1.0
    bad(K=k)
    bad(n_win=-1)
    bad(win_start=None); bad(win_frame=None)
    bad(win_start=np.array([1, 5], np.int32))
    bad(n_win=2, win_start=np.array([0, 3, 2], np.int32))                    # decreasing
    bad(win_start=np.array([0, 1], np.int32))                                # one frame
    bad(win_start=np.array([0, 9], np.int32), win_frame=np.arange(9, dtype=np.int32), n_frames=9,
        R=np.stack([np.eye(3)] * 9), T=np.zeros((9, 3)))                     # nine frames
    bad(win_frame=np.array([0, 1, 2, 3, F], np.int32))
    bad(win_frame=np.array([0, 1, -1, 3, 4], np.int32))
    bad(win_frame=np.array([0, 1, 2, 1, 4], np.int32))                       # repeated
    R = case['R_abs'].copy(); R[4, 1, 1] = np.inf
    bad(R=R)
    T = case['T_abs'].copy(); T[2, 2] = np.nan
    bad(T=T)
    assert _raw(eng, case, T=T, win_start=np.array([0, 2], np.int32), win_frame=np.array([0, 1], np.int32))[0] == 0   # no window names frame 2
    p = case['points0'].copy(); used = int(np.flatnonzero(case['point_use'])[3]); p[used, 1] = np.nan
    bad(points0=p)
    pu = case['point_use'].copy(); pu[used] = 0
    assert _raw(eng, case, points0=p, point_use=pu)[0] == 0                  # a track that is not used may hold anything
    bad(max_points=0)
    bad(code=CAPACITY, max_points=16385)
    bad(min_obs=-1)
    bad(max_iters=0); bad(max_iters=101)
    assert _raw(eng, case, K=None, cams=pin)[0] == 0
    assert _raw(eng, case, outs=False)[0] == 0                               # every output may be NULL
    _equal_results(_call(capi, eng, case), good)                             # the next valid call returns the earlier bytes


def test_no_windows_and_no_tracks(capi, eng, models):
    case = models["noisy_w5"][0]
    rc, o = _raw(eng, case, n_win=0, win_start=None, win_frame=np.zeros(0, np.int32))
    assert rc == 0 and all((x == 7).all() for x in o)
    assert _raw(eng, case, n_win=0, max_iters=0)[0] == INVALID               # the scalar checks come first
    got = eng.bundle_windows(case['tracks'], case['points0'], case['R_abs'], case['T_abs'], [], K=wc.tc.K0)
    assert got['code'].shape == (0,) and got['R'] == []
    none = {'track_start': np.zeros(1, np.int32), 'obs_frame': np.zeros(0, np.int32), 'obs_xy': np.zeros((0, 2), np.float32)}
    got = eng.bundle_windows(none, np.zeros((0, 3)), case['R_abs'], case['T_abs'], [[0, 1, 2]], K=wc.tc.K0)
    assert got['code'].tolist() == [wm.WINDOW_TOO_FEW] and got['n_points'].tolist() == [0]
    assert _same_bits(got['R'][0], case['R_abs'][:3]) and _same_bits(got['T'][0], case['T_abs'][:3])


# ------------------------------------------------------------------ 4. determinism, no side effects
def test_same_call_twice_and_after_a_larger_and_a_smaller_call(capi, eng, models):
    case = models["mixed_views"][0]
    a = _call(capi, eng, case)
    _equal_results(a, _call(capi, eng, case))
    big = _call(capi, eng, models["count_257"][0], max_points=8192)          # the buffers grow
    _equal_results(big, _call(capi, eng, models["count_257"][0]))            # the stride of the slots is not in the result
    _call(capi, eng, models["too_few"][0])
    _equal_results(a, _call(capi, eng, case))


def _bits(arrs):
    return [np.ascontiguousarray(x).view(np.uint8).copy() for x in arrs]


def test_the_run_stays_fetchable(capi, models):
    frames, K = sc.physics_frames()
    e = capi.Engine(640, 480, max_batch=3, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES)
    res = e.estimate_stream(frames[:4], K)
    assert not res[4].any()

    def fetches():
        return _bits(e.fetch_results(3)) + _bits(e.fetch_structure(3)) + _bits(e.fetch_match_indices(3)) + _bits(e.fetch_matched_points(3))
    before = fetches()
    tracks = e.build_tracks()
    R = np.stack([np.eye(3)] * 4); T = np.array([[-0.3 * i, 0.0, 0.0] for i in range(4)])
    pts = e.triangulate_tracks(tracks, R, T, K=K)
    first = e.bundle_windows(tracks, pts['points'], R, T, [[0, 1, 2, 3], [1, 2]], K=K, obs_use=pts['obs_flag'])
    _call(capi, e, models["overlapping"][0])
    again = e.build_tracks()
    for k in ('track_start', 'obs_frame', 'obs_kp', 'obs_xy', 'match_track'):
        assert _same_bits(tracks[k], again[k]), k
    for x, y in zip(before, fetches()):
        assert np.array_equal(x, y)
    pts2 = e.triangulate_tracks(again, R, T, K=K)
    for k in pts:
        assert _same_bits(pts[k], pts2[k]), k
    _equal_results(first, e.bundle_windows(again, pts2['points'], R, T, [[0, 1, 2, 3], [1, 2]], K=K, obs_use=pts2['obs_flag']))
    e.close()


# ------------------------------------------------------------------ 5. the run form
def test_estimate_trajectory_window_equals_the_model(capi, margin):
    """the PHYSICS stream, ORB-1000 / 500: estimate_trajectory(window=4) equals the model fed with the run's own tracks,
    points and chain, within the one margin of the fixture (whose stream_like case has this run's geometry); without the flag the result has the keys and bits it had; against the stream's true poses the fused
    chain is no worse than the input chain plus the band of the CPU model (printed: the values of DESIGN section 8)"""
    from relative_pose_estimation_amd import PoseEstimator, synthetic
    frames, K = sc.physics_frames()
    pe = PoseEstimator(K, nfeatures=sc.PHYSICS_NFEATURES, max_matches=sc.PHYSICS_MAX_MATCHES, max_batch=5)
    plain = pe.estimate_trajectory(frames, points=True)
    d = pe.estimate_trajectory(frames, window=4)
    assert set(d) == set(plain) | {'window', 'R_abs_win', 'T_abs_win', 'centers_win'}
    for k in plain:
        if k in ('tracks', 'points'):
            for kk in plain[k]:
                assert isinstance(plain[k][kk], str) and plain[k][kk] == d[k][kk] or _same_bits(d[k][kk], plain[k][kk]), (k, kk)
        else:
            assert _same_bits(d[k], plain[k]), k
    win, pts = d['window'], d['points']
    use = (pts['code'] == capi.TRACKPT_OK).astype(np.uint8)
    args = (d['tracks'], pts['points'], d[pts['chain']], pts['T_abs'], win['windows'], cm.Cam(K), pts['obs_flag'], use, 4096, 8, 10)
    fw = wm.bundle_windows(*args); rv = wm.bundle_windows(*args, order="reversed")
    worst, ties = np.zeros(5), []
    for w in range(len(fw)):
        if _compare(win, w, fw[w], rv[w], margin, worst):
            ties.append(w)
    print("run form: windows %s codes %s points %s iterations %s rms %s ties %s worst %s" %
          (win['windows'], win['code'].tolist(), win['n_points'].tolist(), win['iterations'].tolist(), win['rms'].tolist(), ties, worst))
    assert len(win['windows']) >= 1 and len(ties) * 4 <= len(fw)
    assert (worst <= margin).all(), (worst, margin)
    # what more views buy, against the truth
    Rt, Tt = synthetic.stream_poses(sc.PHYSICS["n_frames"], seed=sc.PHYSICS["seed"], max_angle_deg=sc.PHYSICS["max_angle_deg"], step=sc.PHYSICS["step"])
    Tt = np.asarray(Tt).reshape(-1, 3)
    group = pts['frame_group']
    fr = list(range(len(group)))
    assert group.tolist() == [0] * 6, group                               # the chain of this stream holds
    r0, c0 = wm.pose_errors(d[pts['chain']][fr], pts['T_abs'][fr], Rt[fr], Tt[fr])
    r1, c1 = wm.pose_errors(d['R_abs_win'][fr], d['T_abs_win'][fr], Rt[fr], Tt[fr])
    print("PHYSICS chain over frames %s: rotation median %.4f -> %.4f deg (worst %.4f -> %.4f), centre median %.4f -> %.4f l (worst %.4f -> %.4f)" %
          (fr, np.median(r0), np.median(r1), r0.max(), r1.max(), np.median(c0), np.median(c1), c0.max(), c1.max()))
    assert np.median(r1) <= np.median(r0) + wm.WINDOW_ROT_BAND_DEG
    assert np.median(c1) <= np.median(c0) + wm.WINDOW_CENTRE_BAND
    pe.close()
