"""CPU tests of the track points: the float64 model (tests/track_point_model.py, the header's rule in scalar Python) on the
hand-built scenes of tests/track_point_cases.py -- what it recovers from exact data, every code, the reselection round, the
group rule, the parallax gate -- geometry.frame_groups against values written out by hand, the C-ABI surface, and the
accuracy table of DESIGN section 8."""
import os
import re

import numpy as np
import pytest

from tests import bundle_math_model as mm
from tests import camera_model as cm
from tests import track_point_cases as tc
from tests import track_point_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    """the model's dict of every case, computed once"""
    return {c['name']: (c, tm.model_case(c)) for c in tc.cases()}


def _rel(points, truth):
    return np.linalg.norm(points - truth, axis=1) / np.linalg.norm(truth, axis=1)


@pytest.mark.parametrize("lens", [False, True])
def test_noise_free_scenes_recover_the_points(lens):
    """Tracks of 2, 3 and 8 views, one K and a lens camera: 1e-9 relative.  That is below what f32 pixels allow (half an
    ulp of a VGA coordinate is 3e-5 px, 1e-7 of the focal length), so the model is fed the f64 pixels here, and the lens
    is one on which the five undistortion rounds converge; the f32 cases follow below at the accuracy f32 gives."""
    case = tc.clean(lens, weak=True)
    r = tm.model_case(case, exact_pixels=case['pixels'])
    assert (r['code'] == tm.OK).all() and sorted(set(r['n_used'].tolist())) == [2, 3, 8]
    assert (r['n_inliers'] == r['n_used']).all() and (r['obs_flag'] == 1).all()
    rel = _rel(r['points'], case['truth'])
    print("noise-free, f64 pixels, lens" if lens else "noise-free, f64 pixels, K", "worst relative error %.3g" % rel.max())
    assert rel.max() < 1e-9
    assert r['rms'].max() < 1e-9


@pytest.mark.parametrize("name", ["clean_k", "clean_lens"])
def test_f32_pixels_cost_what_their_rounding_is(results, name):
    """the same scenes from f32 pixels (per-frame MILD / RATIONAL / WEAK lenses in clean_lens): the error of the rounding,
    3e-5 px, and of five undistortion rounds, 1e-4 px -- 1e-5 relative is ten times that at these baselines"""
    case, r = results[name]
    assert (r['code'] == tm.OK).all()
    assert _rel(r['points'], case['truth']).max() < 1e-5 and r['rms'].max() < 1e-3


def test_every_case_stays_clear_of_the_gate(results):
    for name, (case, r) in results.items():
        thr = case['gates']['threshold_px']
        e = r['obs_err'][r['obs_flag'] > 0]
        assert not ((e > 0.9 * thr) & (e < 1.1 * thr)).any(), name
        mc = r['min_cos'][np.isin(r['code'], (tm.OK, tm.LOW_PARALLAX))]
        gate = case['gates']['max_cos']
        assert gate == 1.0 or (np.abs(mc - gate) > 1e-4).all(), name
        for k in tm.FLOAT_KEYS:
            assert np.isfinite(r[k]).all(), (name, k)


def test_displaced_observation_is_flagged_and_the_point_recovers(results):
    case, r = results["outlier"]
    ts = case['tracks']['track_start']
    assert r['code'].tolist() == [tm.OK, tm.OK, tm.OK, tm.OUTLIERS]
    assert r['n_used'].tolist() == [3, 5, 8, 2] and r['n_inliers'].tolist() == [2, 4, 7, 0]
    for t in range(3):
        flags = r['obs_flag'][ts[t]:ts[t + 1]].tolist()
        assert flags == [1, 2] + [1] * (len(flags) - 2), t
        assert abs(r['obs_err'][ts[t] + 1] - tc.OUTLIER_PX) < 0.5
    assert _rel(r['points'][:3], case['truth'][:3]).max() < 1e-5          # the f32 bound of the clean cases
    assert r['rms'][:3].max() < 1e-3
    # without the reselection the displaced observation drags the point away
    once = tm.triangulate_tracks(case['tracks'], case['R_abs'], case['T_abs'], case['cams'], **dict(case['gates'], threshold_px=1e9))
    assert _rel(once['points'][:3], case['truth'][:3]).min() > 1e-3
    # the same point from two views: nothing says which of the two is wrong
    assert r['obs_flag'][ts[3]:ts[4]].tolist() == [2, 2] and r['min_cos'][3] == 0.0


def test_degenerate_behind_and_too_few(results):
    case, r = results["degenerate"]
    v = tm.make_views(case['tracks']['obs_frame'], case['tracks']['obs_xy'], case['R_abs'], case['T_abs'], case['cams'])
    assert [x.d for x in v] == [[0.0, 0.0, 1.0]] * 2                    # the matrix is exactly diag(2, 2, 0)
    assert r['code'].tolist() == [tm.DEGENERATE] and not r['points'].any() and not r['obs_flag'].any()
    case, r = results["behind"]
    assert r['code'].tolist() == [tm.BEHIND] and r['obs_flag'].tolist() == [2, 2] and r['n_inliers'].tolist() == [0]
    assert np.allclose(r['points'][0], [0.5, 0.0, -2.5], atol=1e-6)     # the midpoint is returned
    case, r = results["too_few_min_views"]
    n = np.diff(case['tracks']['track_start'])
    assert (r['code'][n == 2] == tm.TOO_FEW).all() and (r['code'][n > 2] == tm.OK).all()
    assert not r['points'][n == 2].any() and (r['n_used'] == n).all()


def test_groups(results):
    case, r = results["groups"]
    ts = case['tracks']['track_start']
    assert r['code'].tolist() == [tm.OK, tm.TOO_FEW, tm.OK, tm.TOO_FEW] and r['n_used'].tolist() == [4, 1, 2, 0]
    assert r['obs_flag'][ts[0]:ts[1]].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]        # the first group's views only
    assert r['obs_flag'][ts[2]:ts[3]].tolist() == [0, 1, 1]                       # the used set is the last two observations
    assert _rel(r['points'][[0, 2]], case['truth'][[0, 2]]).max() < 1e-5
    # with every frame in one group the views on the other scale come in and spoil the point
    T = np.nan_to_num(case['T_abs'])
    mixed = tm.triangulate_tracks(case['tracks'], case['R_abs'], T, case['cams'], None, **case['gates'])
    assert mixed['n_used'][0] == 8 and mixed['code'][0] != tm.OK


def test_low_parallax_gate(results):
    case, r = results["parallax"]
    assert r['code'].tolist() == [tm.OK, tm.OK, tm.LOW_PARALLAX, tm.LOW_PARALLAX]
    assert (r['min_cos'][:2] < case['gates']['max_cos']).all() and (r['min_cos'][2:] > case['gates']['max_cos']).all()
    assert r['points'][2:].any(1).all()                                           # the point is still returned
    off = tm.triangulate_tracks(case['tracks'], case['R_abs'], case['T_abs'], case['cams'], **dict(case['gates'], max_cos=1.0))
    assert (off['code'] == tm.OK).all()
    assert np.array_equal(off['points'], r['points']) and np.array_equal(off['min_cos'], r['min_cos'])


def test_max_iters_zero_is_the_midpoint(results):
    case, r = results["midpoint"]
    assert (r['iterations'] == 0).all() and (r['code'] == tm.OK).all()
    ts = case['tracks']['track_start']
    v = tm.make_views(case['tracks']['obs_frame'], case['tracks']['obs_xy'], case['R_abs'], case['T_abs'], case['cams'])
    for t in (0, 7, 39):
        assert r['points'][t].tolist() == tm.midpoint(v[ts[t]:ts[t + 1]])
    lm = tm.model_case(dict(case, gates=dict(case['gates'], max_iters=10)))
    assert (lm['iterations'] > 0).all() and (lm['rms'] <= r['rms']).all() and (lm['rms'] < r['rms']).any()


def test_frame_groups_by_hand():
    from relative_pose_estimation_amd import geometry
    eye = np.stack([np.eye(3)] * 4); t = np.tile([1.0, 0.0, 0.0], (4, 1)); one = np.ones(3)

    def groups(status, code):
        seg = geometry.chain_trajectory(eye, t, status, one, code)[4]
        return seg.tolist(), geometry.frame_groups(status, seg).tolist()
    # a failed pair: frame 2 is related to nothing before it and is the origin of the next segment
    assert groups([0, 1, 0, 0], [0, 0, 0]) == ([0, 1, 2, 2], [0, 0, 2, 2, 2])
    # a failed link between two OK pairs: frame 2 lies in both segments and goes with the earlier one
    assert groups([0, 0, 0, 0], [0, 1, 0]) == ([0, 0, 1, 1], [0, 0, 0, 1, 1])
    # a failed last pair: the last frame has no pose
    assert groups([0, 0, 0, 1], [0, 0, 0]) == ([0, 0, 0, 1], [0, 0, 0, 0, -1])
    # a failed first pair: frame 0 is alone in its group
    assert groups([1, 0, 0, 0], [0, 0, 0]) == ([0, 1, 1, 1], [0, 1, 1, 1, 1])
    assert geometry.frame_groups([0], [0]).tolist() == [0, 0] and geometry.frame_groups([2], [0]).tolist() == [0, -1]
    with pytest.raises(ValueError):
        geometry.frame_groups([0, 0], [0])


def test_capi_surface():
    from relative_pose_estimation_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "rpe_amd.h")).read()
    enum = re.search(r"enum \{ (RPE_TRACKPT_OK[^}]*)\};", hdr).group(1)
    vals = {k.strip(): int(v) for k, v in (x.split("=") for x in enum.replace("\n", " ").split(","))}
    for name, v in vals.items():
        assert getattr(_capi, name[4:]) == v == getattr(tm, name[len("RPE_TRACKPT_"):])
    assert _capi.TRACKPT_NAMES == tuple(k[len("RPE_TRACKPT_"):] for k in sorted(vals, key=vals.get))
    assert "rpe_triangulate_tracks" in _capi.EXPORTS
    csrc = os.path.join(ROOT, "relative_pose_estimation_amd", "csrc")
    dev = open(os.path.join(csrc, "bundle_math.h")).read()             # the constants live with lm_loop, once on either side
    assert '#include "bundle_math.h"' in open(os.path.join(csrc, "geom_device.h")).read()
    for name, v, model in (("REFINE_LAMBDA0", "1e-3", mm.LAMBDA0), ("REFINE_REL_TOL", "1e-6", mm.REL_TOL),
                           ("REFINE_STEP_TOL", "1e-9", mm.STEP_TOL)):
        assert model == float(v), name
        assert re.search(rf"#define {name} {v}\b", dev), name
        assert sum(len(re.findall(rf"#define {name}\b", open(os.path.join(csrc, f)).read())) for f in os.listdir(csrc)
                   if f.endswith((".h", ".hip"))) == 1, name


ACCURACY_VIEWS = (2, 3, 5, 8)


def accuracy_table(n=200, noise=0.3):
    """rows (views, median and worst error of the N-view point, median and worst of the two-view midpoint of the track's
    first two views), errors relative to the point's depth in frame 0; one scene, 0.3 px noise"""
    rows = []
    for nv in ACCURACY_VIEWS:
        case = tc.noisy(nv, n=n, noise=noise)
        r = tm.model_case(case)
        assert (r['code'] == tm.OK).all()
        ts = case['tracks']['track_start']
        two = {'track_start': np.arange(0, 2 * n + 1, 2, dtype=np.int32),
               'obs_frame': np.stack([case['tracks']['obs_frame'][ts[:-1]], case['tracks']['obs_frame'][ts[:-1] + 1]], 1).reshape(-1),
               'obs_xy': np.stack([case['tracks']['obs_xy'][ts[:-1]], case['tracks']['obs_xy'][ts[:-1] + 1]], 1).reshape(-1, 2)}
        mid = tm.triangulate_tracks(two, case['R_abs'], case['T_abs'], case['cams'], **dict(case['gates'], max_iters=0))
        depth = (case['truth'] @ case['R_abs'][0][2]) + case['T_abs'][0][2]
        en = np.linalg.norm(r['points'] - case['truth'], axis=1) / depth
        em = np.linalg.norm(mid['points'] - case['truth'], axis=1) / depth
        rows.append((nv, float(np.median(en)), float(en.max()), float(np.median(em)), float(em.max())))
    return rows


def test_accuracy_table():
    rows = accuracy_table()
    print("\nviews | N-view point: median, worst | two-view midpoint of the first two views: median, worst   (error / depth, 0.3 px noise, 200 tracks)")
    for nv, a, b, c, d in rows:
        print(f"{nv:5d} | {a:.5f} {b:.5f} | {c:.5f} {d:.5f}")
    assert rows[-1][0] == 8 and rows[0][0] == 2 and rows[-1][1] < rows[0][1]
