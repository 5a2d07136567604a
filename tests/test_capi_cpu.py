"""CPU tests of the boundary: the C-ABI library loads and exports every symbol the
header declares; no compute call is made without a GPU; the product fails loudly
when no HIP device is present; the drop-in class mirrors the reference's errors."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_declarations():
    """name -> (return type, [parameter declarations]) of every function include/rpe_amd.h declares"""
    src = open(os.path.join(ROOT, "include", "rpe_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", "", src, flags=re.M)
    decls = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(rpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = [p.strip() for p in params.split(",")]
        decls[name] = (" ".join(ret.split()), [] if params in ([""], ["void"]) else params)
    return decls


def _header_symbols():
    return sorted(_header_declarations())


def test_library_exports_every_declared_symbol():
    from relative_pose_estimation_amd import _capi
    lib = _capi.load()
    syms = _header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rpe_amd.h but not exported"
    assert sorted(_capi.EXPORTS) == syms


def _ctypes_class(decl, is_return=False):
    """the ctypes class a C declaration binds to: a pointer type for pointers and arrays, else the scalar's own"""
    import ctypes as C
    if "*" in decl or "[" in decl:
        return C.c_char_p if is_return else "pointer"
    words = [w for w in decl.split() if w != "const"]
    ctype = " ".join(words if is_return else words[:-1])          # a parameter's last word is its name
    return {"int": C.c_int, "int32_t": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64, "void": None}[ctype]


def _binding_mismatches(signatures):
    import ctypes as C
    decls = _header_declarations()
    bad = sorted(set(decls) ^ set(signatures))
    for name in sorted(set(decls) & set(signatures)):
        ret, params = decls[name]
        restype, argtypes = signatures[name]
        bound = ["pointer" if t is C.c_void_p or issubclass(t, (C._Pointer, C.Array)) else t for t in argtypes]
        if restype is not _ctypes_class(ret, True) or bound != [_ctypes_class(p) for p in params]:
            bad.append(name)
    return len(decls), bad


def test_binding_table_matches_the_header():
    """ctypes takes any argtypes: a wrong arity, or a c_int where the header has a double, only shows as wrong numbers.
    Every function the header declares is bound with as many parameters, of the class the declaration has (pointer or
    array -> a pointer type, int / int32_t -> c_int, double -> c_double, size_t -> c_size_t, int64_t -> c_int64), and
    with its return type.  Reads the table only; the library is not loaded."""
    import ctypes as C
    from relative_pose_estimation_amd import _capi
    n, bad = _binding_mismatches(_capi.SIGNATURES)
    assert n >= 76 and bad == [], bad
    # the comparison itself: a wrong class, a wrong arity and a wrong return type are each found
    for name, wrong in (("rpe_guided_matches", lambda r, a: (r, a[:4] + [C.c_int] + a[5:])),      # gate_px is a double
                        ("rpe_fetch_results", lambda r, a: (r, a[:-1])),
                        ("rpe_orb_pyramid_pixels", lambda r, a: (C.c_int, a))):
        sig = dict(_capi.SIGNATURES)
        sig[name] = wrong(*sig[name])
        assert _binding_mismatches(sig)[1] == [name]


def test_no_cpu_fallback():
    from relative_pose_estimation_amd import _capi
    lib = _capi.load()
    if lib.rpe_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_capi.RpeError, match="no HIP device"):
        _capi.Engine(640, 480)
    from relative_pose_estimation_amd import PoseEstimator
    pe = PoseEstimator(np.eye(3))
    with pytest.raises(_capi.RpeError):
        pe.estimate(np.zeros((480, 640), np.uint8), np.zeros((480, 640), np.uint8))


def test_configuration_limits_are_checked_before_the_device():
    """rpe_create validates the configuration first (no GPU needed): SIFT accepts nfeatures = 0 -- the reference's
    uncapped cv2.SIFT_create(), pose_estimator.py:93-94 -- and caps up to 16320; ORB needs 1 .. 8000."""
    from relative_pose_estimation_amd import _capi
    if _capi.load().rpe_device_count() > 0:
        pytest.skip("a GPU is present")
    sift = dict(feature_method=_capi.FEATURE_SIFT, norm_type=_capi.NORM_L2)
    for kw, msg in ((dict(nfeatures=0), "out of supported range"), (dict(nfeatures=8001), "out of supported range"),
                    (dict(nfeatures=16321, **sift), "NORM_L2: nfeatures must be <= 16320"), (dict(nfeatures=-1, **sift), "SIFT: nfeatures must be 0"),
                    (dict(nfeatures=8000, norm_type=_capi.NORM_L2), "no HIP device"),
                    (dict(nfeatures=0, **sift), "no HIP device"), (dict(nfeatures=16320, **sift), "no HIP device"),
                    (dict(max_matches=8065), "out of supported range"), (dict(stl_runtime=2), "unknown stl_runtime")):
        with pytest.raises(_capi.RpeError, match=msg):
            _capi.Engine(640, 480, **kw)


def test_product_never_imports_oracle():
    """the shipped path must not import, link, include or dlopen anything under oracle/"""
    pkg = os.path.join(ROOT, "relative_pose_estimation_amd")
    bad = re.compile(r"^\s*(import\s+oracle|from\s+oracle)|liboracle|#\s*include\s*[\"<][^\">]*oracle|-loracle|orc_[a-z_]+\s*\(", re.M)
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".inc")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert not bad.search(txt), f


def test_constructor_mirrors_reference():
    from relative_pose_estimation_amd import PoseEstimator
    import inspect
    sig = inspect.signature(PoseEstimator.__init__)
    names = list(sig.parameters)[1:14]
    assert names == ["camera_matrix", "feature_method", "norm_type", "max_matches", "nfeatures", "use_vp_refinement",
                     "vp_max_lines", "vp_max_pairs", "vp_acc_min", "vp_vp2_min", "vp_iters", "vp_lm_lambda",
                     "vp_cost_improve_eps"]                                      # pose_estimator.py:19-32
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["feature_method"], d["norm_type"], d["max_matches"], d["nfeatures"], d["use_vp_refinement"]) == ("ORB", "Hamming", 500, 4000, False)
    with pytest.raises(ValueError, match="Unknown feature extraction method: FOO"):  # pose_estimator.py:96
        PoseEstimator(np.eye(3), feature_method="foo")
    with pytest.raises(ValueError, match="Unknown norm type: L7"):                   # pose_estimator.py:129
        PoseEstimator(np.eye(3), norm_type="l7")
    with pytest.raises(RuntimeError, match=r"Insufficient matches: 3 \(minimum 5 required\)"):  # :514-515
        PoseEstimator._raise_for(2, 3)
    with pytest.raises(RuntimeError, match="Could not estimate Essential matrix."):   # :529-530
        PoseEstimator._raise_for(3, 9)


def test_scene_args_prepare_and_refuse_the_track_scene():
    """_capi._scene_args, the head of Engine.triangulate_tracks and Engine.bundle_windows, needs no library: C-contiguous
    i32 / f32 / f64 arrays of the documented shapes, and a ValueError carrying the caller's name for a pose-count
    mismatch, a track_start that does not end at the number of observations, an empty track_start, both K and cameras,
    neither K nor cameras"""
    from relative_pose_estimation_amd import _capi
    tracks = {'track_start': [0, 2, 4, 7], 'obs_frame': np.arange(7, dtype=np.int64) % 3,
              'obs_xy': np.arange(28, dtype=np.float64).reshape(7, 4)[:, ::2]}         # neither the dtype nor the layout wanted
    R = np.tile(np.eye(3, dtype=np.float32), (3, 1, 1))
    T = np.zeros((3, 3))
    K = np.array([[500., 0., 320.], [0., 500., 240.], [0., 0., 1.]]).T.copy().T        # not C-contiguous
    cam = _capi.Camera(K)
    ts, of, xy, Rc, Tc, F, n, k, cams = _capi._scene_args("who", tracks, R, T, K, None)
    assert (F, n, cams) == (3, 3, None)
    for a, dtype, shape in ((ts, np.int32, (4,)), (of, np.int32, (7,)), (xy, np.float32, (7, 2)), (Rc, np.float64, (3, 9)),
                            (Tc, np.float64, (3, 3)), (k, np.float64, (9,))):
        assert a.dtype == dtype and a.shape == shape and a.flags['C_CONTIGUOUS'], (a.dtype, a.shape)
    assert ts.tolist() == [0, 2, 4, 7] and np.array_equal(xy, np.asarray(tracks['obs_xy'], np.float32))
    assert np.array_equal(Rc, R.reshape(3, 9)) and k.tolist() == K.reshape(9).tolist()
    k, cams = _capi._scene_args("who", tracks, R, T, None, cam)[-2:]
    assert k is None and cams.dtype == _capi.CAMERA_DTYPE and cams.shape == (3,) and cams.flags['C_CONTIGUOUS']
    for who in ("triangulate_tracks", "bundle_windows"):
        for bad, K_, cam_, what in ((dict(R_abs=R[:2]), K, None, "one pose per frame"),
                                    (dict(tracks=dict(tracks, track_start=[0, 2, 4, 6])), K, None, "must end at the number of observations"),
                                    (dict(tracks=dict(tracks, track_start=[])), K, None, "must end at the number of observations"),
                                    ({}, K, cam, "exactly one of K and cameras"), ({}, None, None, "exactly one of K and cameras")):
            args = dict(dict(tracks=tracks, R_abs=R, T_abs=T), **bad)
            with pytest.raises(ValueError, match=who + ": .*" + what):
                _capi._scene_args(who, args['tracks'], args['R_abs'], args['T_abs'], K_, cam_)
