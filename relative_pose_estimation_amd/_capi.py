"""ctypes binding of include/rpe_amd.h (librpe_amd.so, HIP / gfx950).

There is no CPU fallback: if the shared library is missing or no HIP device is
visible, loading / handle creation raises.  Nothing here imports oracle/.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RPE_LIB", os.path.join(_HERE, "librpe_amd.so"))   # RPE_LIB: diagnostic builds only

ABI_VERSION = 3
ORB_LEVELS = 12
PAIR_OK, PAIR_NO_DESCRIPTORS, PAIR_INSUFFICIENT_MATCHES, PAIR_NO_ESSENTIAL, PAIR_AMBIGUOUS_ESSENTIAL = 0, 1, 2, 3, 4
FEATURE_ORB, FEATURE_SIFT = 0, 1
NORM_HAMMING, NORM_L2 = 0, 1
MATCH_CROSSCHECK, MATCH_RATIO = 0, 1
STL_LIBSTDCXX, STL_MSVC = 0, 1          # whose nth_element orders the keypoints (include/rpe_amd.h RPE_STL_*)
# capacity flags (rpe_fetch_overflow)
OVF_ORB_CANDIDATES, OVF_ORB_KEYPOINTS = 1 << 0, 1 << 1
OVF_SIFT_SEEDS, OVF_SIFT_RAW, OVF_SIFT_PREFILTER, OVF_SIFT_CAP, OVF_SIFT_KEYPOINTS = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
SIFT_UNCAPPED_CAPACITY = 16320   # RPE_SIFT_UNCAPPED_CAPACITY: keypoints per image kept by SIFT with nfeatures = 0
MAX_MATCHES_LIMIT = 8064          # rpe_config.max_matches upper bound
CALIB_KINDS = 18
STAGE_COUNT = 12
ORDER_BGR, ORDER_RGB = 0, 1
REFINE_OK, REFINE_SKIPPED, REFINE_REJECTED = 0, 1, 2   # info[:, 0] of refine_poses (include/rpe_amd.h RPE_REFINE_*)
LINK_OK, LINK_PAIR_FAILED, LINK_TOO_FEW = 0, 1, 2      # code[] of scale_links (include/rpe_amd.h RPE_LINK_*)
HOMOGRAPHY_OK, HOMOGRAPHY_SKIPPED, HOMOGRAPHY_NONE = 0, 1, 2   # info[:, 0] of pair_homographies (include/rpe_amd.h RPE_HOMOGRAPHY_*)
LINKPOSE_OK, LINKPOSE_PAIR_FAILED, LINKPOSE_TOO_FEW, LINKPOSE_NONE = 0, 1, 2, 3   # info[:, 0] of link_poses (RPE_LINKPOSE_*)
BUNDLE_OK, BUNDLE_PAIR_FAILED, BUNDLE_TOO_FEW, BUNDLE_SKIPPED, BUNDLE_REJECTED = 0, 1, 2, 3, 4   # info[:, 0] of link_bundles (RPE_BUNDLE_*)
TRACK_EDGES_USABLE, TRACK_EDGES_RANSAC, TRACK_EDGES_ALL = 0, 1, 2   # edge_rule of build_tracks (RPE_TRACK_EDGES_*)
TRACK_COUNTS = ("n_tracks", "n_obs", "n_edges", "dropped_conflict", "dropped_short", "n_frames_seen")   # counts[6] of the track calls
# info[:, 0] / 'code' of triangulate_tracks (RPE_TRACKPT_*)
TRACKPT_OK, TRACKPT_TOO_FEW, TRACKPT_DEGENERATE, TRACKPT_BEHIND, TRACKPT_OUTLIERS, TRACKPT_LOW_PARALLAX = 0, 1, 2, 3, 4, 5
TRACKPT_NAMES = ("OK", "TOO_FEW", "DEGENERATE", "BEHIND", "OUTLIERS", "LOW_PARALLAX")
# info[:, 0] / 'code' of bundle_windows (RPE_WINDOW_*)
WINDOW_OK, WINDOW_NO_BASELINE, WINDOW_TOO_FEW, WINDOW_REJECTED = 0, 1, 2, 3
WINDOW_NAMES = ("OK", "NO_BASELINE", "TOO_FEW", "REJECTED")
WINDOW_MAX_VIEWS, WINDOW_MAX_POINTS = 8, 16384   # RPE_WINDOW_MAX_VIEWS, RPE_WINDOW_MAX_POINTS
# info[:, 0] / 'code' of optimise_graphs (RPE_GRAPH_*), the kinds of its edges (RPE_EDGE_*) and its capacities
GRAPH_OK, GRAPH_NO_EDGES, GRAPH_UNDERDETERMINED, GRAPH_REJECTED = 0, 1, 2, 3
GRAPH_NAMES = ("OK", "NO_EDGES", "UNDERDETERMINED", "REJECTED")
EDGE_METRIC, EDGE_DIRECTION = 0, 1
GRAPH_MAX_FRAMES, GRAPH_MAX_EDGES = 4096, 65536   # RPE_GRAPH_MAX_FRAMES, RPE_GRAPH_MAX_EDGES
SIMILAR_MAX_K = 32             # RPE_SIMILAR_MAX_K: the most candidates per query row of the similarity calls
UNDISTORT_ITERS = 5               # RPE_UNDISTORT_ITERS: fixed-point rounds of the camera path's undistortion

# The binding, one entry per function of include/rpe_amd.h: "<return>:<one letter per parameter>".  Parameters: p pointer or
# array, i int / int32_t, d double, z size_t.  Returns: i int, l int64_t, s const char *, v void.  ctypes checks nothing
# against the header (a wrong arity or an int where the header has a double goes through silently), so
# tests/test_capi_cpu.py compares this table with the header's declarations.
_SIGNATURES = {
    "rpe_default_config": "v:p", "rpe_create": "i:pp", "rpe_destroy": "v:p", "rpe_last_error": "s:p", "rpe_device_count": "i:",
    "rpe_keypoint_capacity": "i:p", "rpe_device_malloc": "i:pzp", "rpe_device_free": "i:pp", "rpe_memcpy_h2d": "i:pppz",
    "rpe_memcpy_d2h": "i:pppz", "rpe_synchronize": "i:p", "rpe_host_alloc": "i:pzp", "rpe_host_free": "i:pp",
    "rpe_host_register": "i:ppz", "rpe_host_unregister": "i:pp",
    "rpe_estimate_batch": "i:pppipppppp", "rpe_estimate_batch_device": "i:pppipppppp", "rpe_enqueue_batch_device": "i:pppip",
    "rpe_fetch_results": "i:pippppp", "rpe_fetch_overflow": "i:pip", "rpe_estimate_stream": "i:ppipppppp",
    "rpe_enqueue_stream_device": "i:ppip",
    "rpe_frames_reserve": "i:pi", "rpe_frames_capacity": "i:p", "rpe_frames_put_device": "i:ppip", "rpe_frames_put": "i:ppip",
    "rpe_frames_info": "i:pippp", "rpe_enqueue_pairs": "i:pppip", "rpe_estimate_pairs": "i:pppipppppp",
    "rpe_frames_set_cameras": "i:pipp", "rpe_enqueue_pairs_cameras": "i:pppi", "rpe_estimate_pairs_cameras": "i:pppippppp",
    "rpe_enqueue_batch_cameras_device": "i:pppipp", "rpe_estimate_batch_cameras_device": "i:pppippppppp",
    "rpe_estimate_batch_cameras": "i:pppippppppp", "rpe_undistort_points": "i:ppipp",
    "rpe_find_essential_cameras": "i:ppppipppppp", "rpe_recover_pose_cameras": "i:pppppippppp",
    "rpe_refine_pose_points_cameras": "i:pppppppippippppp",
    "rpe_bgr_to_gray_device": "i:ppzip", "rpe_bgr_to_gray": "i:ppzip", "rpe_lsd_detect": "i:piipip",
    "rpe_fetch_matched_points": "i:pipp", "rpe_fetch_structure": "i:pippp", "rpe_refine_poses": "i:piippppp",
    "rpe_fetch_match_indices": "i:pipp", "rpe_scale_links": "i:pipppippp", "rpe_link_poses": "i:pipppidiipppppp",
    "rpe_link_bundles": "i:pipppppdiippppppppp", "rpe_bundle_three_view": "i:pippppppppppddippppppppp",
    "rpe_last_run_pairs": "i:p", "rpe_build_tracks": "i:ppiipppppp", "rpe_tracks_from_matches": "i:piippppppppipppppp",
    "rpe_triangulate_tracks": "i:pipppipppppdidipppppp",
    "rpe_bundle_windows": "i:pippppppippppippiiippppppp",
    "rpe_optimise_graphs": "i:pippipppppppppp" "diid" "ppppppp",
    "rpe_frames_similar": "i:pipipiippiiipppp", "rpe_similarity_hamming": "i:pppiipipiippiiipppp",
    "rpe_guided_matches": "i:pippdipppppp",
    "rpe_guided_matches_l2": "i:pippddpppppp",
    "rpe_pair_homographies": "i:piidppppp", "rpe_find_homography": "i:ppppipidppppp",
    "rpe_orb_detect_and_compute": "i:ppippp", "rpe_orb_debug_fetch": "i:piip", "rpe_orb_pyramid_pixels": "l:p",
    "rpe_orb_group_min_images": "i:",
    "rpe_orb_debug_retain": "i:piipppiip",
    "rpe_match_hamming": "i:pppppipppp", "rpe_match_hamming_guided": "i:pppppppipppdipppp",
    "rpe_sift_detect_and_compute": "i:ppippp", "rpe_sift_debug_gauss": "l:pip", "rpe_match_l2": "i:pppppipppp",
    "rpe_match_l2_guided": "i:pppppppipppddpppp",
    "rpe_find_essential": "i:ppppippppp", "rpe_recover_pose": "i:pppppipppp", "rpe_refine_pose_points": "i:pppppppipippppp",
    "rpe_set_profiling": "i:pi", "rpe_get_stage_ms": "i:pp", "rpe_stage_name": "s:i",
    "rpe_comm_unique_id": "i:p", "rpe_comm_create": "i:piipp", "rpe_comm_prepare": "i:piip", "rpe_comm_connect": "i:pp",
    "rpe_comm_destroy": "i:p", "rpe_comm_last_error": "s:", "rpe_gather_poses": "i:ppiiip", "rpe_comm_allreduce_max": "i:pp",
    "rpe_comm_barrier": "i:p",
    "rpe_calibrate_valu": "i:piip", "rpe_calibrate_valu_name": "s:i", "rpe_calibrate_hbm": "i:pp",
}
_ARG = {"p": C.c_void_p, "i": C.c_int, "d": C.c_double, "z": C.c_size_t}
_RET = {"i": C.c_int, "l": C.c_int64, "s": C.c_char_p, "v": None}
# name -> (restype, argtypes): what load() sets on the library, readable without it
SIGNATURES = {name: (_RET[sig[0]], [_ARG[c] for c in sig[2:]]) for name, sig in _SIGNATURES.items()}
EXPORTS = list(SIGNATURES)


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("max_batch", C.c_int32), ("feature_method", C.c_int32), ("norm_type", C.c_int32),
                ("max_matches", C.c_int32), ("nfeatures", C.c_int32), ("fast_threshold", C.c_int32),
                ("ransac_max_iters", C.c_int32), ("ransac_prob", C.c_double), ("ransac_threshold", C.c_double),
                ("match_mode", C.c_int32), ("stl_runtime", C.c_int32), ("match_ratio", C.c_double)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("lx", "<i4"), ("ly", "<i4")])

SIFT_KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                          ("octave", "<i4")])

# struct rpe_camera (include/rpe_amd.h): 96 bytes
CAMERA_DTYPE = np.dtype([("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("dist", "<f8", (8,))])

_lib = None


class RpeError(RuntimeError):
    pass


class Camera:
    """Camera model of one frame (struct rpe_camera): pinhole intrinsics from K (fx, fy, cx, cy; skew is ignored, as
    everywhere in the library) and cv2's distortion coefficients in cv2's order (k1, k2, p1, p2[, k3[, k4, k5, k6]]):
    `dist` holds 4, 5 or 8 values, None = pinhole.  Validated here, before any device call: finite fields, fx > 0,
    fy > 0."""

    def __init__(self, K, dist=None):
        K = np.asarray(K, np.float64)
        if K.shape != (3, 3):
            raise ValueError(f"Camera: K must be 3 x 3, got shape {K.shape}")
        d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).reshape(-1)
        if d.size not in (0, 4, 5, 8):
            raise ValueError(f"Camera: dist must hold 4, 5 or 8 coefficients (cv2 order), got {d.size}")
        self.fx, self.fy, self.cx, self.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        self.dist = np.zeros(8)
        self.dist[:d.size] = d
        if not (np.isfinite([self.fx, self.fy, self.cx, self.cy]).all() and np.isfinite(self.dist).all()):
            raise ValueError("Camera: non-finite field")
        if not (self.fx > 0 and self.fy > 0):
            raise ValueError("Camera: fx and fy must be > 0")

    @property
    def K(self):
        return np.array([[self.fx, 0., self.cx], [0., self.fy, self.cy], [0., 0., 1.]])

    def record(self):
        r = np.zeros(1, CAMERA_DTYPE)
        r["fx"], r["fy"], r["cx"], r["cy"], r["dist"] = self.fx, self.fy, self.cx, self.cy, self.dist
        return r


def camera_records(cameras, n):
    """n rpe_camera records from one Camera (repeated) or a sequence of n; an array of CAMERA_DTYPE passes through
    unchecked (the library validates it)"""
    if isinstance(cameras, np.ndarray) and cameras.dtype == CAMERA_DTYPE:
        rec = np.ascontiguousarray(cameras).reshape(-1)
    elif isinstance(cameras, Camera):
        rec = np.repeat(cameras.record(), n)
    else:
        cameras = list(cameras)
        if not all(isinstance(c, Camera) for c in cameras):
            raise ValueError("cameras: expected Camera objects")
        rec = np.concatenate([c.record() for c in cameras]) if cameras else np.zeros(0, CAMERA_DTYPE)
    if rec.size != n:
        raise ValueError(f"cameras: expected {n}, got {rec.size}")
    return np.ascontiguousarray(rec)


def load():
    """dlopen librpe_amd.so; raises (loudly) when the HIP extension is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RpeError(f"{LIB_PATH} not found: build it with __graft_entry__.build() "
                       "(make -C relative_pose_estimation_amd/csrc); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _opt(a):
    return None if a is None else _p(a)


def _f64(a):
    """a camera matrix (or any f64 array) as the library reads it"""
    return np.ascontiguousarray(a, np.float64)


def _i32(a):
    """slot numbers, counts, pair indices: a flat int32 array"""
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _slot_pairs(slot1, slot2):
    s1, s2 = _i32(slot1), _i32(slot2)
    assert s1.size == s2.size
    return s1, s2


def _scene_args(who, tracks, R_abs, T_abs, K, cameras):
    """The track scene of triangulate_tracks and bundle_windows as the library reads it: track_start i32[n + 1],
    obs_frame i32[n_obs], obs_xy f32[n_obs, 2], R f64[F, 9], T f64[F, 3], then F, n, K f64[9] or None and the F camera
    records or None"""
    ts, of = _i32(tracks['track_start']), _i32(tracks['obs_frame'])
    xy = np.ascontiguousarray(tracks['obs_xy'], np.float32).reshape(-1, 2)
    R = np.ascontiguousarray(np.asarray(R_abs, np.float64).reshape(-1, 9))
    T = np.ascontiguousarray(np.asarray(T_abs, np.float64).reshape(-1, 3))
    F, n = R.shape[0], ts.size - 1
    if n < 0 or T.shape[0] != F or of.size != xy.shape[0] or int(ts[-1]) != of.size:
        raise ValueError(f"{who}: track_start must end at the number of observations, and R_abs and T_abs hold one pose per frame")
    if (K is None) == (cameras is None):
        raise ValueError(f"{who}: exactly one of K and cameras must be given")
    return ts, of, xy, R, T, F, n, None if K is None else _f64(K).reshape(9), None if cameras is None else camera_records(cameras, F)


def lsd_detect(gray, capacity=8192):
    """cv2.createLineSegmentDetector(LSD_REFINE_STD).detect(gray)[0] restated: (N, 4) float64 segments
    (pose_estimator.py:160-175).  Host code inside librpe_amd.so; needs no GPU handle."""
    g = np.ascontiguousarray(gray, np.uint8)
    assert g.ndim == 2
    out = np.zeros((capacity, 4), np.float32)
    n = np.zeros(1, np.int32)
    rc = load().rpe_lsd_detect(_p(g), g.shape[1], g.shape[0], _p(out), capacity, _p(n))
    if rc != 0:
        raise RpeError(f"rpe_lsd_detect failed ({rc})")
    return out[:min(int(n[0]), capacity)].astype(np.float64)


class Engine:
    """One rpe_handle: one GPU, one stream, fixed image size and capacities."""

    def __init__(self, width, height, max_batch=1, nfeatures=4000, max_matches=500, device=0,
                 feature_method=FEATURE_ORB, norm_type=NORM_HAMMING, fast_threshold=15,
                 ransac_max_iters=1000, ransac_prob=0.999, ransac_threshold=1.0,
                 match_mode=MATCH_CROSSCHECK, match_ratio=0.75, stl_runtime=STL_LIBSTDCXX):
        self.lib = load()
        cfg = Config()
        self.lib.rpe_default_config(C.byref(cfg))
        cfg.device = device; cfg.width = width; cfg.height = height; cfg.max_batch = max_batch
        cfg.feature_method = feature_method; cfg.norm_type = norm_type
        cfg.max_matches = max_matches; cfg.nfeatures = nfeatures; cfg.fast_threshold = fast_threshold
        cfg.ransac_max_iters = ransac_max_iters; cfg.ransac_prob = ransac_prob; cfg.ransac_threshold = ransac_threshold
        cfg.match_mode = match_mode; cfg.match_ratio = match_ratio; cfg.stl_runtime = stl_runtime
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.lib.rpe_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RpeError(f"rpe_create failed ({rc}): {self.lib.rpe_last_error(None).decode()}")
        self.h = h
        self.width, self.height, self.max_batch = width, height, max_batch
        self.max_matches = max_matches
        self.kcap = self.lib.rpe_keypoint_capacity(h)
        self.desc_dim = 128 if feature_method == FEATURE_SIFT else 32

    def close(self):
        if getattr(self, "h", None):
            self.free_pinned()
            self.lib.rpe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RpeError(f"librpe_amd error {rc}: {self.lib.rpe_last_error(self.h).decode()}")

    # ---- device buffers
    def device_malloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.rpe_device_malloc(self.h, nbytes, C.byref(p)))
        return p

    def device_free(self, p):
        self._chk(self.lib.rpe_device_free(self.h, p))

    def pinned_empty(self, shape, dtype=np.uint8):
        """numpy array on page-locked host memory (rpe_host_alloc): image batches for estimate_batch / estimate_stream that
        upload without blocking and at the full PCIe rate.  Freed with the engine (or free_pinned)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self.lib.rpe_host_alloc(self.h, n, C.byref(p)))
        buf = (C.c_uint8 * n).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return arr

    def free_pinned(self):
        for p in getattr(self, "_pinned", []):
            self.lib.rpe_host_free(self.h, p)
        self._pinned = []

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.device_malloc(arr.nbytes)
        self._chk(self.lib.rpe_memcpy_h2d(self.h, p, _p(arr), arr.nbytes))
        return p

    def synchronize(self):
        self._chk(self.lib.rpe_synchronize(self.h))

    # ---- image ingest (image_loader.py:27-28: BGR2GRAY)
    def bgr_to_gray(self, images, order=ORDER_BGR):
        """(..., H, W, 3) uint8 -> (..., H, W) uint8 gray, cv2's fixed-point weights, computed on the GPU."""
        a = np.ascontiguousarray(images, np.uint8)
        assert a.shape[-1] == 3, a.shape
        out = np.empty(a.shape[:-1], np.uint8)
        self._chk(self.lib.rpe_bgr_to_gray(self.h, _p(a), out.size, order, _p(out)))
        return out

    def upload_bgr_as_gray(self, images, order=ORDER_BGR):
        """Upload interleaved 3-channel frames and convert them in HBM; returns the device pointer of
        the gray frames (caller frees) -- feeds enqueue_batch_device / enqueue_stream_device."""
        a = np.ascontiguousarray(images, np.uint8)
        assert a.shape[-1] == 3, a.shape
        n = a.size // 3
        d_bgr = self.upload(a)
        d_gray = self.device_malloc(n)
        try:
            self._chk(self.lib.rpe_bgr_to_gray_device(self.h, d_bgr, n, order, d_gray))
            self.synchronize()
        finally:
            self.device_free(d_bgr)
        return d_gray

    # ---- hot path
    def _outs(self, B):
        return (np.zeros((B, 3, 3)), np.zeros((B, 3, 1)), np.zeros(B, np.int32), np.zeros(B, np.int32),
                np.zeros(B, np.int32))

    def _image_pair(self, imgs1, imgs2):
        imgs1 = np.ascontiguousarray(imgs1, np.uint8); imgs2 = np.ascontiguousarray(imgs2, np.uint8)
        B = imgs1.shape[0]
        assert imgs1.shape == imgs2.shape == (B, self.height, self.width), (imgs1.shape, imgs2.shape)
        return imgs1, imgs2, B

    def _estimate(self, fn, n, *args):
        """fn(handle, *args, R, t, inliers, n_matches, status) over n pairs: the five results"""
        outs = self._outs(n)
        self._chk(fn(self.h, *args, *map(_p, outs)))
        return outs

    def estimate_batch(self, imgs1, imgs2, K):
        imgs1, imgs2, B = self._image_pair(imgs1, imgs2)
        K = _f64(K)
        return self._estimate(self.lib.rpe_estimate_batch, B, _p(imgs1), _p(imgs2), B, _p(K))

    def estimate_stream(self, frames, K):
        frames = np.ascontiguousarray(frames, np.uint8)
        F = frames.shape[0]
        assert frames.shape == (F, self.height, self.width)
        K = _f64(K)
        return self._estimate(self.lib.rpe_estimate_stream, F - 1, _p(frames), F, _p(K))

    def enqueue_stream_device(self, d_frames, F, K):
        K = _f64(K)
        self._chk(self.lib.rpe_enqueue_stream_device(self.h, d_frames, F, _p(K)))

    def estimate_batch_device(self, d_imgs1, d_imgs2, B, K):
        K = _f64(K)
        return self._estimate(self.lib.rpe_estimate_batch_device, B, d_imgs1, d_imgs2, B, _p(K))

    def enqueue_batch_device(self, d_imgs1, d_imgs2, B, K):
        K = _f64(K)
        self._chk(self.lib.rpe_enqueue_batch_device(self.h, d_imgs1, d_imgs2, B, _p(K)))

    def fetch_results(self, B):
        return self._estimate(self.lib.rpe_fetch_results, B, B)

    def fetch_overflow(self, n_pairs):
        """OVF_* capacity flags of the last batch / stream, one word per pair."""
        f = np.zeros(n_pairs, np.uint32)
        self._chk(self.lib.rpe_fetch_overflow(self.h, n_pairs, _p(f)))
        return f

    def fetch_matched_points(self, B):
        p1 = np.zeros((B, self.max_matches, 2), np.float32); p2 = np.zeros_like(p1)
        self._chk(self.lib.rpe_fetch_matched_points(self.h, B, _p(p1), _p(p2)))
        return p1, p2

    def fetch_structure(self, B):
        """Per-match results of the last batch / stream (rpe_fetch_structure): (ransac_mask bool[B, mm],
        pose_mask bool[B, mm], points f64[B, mm, 3]).  ransac_mask is findEssentialMat's inlier mask, pose_mask
        recoverPose's cheirality mask of the returned pose (sums to the inlier count), points the triangulated point
        of every match in the camera-1 frame on the |t| = 1 scale.  Zero past each pair's match count and for pairs
        whose status is not OK."""
        mm = self.max_matches
        rm = np.zeros((B, mm), np.uint8); pm = np.zeros((B, mm), np.uint8); pts = np.zeros((B, mm, 3))
        self._chk(self.lib.rpe_fetch_structure(self.h, B, _p(rm), _p(pm), _p(pts)))
        return rm.astype(bool), pm.astype(bool), pts

    def _refine_outs(self, B):
        return np.zeros((B, 3, 3)), np.zeros((B, 3, 1)), np.zeros(B, np.int32), np.zeros((B, 4), np.int32), np.zeros((B, 2))

    def refine_poses(self, B, max_iters=10):
        """Non-linear refinement of the poses of the last batch / stream (rpe_refine_poses; not in the reference):
        Levenberg-Marquardt on the Sampson error over findEssentialMat's inliers, started from the batch's (R, t).
        Returns (R[B,3,3], t[B,3,1], inliers[B], info[B,4], rms[B,2]): info = (REFINE_* code, iterations run, residuals
        used, accepted steps), rms = (before, after) in pixels.  The batch's own results are not modified."""
        outs = self._refine_outs(B)
        self._chk(self.lib.rpe_refine_poses(self.h, B, max_iters, *map(_p, outs)))
        return outs

    # ---- scale links (rpe_fetch_match_indices / rpe_scale_links; not in the reference)
    def fetch_match_indices(self, B):
        """Keypoint indices of the matches of the last batch / stream / pair list: (qidx i32[B, mm] into image 1's
        keypoints, tidx i32[B, mm] into image 2's), -1 past each pair's match count."""
        q = np.zeros((B, self.max_matches), np.int32); t = np.zeros_like(q)
        self._chk(self.lib.rpe_fetch_match_indices(self.h, B, _p(q), _p(t)))
        return q, t

    def scale_links(self, pair_a, pair_b, side, min_shared=8):
        """Relative scale of pairs of the last stream / pair list that share a frame (rpe_scale_links).  Link l joins
        pairs pair_a[l] and pair_b[l]; side[l] bit 0 / bit 1 = the shared frame is image 2 (else image 1) of pair_a /
        pair_b.  Returns (stats f64[L, 3], n_shared i32[L], code i32[L]): stats = lower quartile, median, upper quartile
        of d_a / d_b over the shared keypoints = baseline of pair_b in units of the baseline of pair_a; code = LINK_*
        (stats are zero unless LINK_OK).  The run's own results are not modified."""
        a, b, s = _i32(pair_a), _i32(pair_b), _i32(side)
        if not (a.size == b.size == s.size):
            raise ValueError(f"scale_links: pair_a, pair_b and side must have one length, got {(a.size, b.size, s.size)}")
        L = a.size
        stats = np.zeros((L, 3)); n = np.zeros(L, np.int32); code = np.zeros(L, np.int32)
        self._chk(self.lib.rpe_scale_links(self.h, L, _p(a), _p(b), _p(s), int(min_shared), _p(stats), _p(n), _p(code)))
        return stats, n, code

    def link_poses(self, pair_a, pair_b, side, iters=256, threshold_px=None, min_shared=8, refine_iters=10):
        """Pose of pair_b's other frame against the points pair_a triangulated, per link of the last stream / pair list
        (rpe_link_poses): P3P RANSAC over the keypoints of the shared frame, `iters` samples, all evaluated;
        threshold_px = the reprojection gate in pixels (None = the handle's ransac_threshold); refine_iters
        Levenberg-Marquardt iterations over the winner's inliers (0: the minimal pose).  Links as in scale_links.
        Returns (R f64[L, 3, 3], t f64[L, 3]: pair_b's relative pose, image 1 -> image 2, on pair_a's scale -- |t| is the
        baseline ratio; mask bool[L, mm] by pair_b's match index; counts i32[L, 2] = (shared keypoints, inliers);
        info i32[L, 4] = (LINKPOSE_* code, winning iteration, winning root, polish iterations / 0 none / -1 rejected);
        rms f64[L, 2] = reprojection rms in pixels of the minimal and of the returned pose).  Everything but the code and
        the shared count is zero unless LINKPOSE_OK.  The run's own results are not modified."""
        a, b, s = _i32(pair_a), _i32(pair_b), _i32(side)
        if not (a.size == b.size == s.size):
            raise ValueError(f"link_poses: pair_a, pair_b and side must have one length, got {(a.size, b.size, s.size)}")
        L = a.size
        R = np.zeros((L, 3, 3)); t = np.zeros((L, 3)); mask = np.zeros((L, self.max_matches), np.uint8)
        counts = np.zeros((L, 2), np.int32); info = np.zeros((L, 4), np.int32); rms = np.zeros((L, 2))
        thr = float(self.cfg.ransac_threshold if threshold_px is None else threshold_px)
        self._chk(self.lib.rpe_link_poses(self.h, L, _p(a), _p(b), _p(s), int(iters), thr, int(min_shared), int(refine_iters),
                                          _p(R), _p(t), _p(mask), _p(counts), _p(info), _p(rms)))
        return R, t, mask.astype(bool), counts, info, rms

    # ---- link bundles (rpe_link_bundles / rpe_bundle_three_view; not in the reference)
    def _bundle_outs(self, n):
        mm = self.max_matches
        return (np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, mm, 3)),
                np.zeros((n, mm), np.uint8), np.zeros((n, 2), np.int32), np.zeros((n, 4), np.int32), np.zeros((n, 2)))

    def link_bundles(self, pair_a, pair_b, side, R0, t0, threshold_px=None, min_shared=8, max_iters=10):
        """Bundle adjustment of the three views of every link of the last stream / pair list (rpe_link_bundles): the poses
        of pair_a and pair_b and the points both see, refined together on the reprojection error, the shared frame fixed
        and |t_a| = 1.  R0 f64[L, 3, 3], t0 f64[L, 3]: the start pose of pair_b on pair_a's scale, what link_poses
        returns (an all-zero R0 skips the link: BUNDLE_SKIPPED); threshold_px gates pair_b's observations under that pose
        (None = the handle's ransac_threshold).  Links as in scale_links.  Returns (R_a, t_a, R_b, t_b: the two pairs'
        poses in their own conventions, t_b on pair_a's scale; points f64[L, mm, 3] by pair_a's match index in its camera-1
        frame; views u8[L, mm]: 0 no point, 1 seen by pair_a's two frames, 3 by all three; counts i32[L, 2] = (points,
        points seen by all three); info i32[L, 4] = (BUNDLE_* code, iterations, accepted steps, 0); rms f64[L, 2] =
        reprojection rms in pixels before and after).  BUNDLE_REJECTED returns the input poses and points; the other codes
        but OK return zeros.  The run's own results are not modified."""
        a, b, s = _i32(pair_a), _i32(pair_b), _i32(side)
        if not (a.size == b.size == s.size):
            raise ValueError(f"link_bundles: pair_a, pair_b and side must have one length, got {(a.size, b.size, s.size)}")
        L = a.size
        R0 = None if R0 is None else np.ascontiguousarray(np.asarray(R0, np.float64).reshape(L, 9))
        t0 = None if t0 is None else np.ascontiguousarray(np.asarray(t0, np.float64).reshape(L, 3))
        outs = self._bundle_outs(L)
        thr = float(self.cfg.ransac_threshold if threshold_px is None else threshold_px)
        self._chk(self.lib.rpe_link_bundles(self.h, L, _p(a), _p(b), _p(s), _opt(R0), _opt(t0), thr, int(min_shared), int(max_iters),
                                            *map(_p, outs)))
        return outs

    def bundle_three_view(self, obs_s, obs_a, obs_c, has_c, X0, Ra0, ta0, Rc0, tc0, f_a, f_c, max_iters=10):
        """The bundle kernel on the caller's own tracks (rpe_bundle_three_view): B problems, problem p with obs_s[p], obs_a[p],
        obs_c[p] f64[n_p, 2] (normalised observations on the gauge view S and on A and C), has_c[p] bool[n_p], X0[p]
        f64[n_p, 3] (start points in S's frame) and start poses S -> A (|ta0| = 1) and S -> C; f_a, f_c scale the residuals
        to pixels.  Returns link_bundles' tuple in the solved form: (R_a, t_a, R_c, t_c, points by point number in S's
        frame, views, counts, info, rms).  Fewer than 6 points seen by C: BUNDLE_TOO_FEW."""
        B, mm = len(X0), self.max_matches
        n = np.array([len(x) for x in X0], np.int32)
        if n.max(initial=0) > mm:
            raise ValueError(f"bundle_three_view: more than max_matches = {mm} points in a problem")
        pad = lambda arrs, w, dt: np.stack([np.concatenate([np.asarray(x, dt).reshape(-1, w), np.zeros((mm - len(x), w), dt)]) for x in arrs])
        os_, oa, oc, x0 = pad(obs_s, 2, np.float64), pad(obs_a, 2, np.float64), pad(obs_c, 2, np.float64), pad(X0, 3, np.float64)
        hc = pad(has_c, 1, np.uint8)
        poses = [np.ascontiguousarray(np.asarray(v, np.float64).reshape(B, w)) for v, w in ((Ra0, 9), (ta0, 3), (Rc0, 9), (tc0, 3))]
        outs = self._bundle_outs(B)
        self._chk(self.lib.rpe_bundle_three_view(self.h, B, _p(n), _p(os_), _p(oa), _p(oc), _p(hc), _p(x0), *map(_p, poses),
                                                 float(f_a), float(f_c), int(max_iters), *map(_p, outs)))
        return outs

    # ---- multi-view tracks (rpe_build_tracks / rpe_tracks_from_matches; not in the reference)
    def _tracks(self, P, call):
        """call(counts, track_start, obs_frame, obs_kp, obs_xy, match_track) -> rc, over arrays sized by the bound; the
        dict of both track calls, trimmed to the counts"""
        n = P * self.max_matches
        counts = np.zeros(6, np.int32); ts = np.zeros(n + 1, np.int32)
        of = np.zeros(2 * n, np.int32); ok = np.zeros(2 * n, np.int32); xy = np.zeros((2 * n, 2), np.float32)
        mt = np.full((P, self.max_matches), -1, np.int32)
        self._chk(call(_p(counts), _p(ts), _p(of), _p(ok), _p(xy), _p(mt)))
        nt, no = int(counts[0]), int(counts[1])
        out = {'track_start': ts[:nt + 1].copy(), 'obs_frame': of[:no].copy(), 'obs_kp': ok[:no].copy(), 'obs_xy': xy[:no].copy(),
               'match_track': mt}
        out.update({k: int(v) for k, v in zip(TRACK_COUNTS, counts)})
        return out

    def build_tracks(self, use_pair=None, edge_rule=TRACK_EDGES_USABLE, min_len=2):
        """Feature tracks over all pairs of the last stream / pair list (rpe_build_tracks): the connected components of the
        match graph with at most one keypoint per frame and at least min_len of them.  A frame is its position in the
        stream or its store slot.  edge_rule: TRACK_EDGES_USABLE (RANSAC and cheirality inliers of OK pairs),
        TRACK_EDGES_RANSAC (RANSAC inliers: the rule for rotation-only pairs) or TRACK_EDGES_ALL (every match); use_pair
        bool[P] switches pairs off.  Returns a dict: 'track_start' i32[n_tracks + 1] (CSR), 'obs_frame' / 'obs_kp'
        i32[n_obs], 'obs_xy' f32[n_obs, 2] (pixels), 'match_track' i32[P, mm] (the track of each match, -1 none) and the
        counts 'n_tracks', 'n_obs', 'n_edges', 'dropped_conflict', 'dropped_short', 'n_frames_seen'.  Tracks are ordered by
        their first observation, observations by (frame, keypoint).  The run's own results are not modified.  A batch is
        refused (its pairs share no frame), except a batch of ONE pair, which is the stream of its two images (frames 0, 1)."""
        P = int(self.lib.rpe_last_run_pairs(self.h))        # the library writes its outputs by this count: sized by it
        up = None if use_pair is None else np.ascontiguousarray(np.asarray(use_pair).astype(bool), np.uint8).reshape(-1)
        if up is not None and up.size != P:
            raise ValueError(f"build_tracks: use_pair must have one entry per pair of the last run ({P}), got {up.size}")
        return self._tracks(P, lambda *o: self.lib.rpe_build_tracks(self.h, _opt(up), int(edge_rule), int(min_len), *o))

    def tracks_from_matches(self, frame1, frame2, qidx, tidx, n_frames, edge=None, pts1=None, pts2=None, min_len=2):
        """The track kernels on the caller's own matches (rpe_tracks_from_matches): pair p joins frames frame1[p] and
        frame2[p] of n_frames and has the matches (qidx[p][i], tidx[p][i]) -- ragged per-pair lists; edge[p] bool[n_p]
        (None: every match is an edge); pts1[p] / pts2[p] f32[n_p, 2] the matched pixels (None: 'obs_xy' is zero).
        Returns build_tracks' dict.  The last run stays fetchable."""
        f1, f2 = _i32(frame1), _i32(frame2)
        P, mm = f1.size, self.max_matches
        if not (f2.size == len(qidx) == len(tidx) == P) or any(x is not None and len(x) != P for x in (edge, pts1, pts2)):
            raise ValueError("tracks_from_matches: frame1, frame2 and the per-pair lists must have one length")
        m = np.array([len(x) for x in qidx], np.int32)
        if m.max(initial=0) > mm or any(len(t) != n for t, n in zip(tidx, m)):
            raise ValueError(f"tracks_from_matches: qidx[p] and tidx[p] must have one length of at most max_matches = {mm}")

        def pad(rows, w, dt):
            a = np.zeros((P, mm) + ((w,) if w else ()), dt)
            for p, r in enumerate(rows):
                a[p, :m[p]] = np.asarray(r, dt).reshape((m[p], w) if w else (m[p],))
            return a
        q, t = pad(qidx, 0, np.int32), pad(tidx, 0, np.int32)
        e = None if edge is None else pad(edge, 0, np.uint8)
        p1 = None if pts1 is None else pad(pts1, 2, np.float32)
        p2 = None if pts2 is None else pad(pts2, 2, np.float32)
        return self._tracks(P, lambda *o: self.lib.rpe_tracks_from_matches(
            self.h, P, int(n_frames), _p(f1), _p(f2), _p(m), _p(q), _p(t), _opt(e), _opt(p1), _opt(p2), int(min_len), *o))

    # ---- track points (rpe_triangulate_tracks; not in the reference)
    def triangulate_tracks(self, tracks, R_abs, T_abs, K=None, cameras=None, frame_group=None, threshold_px=2.0, min_views=2,
                           max_cos=1.0, max_iters=10):
        """One scene point per track from all its views (rpe_triangulate_tracks).  tracks: the dict build_tracks returns
        ('track_start', 'obs_frame' and 'obs_xy' are read); R_abs [F, 3, 3], T_abs [F, 3]: world-to-camera poses
        x = R X + T per frame, as geometry.chain_trajectory returns them; exactly one of K (one camera) and cameras (one
        Camera, or F of them); frame_group i32[F]: frames of one value >= 0 share a scale, negative = no pose, None = all
        in one group (geometry.frame_groups gives a chain's).  A track uses the views of its first group, is solved by a
        midpoint start and Levenberg-Marquardt, loses the views beyond threshold_px and is solved once more.  Returns a
        dict: 'points' f64[n, 3] in the frame of the poses, 'code' (TRACKPT_*), 'n_used', 'n_inliers', 'iterations'
        i32[n], 'rms' f64[n] (px, over the inliers), 'min_cos' f64[n] (smallest cosine between the rays of two inlier
        views; above max_cos the code is TRACKPT_LOW_PARALLAX), 'obs_flag' u8[n_obs] (0 not used, 1 inlier, 2 outlier),
        'obs_err' f64[n_obs] (px; -1 behind the camera).  The last run stays fetchable."""
        ts, of, xy, R, T, F, n, k, cams = _scene_args("triangulate_tracks", tracks, R_abs, T_abs, K, cameras)
        g = None if frame_group is None else _i32(frame_group)
        if g is not None and g.size != F:
            raise ValueError(f"triangulate_tracks: frame_group must have one entry per frame ({F}), got {g.size}")
        pts = np.zeros((n, 3)); info = np.zeros((n, 4), np.int32); rms = np.zeros(n); mc = np.zeros(n)
        flag = np.zeros(of.size, np.uint8); err = np.zeros(of.size)
        self._chk(self.lib.rpe_triangulate_tracks(self.h, n, _p(ts), _p(of), _p(xy), F, _p(R), _p(T), _opt(g), _opt(k), _opt(cams),
                                                  float(threshold_px), int(min_views), float(max_cos), int(max_iters),
                                                  _p(pts), _p(info), _p(rms), _p(mc), _p(flag), _p(err)))
        return {'points': pts, 'code': info[:, 0].copy(), 'n_used': info[:, 1].copy(), 'n_inliers': info[:, 2].copy(),
                'iterations': info[:, 3].copy(), 'rms': rms, 'min_cos': mc, 'obs_flag': flag, 'obs_err': err}

    # ---- window bundles (rpe_bundle_windows; not in the reference)
    def bundle_windows(self, tracks, points, R_abs, T_abs, windows, K=None, cameras=None, obs_use=None, point_use=None,
                       max_points=4096, min_obs=8, max_iters=10):
        """Bundle adjustment of windows of 2 .. 8 frames over a run's tracks (rpe_bundle_windows).  tracks: the dict
        build_tracks returns; points f64[n, 3]: a start point per track in the frame of the poses (triangulate_tracks'
        'points'); R_abs [F, 3, 3], T_abs [F, 3]: world-to-camera poses; windows: a list of lists of distinct frames, the
        first of each is its gauge; exactly one of K and cameras; obs_use u8[n_obs]: an observation is selected where the
        byte is 1 (triangulate_tracks' 'obs_flag' passes as it is), point_use u8[n]: a track is used where it is not 0;
        None selects all.  Each window is solved on its own from these inputs.  Returns a dict: 'R', 'T': lists, one
        [W, 3, 3] / [W, 3] array per window, in the caller's frame; 'points': a list of f64[n_w, 3]; 'point_track': a list
        of i32[n_w]; 'code' (WINDOW_*), 'views', 'n_points', 'n_obs', 'dropped', 'iterations', 'accepted', 'anchor'
        i32[n_win]; 'rms' f64[n_win, 2] (px, before and after).  For every code but WINDOW_OK the inputs come back.  The
        last run stays fetchable."""
        ts, of, xy, R, T, F, n, k, cams = _scene_args("bundle_windows", tracks, R_abs, T_abs, K, cameras)
        p0 = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
        if p0.shape[0] != n:
            raise ValueError("bundle_windows: points hold one row per track")
        ou = None if obs_use is None else np.ascontiguousarray(obs_use, np.uint8).reshape(-1)
        pu = None if point_use is None else np.ascontiguousarray(point_use, np.uint8).reshape(-1)
        if (ou is not None and ou.size != of.size) or (pu is not None and pu.size != n):
            raise ValueError("bundle_windows: obs_use has one byte per observation and point_use one per track")
        wl = [_i32(w) for w in windows]
        nw = len(wl)
        wstart = np.zeros(nw + 1, np.int32)
        wstart[1:] = np.cumsum([w.size for w in wl])
        wframe = _i32(np.concatenate(wl)) if nw else np.zeros(0, np.int32)
        mp, nwf = int(max_points), int(wstart[-1])
        slots = nw * max(mp, 0) if mp <= WINDOW_MAX_POINTS else 0
        Ro = np.zeros((nwf, 3, 3)); To = np.zeros((nwf, 3)); pts = np.zeros((slots, 3)); ptk = np.zeros(slots, np.int32)
        counts = np.zeros((nw, 4), np.int32); info = np.zeros((nw, 4), np.int32); rms = np.zeros((nw, 2))
        self._chk(self.lib.rpe_bundle_windows(self.h, n, _p(ts), _p(of), _p(xy), _p(p0), _opt(pu), _opt(ou), F, _p(R), _p(T), _opt(k),
                                              _opt(cams), nw, _p(wstart), _p(wframe), mp, int(min_obs), int(max_iters),
                                              _p(Ro), _p(To), _p(pts), _p(ptk), _p(counts), _p(info), _p(rms)))
        cnt = counts[:, 1]
        return {'R': [Ro[wstart[w]:wstart[w + 1]].copy() for w in range(nw)], 'T': [To[wstart[w]:wstart[w + 1]].copy() for w in range(nw)],
                'points': [pts[w * mp:w * mp + cnt[w]].copy() for w in range(nw)],
                'point_track': [ptk[w * mp:w * mp + cnt[w]].copy() for w in range(nw)],
                'code': info[:, 0].copy(), 'views': counts[:, 0].copy(), 'n_points': cnt.copy(), 'n_obs': counts[:, 2].copy(),
                'dropped': counts[:, 3].copy(), 'iterations': info[:, 1].copy(), 'accepted': info[:, 2].copy(),
                'anchor': info[:, 3].copy(), 'rms': rms}

    # ---- pose graphs (rpe_optimise_graphs; not in the reference)
    def optimise_graphs(self, R_abs, T_abs, graphs, edges, fixed=None, huber=0.0, max_iters=20, cg_iters=32, cg_tol=1e-3):
        """Pose-graph optimisation of a chain's poses over relative-pose edges (rpe_optimise_graphs; the rule is in
        include/rpe_amd.h, "pose graphs").  R_abs [F, 3, 3], T_abs [F, 3]: world-to-camera poses; graphs: a list of lists of
        distinct frames, the first of each is fixed; edges: one dict per graph of 'i', 'j' (frame indices), 'R' [E, 3, 3],
        't' [E, 3] (X_j = R X_i + t), 'w' [E, 2] (w_rot, w_trans) and 'kind' [E] (EDGE_METRIC / EDGE_DIRECTION) --
        geometry.chain_edges and loop_edges build them; fixed: None or one byte array per graph (or None), laid out like the
        graph's frames.  Each graph is solved on its own from these poses.  Returns a dict: 'R', 'T': lists, one [n, 3, 3] /
        [n, 3] array per graph; 'code' (GRAPH_*), 'frames', 'free', 'used_edges', 'unused_edges', 'iterations', 'accepted',
        'pcg_iterations' i32[n_graphs]; 'cost' f64[n_graphs, 2] (before and after); 'edge_chi': a list of f64[E, 2], the length
        of each used edge's rows before and after (0 for unused edges); 'edge_used': a list of u8[E].  For every code but
        GRAPH_OK the inputs come back.  The last run stays fetchable."""
        R = np.ascontiguousarray(np.asarray(R_abs, np.float64).reshape(-1, 9))
        T = np.ascontiguousarray(np.asarray(T_abs, np.float64).reshape(-1, 3))
        if T.shape[0] != R.shape[0]:
            raise ValueError("optimise_graphs: R_abs and T_abs hold one pose per frame")
        gl = [_i32(g) for g in graphs]
        ng = len(gl)
        if len(edges) != ng or (fixed is not None and len(fixed) != ng):
            raise ValueError("optimise_graphs: edges (and fixed) hold one entry per graph")
        gstart = np.zeros(ng + 1, np.int32); estart = np.zeros(ng + 1, np.int32)
        gstart[1:] = np.cumsum([g.size for g in gl])
        el = []
        for e in edges:
            i, j = _i32(e['i']), _i32(e['j'])
            n = i.size
            M = np.asarray(e['R'], np.float64).reshape(-1, 9); m = np.asarray(e['t'], np.float64).reshape(-1, 3)
            w = np.asarray(e['w'], np.float64).reshape(-1, 2); k = _i32(e['kind'])
            if not (j.size == M.shape[0] == m.shape[0] == w.shape[0] == k.size == n):
                raise ValueError("optimise_graphs: the arrays of a graph's edges hold one row per edge")
            el.append((i, j, M, m, w, k))
        estart[1:] = np.cumsum([e[0].size for e in el])
        cat = lambda k, dtype, shape: np.ascontiguousarray(np.concatenate([e[k] for e in el]) if el else np.zeros(shape, dtype), dtype)
        gframe = np.ascontiguousarray(np.concatenate(gl) if ng else np.zeros(0, np.int32), np.int32)
        ei, ej, eM, em, ew, ek = (cat(0, np.int32, 0), cat(1, np.int32, 0), cat(2, np.float64, (0, 9)), cat(3, np.float64, (0, 3)),
                                  cat(4, np.float64, (0, 2)), cat(5, np.int32, 0))
        fx = None
        if fixed is not None:
            fx = np.zeros(gframe.size, np.uint8)
            for g, f in enumerate(fixed):
                if f is not None:
                    f = np.asarray(f).reshape(-1)
                    if f.size != gl[g].size:
                        raise ValueError("optimise_graphs: fixed holds one byte per frame of its graph")
                    fx[gstart[g]:gstart[g + 1]] = f != 0
        nf, ne = int(gstart[-1]), int(estart[-1])
        Ro = np.zeros((nf, 3, 3)); To = np.zeros((nf, 3)); counts = np.zeros((ng, 4), np.int32); info = np.zeros((ng, 4), np.int32)
        cost = np.zeros((ng, 2)); chi = np.zeros((ne, 2)); used = np.zeros(ne, np.uint8)
        self._chk(self.lib.rpe_optimise_graphs(self.h, R.shape[0], _p(R), _p(T), ng, _p(gstart), _p(gframe), _opt(fx), _p(estart),
                                               _p(ei), _p(ej), _p(eM), _p(em), _p(ew), _p(ek), float(huber), int(max_iters),
                                               int(cg_iters), float(cg_tol), _p(Ro), _p(To), _p(counts), _p(info), _p(cost),
                                               _p(chi), _p(used)))
        per_g = lambda a: [a[gstart[g]:gstart[g + 1]].copy() for g in range(ng)]
        per_e = lambda a: [a[estart[g]:estart[g + 1]].copy() for g in range(ng)]
        return {'R': per_g(Ro), 'T': per_g(To), 'code': info[:, 0].copy(), 'iterations': info[:, 1].copy(),
                'accepted': info[:, 2].copy(), 'pcg_iterations': info[:, 3].copy(), 'frames': counts[:, 0].copy(),
                'free': counts[:, 1].copy(), 'used_edges': counts[:, 2].copy(), 'unused_edges': counts[:, 3].copy(),
                'cost': cost, 'edge_chi': per_e(chi), 'edge_used': per_e(used)}

    # ---- guided matching (rpe_guided_matches / rpe_match_hamming_guided; not in the reference)
    def _poses(self, B, R, t):
        if (R is None) != (t is None):
            raise ValueError("guided matching: R and t must both be given or both be None")
        if R is None:
            return None, None
        return (np.ascontiguousarray(np.asarray(R, np.float64).reshape(B, 9)),
                np.ascontiguousarray(np.asarray(t, np.float64).reshape(B, 3)))

    def _match_outs(self, B, dist_dtype=np.int32):
        """qidx, tidx, dist [B, mm] and n_matches [B]"""
        mm = self.max_matches
        return np.zeros((B, mm), np.int32), np.zeros((B, mm), np.int32), np.zeros((B, mm), dist_dtype), np.zeros(B, np.int32)

    def _pack_features(self, rows, n, tail, dtype):
        """per pair the first n[i] rows of rows[i], packed to [B, kcap, *tail]"""
        out = np.zeros((len(n), self.kcap) + tail, dtype)
        for i in range(len(n)):
            out[i, :n[i]] = rows[i][:n[i]]
        return out

    def guided_matches(self, B, R=None, t=None, gate_px=None, max_distance=256):
        """Matches of the last batch / stream / pair list again under the epipolar gate of a pose (rpe_guided_matches):
        the mutual nearest neighbour among the keypoint pairs within gate_px (Sampson, pixels; None = the handle's
        ransac_threshold) of the pose and max_distance in Hamming distance.  R, t None: the run's own poses (pairs whose
        status is not OK get no matches); otherwise R[B,3,3], t[B,3] to gate with, every pair matched.  Returns
        (qidx, tidx, dist i32[B, mm], pts1, pts2 f32[B, mm, 2], n_matches i32[B]); -1 / zero past each pair's count.  The
        run's own results are not modified."""
        Rc, tc = self._poses(B, R, t)
        q, ti, d, nm = self._match_outs(B)
        p1 = np.zeros((B, self.max_matches, 2), np.float32); p2 = np.zeros_like(p1)
        gate = float(self.cfg.ransac_threshold if gate_px is None else gate_px)
        self._chk(self.lib.rpe_guided_matches(self.h, B, _opt(Rc), _opt(tc), gate, int(max_distance),
                                              _p(q), _p(ti), _p(d), _p(p1), _p(p2), _p(nm)))
        return q, ti, d, p1, p2, nm

    def match_hamming_guided(self, desc1, pts1, n1, desc2, pts2, n2, K, R, t, gate_px=None, max_distance=256):
        """Stage form of guided_matches, the sibling of match_hamming: per pair the caller's descriptors (n, 32) u8 and
        keypoint pixels (n, 2) f32 of both images, one K, the poses R[B,3,3], t[B,3].  Returns (qidx, tidx, dist,
        n_matches)."""
        B = len(n1)
        d1 = self._pack_features(desc1, n1, (32,), np.uint8); d2 = self._pack_features(desc2, n2, (32,), np.uint8)
        p1 = self._pack_features(pts1, n1, (2,), np.float32); p2 = self._pack_features(pts2, n2, (2,), np.float32)
        n1, n2, K = _i32(n1), _i32(n2), _f64(K)
        Rc, tc = self._poses(B, R, t)
        q, ti, d, nm = self._match_outs(B)
        gate = float(self.cfg.ransac_threshold if gate_px is None else gate_px)
        self._chk(self.lib.rpe_match_hamming_guided(self.h, _p(d1), _p(p1), _p(n1), _p(d2), _p(p2), _p(n2), B, _p(K),
                                                    _opt(Rc), _opt(tc), gate, int(max_distance), _p(q), _p(ti), _p(d), _p(nm)))
        return q, ti, d, nm

    # the same for NORM_L2 handles (rpe_guided_matches_l2 / rpe_match_l2_guided): f32 distances, a float bound
    def guided_matches_l2(self, B, R=None, t=None, gate_px=None, max_distance=None):
        """guided_matches for an L2 handle (SIFT, or ORB bytes under NORM_L2; rpe_guided_matches_l2): dist is the
        matcher's f32 distance, max_distance a float bound on it (None: no bound).  Returns (qidx, tidx i32[B, mm],
        dist f32[B, mm], pts1, pts2 f32[B, mm, 2], n_matches i32[B]); past each pair's count -1 / zero and, in dist,
        all-ones bits (a NaN)."""
        Rc, tc = self._poses(B, R, t)
        q, ti, d, nm = self._match_outs(B, np.float32)
        p1 = np.zeros((B, self.max_matches, 2), np.float32); p2 = np.zeros_like(p1)
        gate = float(self.cfg.ransac_threshold if gate_px is None else gate_px)
        bound = float("inf") if max_distance is None else float(max_distance)
        self._chk(self.lib.rpe_guided_matches_l2(self.h, B, _opt(Rc), _opt(tc), gate, bound,
                                                 _p(q), _p(ti), _p(d), _p(p1), _p(p2), _p(nm)))
        return q, ti, d, p1, p2, nm

    def match_l2_guided(self, desc1, pts1, n1, desc2, pts2, n2, K, R, t, gate_px=None, max_distance=None):
        """Stage form of guided_matches_l2, the sibling of match_l2: per pair the caller's byte-valued descriptors
        (n, desc_dim) and keypoint pixels (n, 2) f32 of both images, one K, the poses R[B,3,3], t[B,3].  Returns
        (qidx, tidx, dist f32, n_matches)."""
        B = len(n1)
        d1 = self._pack_features(desc1, n1, (self.desc_dim,), np.float32); d2 = self._pack_features(desc2, n2, (self.desc_dim,), np.float32)
        p1 = self._pack_features(pts1, n1, (2,), np.float32); p2 = self._pack_features(pts2, n2, (2,), np.float32)
        n1, n2, K = _i32(n1), _i32(n2), _f64(K)
        Rc, tc = self._poses(B, R, t)
        q, ti, d, nm = self._match_outs(B, np.float32)
        gate = float(self.cfg.ransac_threshold if gate_px is None else gate_px)
        bound = float("inf") if max_distance is None else float(max_distance)
        self._chk(self.lib.rpe_match_l2_guided(self.h, _p(d1), _p(p1), _p(n1), _p(d2), _p(p2), _p(n2), B, _p(K),
                                               _opt(Rc), _opt(tc), gate, bound, _p(q), _p(ti), _p(d), _p(nm)))
        return q, ti, d, nm

    # ---- homography / rotation-only (rpe_pair_homographies / rpe_find_homography; not in the reference)
    def _homography_outs(self, B):
        return (np.zeros((B, 3, 3)), np.zeros((B, 3, 3)), np.zeros((B, self.max_matches), np.uint8),
                np.zeros((B, 3), np.int32), np.zeros((B, 4), np.int32))

    def pair_homographies(self, B, iters=256, threshold_px=None):
        """A homography by RANSAC over the matches of each of the first B pairs of the last batch / stream / pair list
        (rpe_pair_homographies), the rotation fitted to its inliers, and the inlier counts of the three models.
        `iters` samples, all evaluated; threshold_px = the transfer gate in pixels (None = the handle's
        ransac_threshold).  Returns (H f64[B, 3, 3] in normalised coordinates, unit norm; R_rot f64[B, 3, 3];
        mask bool[B, mm], H's inliers; counts i32[B, 3] = (n_H, n_rot, n_E); info i32[B, 4] = (HOMOGRAPHY_* code, winning
        iteration, valid models, 0)).  The run's own results are not modified."""
        H, R, mask, counts, info = self._homography_outs(B)
        thr = float(self.cfg.ransac_threshold if threshold_px is None else threshold_px)
        self._chk(self.lib.rpe_pair_homographies(self.h, B, int(iters), thr, _p(H), _p(R), _p(mask), _p(counts), _p(info)))
        return H, R, mask.astype(bool), counts, info

    def find_homography(self, pts1, pts2, K, iters=256, threshold_px=None):
        """Stage form of pair_homographies, the sibling of find_essential: per pair the caller's matched pixels (n, 2)
        f32 of both images, one K.  Same outputs; counts[:, 2] (n_E) is -1: no essential RANSAC runs."""
        p1, p2, m = self._pack_points(pts1, pts2)
        B = len(m); K = _f64(K)
        H, R, mask, counts, info = self._homography_outs(B)
        thr = float(self.cfg.ransac_threshold if threshold_px is None else threshold_px)
        self._chk(self.lib.rpe_find_homography(self.h, _p(p1), _p(p2), _p(m), B, _p(K), int(iters), thr,
                                               _p(H), _p(R), _p(mask), _p(counts), _p(info)))
        return H, R, mask.astype(bool), counts, info

    # ---- frame store (rpe_frames_* / rpe_enqueue_pairs; not in the reference)
    def frames_reserve(self, n_slots):
        """Create / resize / free (0) the store of per-frame features; slots below the new size are kept."""
        self._chk(self.lib.rpe_frames_reserve(self.h, int(n_slots)))

    def frames_capacity(self):
        return int(self.lib.rpe_frames_capacity(self.h))

    def frames_put(self, frames, slots):
        """Extract frames [n, H, W] (host) once and keep their features in the store slots `slots` (n distinct ints)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        slots = _i32(slots)
        n = frames.shape[0]
        assert frames.shape == (n, self.height, self.width) and slots.size == n, (frames.shape, slots.shape)
        self._chk(self.lib.rpe_frames_put(self.h, _p(frames), n, _p(slots)))

    def frames_put_device(self, d_frames, n, slots):
        """Same, frames resident in HBM; asynchronous (the frames must stay valid until the next synchronising call)."""
        slots = _i32(slots)
        assert slots.size == n
        self._chk(self.lib.rpe_frames_put_device(self.h, d_frames, int(n), _p(slots)))

    def frames_info(self, slots):
        """(keypoint counts, OVF_* flags) of the slots; count -1 = never filled."""
        slots = _i32(slots)
        cnt = np.zeros(slots.size, np.int32); fl = np.zeros(slots.size, np.uint32)
        self._chk(self.lib.rpe_frames_info(self.h, slots.size, _p(slots), _p(cnt), _p(fl)))
        return cnt, fl

    def enqueue_pairs(self, slot1, slot2, K):
        s1, s2 = _slot_pairs(slot1, slot2)
        K = _f64(K)
        self._chk(self.lib.rpe_enqueue_pairs(self.h, _p(s1), _p(s2), s1.size, _p(K)))

    def estimate_pairs(self, slot1, slot2, K):
        """Poses of the pairs (slot1[p], slot2[p]) of stored frames: the batch's match / RANSAC / pose kernels, no
        extraction.  Returns R, t, inliers, n_matches, status like estimate_batch; the list is 'the last batch' of
        fetch_structure / refine_poses / fetch_overflow / fetch_matched_points afterwards."""
        s1, s2 = _slot_pairs(slot1, slot2)
        K = _f64(K)
        return self._estimate(self.lib.rpe_estimate_pairs, s1.size, _p(s1), _p(s2), s1.size, _p(K))

    # ---- pair proposals (rpe_frames_similar / rpe_similarity_hamming; not in the reference)
    def _similar(self, call, q, t, step, max_distance, q_time, t_time, exclude, min_score, k, want_scores):
        """the shared tail of the two forms: {"scores" [nq, nt] or None, "cand" / "cand_score" [nq, k] and "n_cand" [nq], or
        None without candidates (k = 0)}.  cand holds POSITIONS in the target list, -1 past a row's count."""
        q, t = _i32(q), _i32(t)
        q_time = None if q_time is None else _i32(q_time)
        t_time = None if t_time is None else _i32(t_time)
        assert (q_time is None or q_time.size == q.size) and (t_time is None or t_time.size == t.size)
        k = int(k)
        scores = np.zeros((q.size, t.size), np.int32) if want_scores else None
        cand = cscore = ncand = None
        if k > 0:
            cand = np.full((q.size, k), -1, np.int32); cscore = np.full((q.size, k), -1, np.int32); ncand = np.zeros(q.size, np.int32)
        self._chk(call(q.size, _p(q), t.size, _p(t), int(step), int(max_distance), _opt(q_time), _opt(t_time), int(exclude), int(min_score), k,
                       _opt(scores), _opt(cand), _opt(cscore), _opt(ncand)))
        return {"scores": scores, "cand": cand, "cand_score": cscore, "n_cand": ncand}

    def frames_similar(self, q_slots, t_slots, step=1, max_distance=48, q_time=None, t_time=None, exclude=-1, min_score=0, k=0,
                       want_scores=True):
        """Similarity of stored frames: scores[r, c] = crossCheck matches within max_distance between every step-th
        descriptor of slot q_slots[r] and of slot t_slots[c]; with k > 0 the k best eligible columns per row (slots
        differ, |q_time - t_time| > exclude when exclude >= 0, score >= min_score; times default to the slot numbers)."""
        return self._similar(lambda *a: self.lib.rpe_frames_similar(self.h, *a), q_slots, t_slots, step, max_distance, q_time, t_time,
                             exclude, min_score, k, want_scores)

    def similarity_hamming(self, desc, n, q_idx, t_idx, step=1, max_distance=48, q_time=None, t_time=None, exclude=-1, min_score=0, k=0,
                           want_scores=True):
        """The stage form: desc is a list of F uint8 [n_f, 32] descriptor arrays (or one [F, kcap, 32] array with counts n);
        q_idx / t_idx index the frames."""
        if n is None:
            n = np.array([len(d) for d in desc], np.int32)
            desc = self._pack_features(desc, n, (32,), np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8); n = _i32(n)
        assert desc.shape == (n.size, self.kcap, 32), desc.shape
        return self._similar(lambda *a: self.lib.rpe_similarity_hamming(self.h, _p(desc), _p(n), n.size, *a), q_idx, t_idx, step, max_distance,
                             q_time, t_time, exclude, min_score, k, want_scores)

    # ---- camera models (rpe_*_cameras; not in the reference): one Camera, or one per frame
    def frames_set_cameras(self, slots, cameras):
        """Cameras of the store slots `slots`; a slot keeps its camera until it is given another."""
        slots = _i32(slots)
        rec = camera_records(cameras, slots.size)
        self._chk(self.lib.rpe_frames_set_cameras(self.h, slots.size, _p(slots), _p(rec)))

    def enqueue_pairs_cameras(self, slot1, slot2):
        s1, s2 = _slot_pairs(slot1, slot2)
        self._chk(self.lib.rpe_enqueue_pairs_cameras(self.h, _p(s1), _p(s2), s1.size))

    def estimate_pairs_cameras(self, slot1, slot2):
        """estimate_pairs with every pair on the cameras of its two slots (frames_set_cameras)."""
        s1, s2 = _slot_pairs(slot1, slot2)
        return self._estimate(self.lib.rpe_estimate_pairs_cameras, s1.size, _p(s1), _p(s2), s1.size)

    def enqueue_batch_cameras_device(self, d_imgs1, d_imgs2, B, cameras1, cameras2):
        c1 = camera_records(cameras1, B); c2 = camera_records(cameras2, B)
        self._chk(self.lib.rpe_enqueue_batch_cameras_device(self.h, d_imgs1, d_imgs2, B, _p(c1), _p(c2)))

    def estimate_batch_cameras_device(self, d_imgs1, d_imgs2, B, cameras1, cameras2):
        c1 = camera_records(cameras1, B); c2 = camera_records(cameras2, B)
        return self._estimate(self.lib.rpe_estimate_batch_cameras_device, B, d_imgs1, d_imgs2, B, _p(c1), _p(c2))

    def estimate_batch_cameras(self, imgs1, imgs2, cameras1, cameras2):
        """estimate_batch with a camera per image (cameras1[p] for imgs1[p], cameras2[p] for imgs2[p])."""
        imgs1, imgs2, B = self._image_pair(imgs1, imgs2)
        c1 = camera_records(cameras1, B); c2 = camera_records(cameras2, B)
        return self._estimate(self.lib.rpe_estimate_batch_cameras, B, _p(imgs1), _p(imgs2), B, _p(c1), _p(c2))

    def undistort_points(self, pts, camera):
        """(n, 2) f32 pixels -> (n, 2) f64 normalised, undistorted coordinates: what the geometry stages of the camera
        path work on."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        rec = camera_records(camera, 1)
        out = np.zeros((pts.shape[0], 2))
        self._chk(self.lib.rpe_undistort_points(self.h, _p(pts), pts.shape[0], _p(rec), _p(out)))
        return out

    def find_essential_cameras(self, pts1, pts2, cameras1, cameras2):
        return self._find_essential(self.lib.rpe_find_essential_cameras, pts1, pts2, cameras1, cameras2)

    def recover_pose_cameras(self, E, pts1, pts2, cameras1, cameras2):
        return self._recover_pose(self.lib.rpe_recover_pose_cameras, E, pts1, pts2, cameras1, cameras2)

    def refine_pose_points_cameras(self, R0, t0, pts1, pts2, masks, cameras1, cameras2, max_iters=10):
        return self._refine_pose_points(self.lib.rpe_refine_pose_points_cameras, R0, t0, pts1, pts2, masks, max_iters, cameras1, cameras2)

    # ---- stage API
    def orb_detect_and_compute(self, imgs):
        imgs = np.ascontiguousarray(imgs, np.uint8)
        n = imgs.shape[0]
        kps = np.zeros((n, self.kcap), KP_DTYPE); desc = np.zeros((n, self.kcap, 32), np.uint8)
        cnt = np.zeros(n, np.int32)
        self._chk(self.lib.rpe_orb_detect_and_compute(self.h, _p(imgs), n, _p(kps), _p(desc), _p(cnt)))
        return kps, desc, cnt

    def orb_debug_fetch(self, index, which):
        out = np.zeros(self.lib.rpe_orb_pyramid_pixels(self.h), np.uint8)
        self._chk(self.lib.rpe_orb_debug_fetch(self.h, index, which, _p(out)))
        return out

    def orb_debug_retain(self, kind, stl, lists, n_points, cap=None):
        """retainBest(n_points[i]) on every list (kind 0: uint32 FAST entries, 1: uint64 Harris entries) in one launch of
        the selection kernels' routine; returns the lists as left behind (whole, by their old lengths) and the new sizes"""
        dt = np.uint64 if kind else np.uint32
        n = len(lists)
        cap = max(1, max(len(a) for a in lists)) if cap is None else cap
        ln = _i32([len(a) for a in lists]); npts = _i32(n_points); out_len = np.zeros(n, np.int32)
        buf = np.zeros((n, max(cap, int(ln.max()))), dt)
        for i, a in enumerate(lists):
            buf[i, :len(a)] = a
        self._chk(self.lib.rpe_orb_debug_retain(self.h, kind, stl, _p(buf), _p(ln), _p(npts), n, cap, _p(out_len)))
        return [buf[i, :ln[i]].copy() for i in range(n)], out_len

    def sift_detect_and_compute(self, imgs):
        imgs = np.ascontiguousarray(imgs, np.uint8)
        n = imgs.shape[0]
        kps = np.zeros((n, self.kcap), SIFT_KP_DTYPE); desc = np.zeros((n, self.kcap, 128), np.float32)
        cnt = np.zeros(n, np.int32)
        self._chk(self.lib.rpe_sift_detect_and_compute(self.h, _p(imgs), n, _p(kps), _p(desc), _p(cnt)))
        return kps, desc, cnt

    def sift_debug_gauss(self, index):
        n = self.lib.rpe_sift_debug_gauss(self.h, index, None)
        out = np.zeros(n, np.float32)
        self.lib.rpe_sift_debug_gauss(self.h, index, _p(out))
        return out

    def _match(self, fn, desc1, n1, desc2, n2, dim, dtype):
        """the stage matchers: descriptors [n, dim] of `dtype` per pair and image; distances come back in that norm's type"""
        B = len(n1)
        d1 = self._pack_features(desc1, n1, (dim,), dtype); d2 = self._pack_features(desc2, n2, (dim,), dtype)
        n1, n2 = _i32(n1), _i32(n2)
        q, t, d, nm = self._match_outs(B, np.float32 if dtype == np.float32 else np.int32)
        self._chk(fn(self.h, _p(d1), _p(n1), _p(d2), _p(n2), B, _p(q), _p(t), _p(d), _p(nm)))
        return q, t, d, nm

    def match_l2(self, desc1, n1, desc2, n2):
        return self._match(self.lib.rpe_match_l2, desc1, n1, desc2, n2, self.desc_dim, np.float32)

    def match_hamming(self, desc1, n1, desc2, n2):
        return self._match(self.lib.rpe_match_hamming, desc1, n1, desc2, n2, 32, np.uint8)

    def _pack_points(self, pts1, pts2):
        B = len(pts1)
        mm = self.max_matches
        p1 = np.zeros((B, mm, 2), np.float32); p2 = np.zeros_like(p1); m = np.zeros(B, np.int32)
        for i in range(B):
            m[i] = len(pts1[i]); p1[i, :m[i]] = pts1[i]; p2[i, :m[i]] = pts2[i]
        return p1, p2, m

    # The geometry stages take one K (rpe_*) or the cameras of the two sides (rpe_*_cameras): `cam` is (K,) or
    # (cameras1, cameras2), and the arrays it becomes sit where the C signatures have K / cam1, cam2
    def _camera_args(self, B, *cam):
        return (_f64(cam[0]),) if len(cam) == 1 else (camera_records(cam[0], B), camera_records(cam[1], B))

    def _find_essential(self, fn, pts1, pts2, *cam):
        p1, p2, m = self._pack_points(pts1, pts2)
        B = len(m)
        cam = self._camera_args(B, *cam)
        E = np.zeros((B, 3, 3)); mask = np.zeros((B, self.max_matches), np.uint8)
        found = np.zeros(B, np.int32); info = np.zeros((B, 4), np.int32)
        self._chk(fn(self.h, _p(p1), _p(p2), _p(m), B, *map(_p, cam), _p(E), _p(mask), _p(found), _p(info)))
        return E, mask, found, info

    def _recover_pose(self, fn, E, pts1, pts2, *cam):
        p1, p2, m = self._pack_points(pts1, pts2)
        B = len(m); E = _f64(E)
        cam = self._camera_args(B, *cam)
        R, t, inl = self._outs(B)[:3]
        self._chk(fn(self.h, _p(E), _p(p1), _p(p2), _p(m), B, *map(_p, cam), _p(R), _p(t), _p(inl)))
        return R, t, inl

    def _refine_pose_points(self, fn, R0, t0, pts1, pts2, masks, max_iters, *cam):
        p1, p2, m = self._pack_points(pts1, pts2)
        B = len(m)
        cam = self._camera_args(B, *cam)
        R0 = np.ascontiguousarray(np.asarray(R0, np.float64).reshape(B, 9)); t0 = np.ascontiguousarray(np.asarray(t0, np.float64).reshape(B, 3))
        mk = np.zeros((B, self.max_matches), np.uint8)
        for i in range(B):
            mk[i, :m[i]] = np.asarray(masks[i]).astype(bool)[:m[i]]
        outs = self._refine_outs(B)
        self._chk(fn(self.h, _p(R0), _p(t0), _p(p1), _p(p2), _p(mk), _p(m), B, *map(_p, cam), max_iters, *map(_p, outs)))
        return outs

    def find_essential(self, pts1, pts2, K):
        return self._find_essential(self.lib.rpe_find_essential, pts1, pts2, K)

    def recover_pose(self, E, pts1, pts2, K):
        return self._recover_pose(self.lib.rpe_recover_pose, E, pts1, pts2, K)

    def refine_pose_points(self, R0, t0, pts1, pts2, masks, K, max_iters=10):
        """Stage form of refine_poses: per pair the start (R0, t0), the matched points and a mask (one entry per match)
        selecting the residuals.  Same outputs as refine_poses."""
        return self._refine_pose_points(self.lib.rpe_refine_pose_points, R0, t0, pts1, pts2, masks, max_iters, K)

    # ---- roofline calibration
    def calibrate_valu(self, kind, waves_per_simd):
        """(instruction name, measured wave-instructions per second of the whole chip)"""
        v = C.c_double(0.)
        self._chk(self.lib.rpe_calibrate_valu(self.h, kind, waves_per_simd, C.byref(v)))
        return self.lib.rpe_calibrate_valu_name(kind).decode(), float(v.value)

    def calibrate_hbm(self):
        v = C.c_double(0.)
        self._chk(self.lib.rpe_calibrate_hbm(self.h, C.byref(v)))
        return float(v.value)

    # ---- profiling
    def set_profiling(self, on):
        self._chk(self.lib.rpe_set_profiling(self.h, 1 if on else 0))

    def stage_ms(self):
        ms = np.zeros(STAGE_COUNT, np.float32)
        self._chk(self.lib.rpe_get_stage_ms(self.h, _p(ms)))
        return {self.lib.rpe_stage_name(i).decode(): float(ms[i]) for i in range(STAGE_COUNT)}
