"""Drop-in PoseEstimator backed by librpe_amd.so (HIP kernels on MI355X).

Mirrors reference src/core/pose_estimator.py: same constructor signature and
defaults (:19-32), estimate(img1, img2, R_prev=None) -> (R, t) (:487-569),
estimate_with_debug(...) -> dict with the reference's keys (:571-688, dict
:624-633), same exception types and messages (:96, :129, :508-509, :514-515,
:529-530).  Added: estimate_batch() for many pairs per call; estimate_with_structure() / last_structure() for the
per-match inlier masks and triangulated points; `dist_coeffs` / Camera for lens distortion and per-frame cameras
(the camera path: matched points are undistorted on the GPU before the geometry stages); last_homographies() /
estimate_with_geometry() for the homography, the rotation-only fit and which model a pair obeys.

Scope: the feature -> match -> essential -> pose path on the GPU: ORB or SIFT features, Hamming or L2 matcher
(every combination cv2 can run: ORB + Hamming, ORB + L2, SIFT + L2; SIFT + Hamming constructs, as in the reference,
and fails at the first estimate with cv2's batchDistance message, where the reference's match() fails).  Added, opt-in
and NOT in the reference: `ratio` = Lowe ratio test instead of crossCheck; `keypoint_order` = which cv2 build's
keypoint order to reproduce ("libstdc++": the Linux wheels, default; "msvc": the Windows wheels).  VP refinement
(:160-481, :536-567) is the reference's CPU post-step on R; it is applied exactly where the
reference applies it -- `use_vp_refinement` set and `R_prev` given -- by vp_refinement.py on top of the
library's LSD restatement (host code, as in the reference).
"""
import numpy as np

from . import _capi, geometry, vp_refinement


def plan_pairs(n_frames, n_pairs, max_batch):
    """Chunk plan of PoseEstimator.estimate_pairs, a pure function: (put_chunks, pair_chunks), lists of (start, stop).
    Every frame is put exactly once, frame f into store slot f, in chunks of at most 2*max_batch frames (the library's
    image workspace); the pair list then runs in list order in chunks of at most max_batch pairs."""
    if n_frames < 1 or n_pairs < 0 or max_batch < 1:
        raise ValueError(f"plan_pairs: need n_frames >= 1, n_pairs >= 0, max_batch >= 1, got {(n_frames, n_pairs, max_batch)}")
    puts = [(a, min(a + 2 * max_batch, n_frames)) for a in range(0, n_frames, 2 * max_batch)]
    runs = [(a, min(a + max_batch, n_pairs)) for a in range(0, n_pairs, max_batch)]
    return puts, runs


def _check_pairs(pairs, n_slots, what):
    """[P, 2] integer array with every index inside [0, n_slots); ValueError otherwise, before any device call"""
    a = np.asarray(pairs)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"pairs: expected an integer array of shape [P, 2] with P >= 1, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValueError(f"pairs: expected integers, got dtype {a.dtype}")
    if (a < 0).any() or (a >= n_slots).any():
        raise ValueError(f"pairs: {what} index outside [0, {n_slots})")
    return np.ascontiguousarray(a, np.int32)


class FrameStore:
    """Per-frame features resident on the GPU for online use (PoseEstimator.frame_store; not in the reference): put a
    frame into a numbered slot once, then estimate any list of (slot, slot) pairs without extracting again.  The slot
    numbers are the caller's: a ring of the last k frames is `slot = frame_index % k`.  The store lives on the
    estimator's engine for the frames' image size; a call that makes the estimator build a larger engine
    (estimate_batch with more pairs than max_batch) ends it."""

    def __init__(self, estimator, capacity):
        if int(capacity) < 1:
            raise ValueError("FrameStore: capacity must be >= 1")
        self._est, self.capacity, self._eng = estimator, int(capacity), None
        self._has_cam = np.zeros(self.capacity, bool)      # slots that were given a camera

    def _engine(self, shape):
        if self._eng is None:
            eng = self._est._engine(shape[0], shape[1], 1)
            if getattr(eng, "_store_owner", None) is not None:
                raise _capi.RpeError("the engine of this image size already serves a frame store: close it first")
            eng.frames_reserve(self.capacity)
            eng._store_owner = self
            self._eng = eng
        if self._eng.h is None or getattr(self._eng, "_store_owner", None) is not self:
            raise _capi.RpeError("FrameStore: its engine is gone (closed, or replaced by a larger one)")
        if (self._eng.height, self._eng.width) != tuple(shape):
            raise ValueError(f"FrameStore: frames are {self._eng.height} x {self._eng.width}, got {tuple(shape)}")
        return self._eng

    def put(self, slot, image, camera=None):
        self.put_many([slot], self._est._gray(image)[None], None if camera is None else [camera])

    def put_many(self, slots, images, cameras=None):
        """cameras: None (the slots keep whatever camera they have; with none they run on the estimator's K), one Camera
        for all the frames, or one per frame.  An estimator built with dist_coeffs gives its camera to every frame put
        without one."""
        slots = np.asarray(slots)
        images = np.asarray(images)
        if cameras is None and self._est._camera is not None:
            cameras = self._est._camera
        if cameras is not None:
            cameras = _capi.camera_records(cameras, slots.size)         # ValueError before any device call
        if slots.ndim != 1 or slots.dtype.kind not in "iu" or images.ndim != 3 or images.dtype != np.uint8 or images.shape[0] != slots.size:
            raise ValueError("put_many: expected n integer slots and n uint8 grayscale images [n, H, W]")
        if slots.size == 0 or (slots < 0).any() or (slots >= self.capacity).any() or np.unique(slots).size != slots.size:
            raise ValueError(f"put_many: slots must be distinct and inside [0, {self.capacity})")
        eng = self._engine(images.shape[1:])
        step = 2 * eng.max_batch
        for a in range(0, slots.size, step):
            eng.frames_put(images[a:a + step], slots[a:a + step])
        if cameras is not None:
            eng.frames_set_cameras(slots, cameras)
            self._has_cam[slots] = True

    def estimate(self, pairs):
        """(R[P,3,3], t[P,3,1], inliers[P], n_matches[P], status[P]) of the slot pairs [P, 2]; a failing pair never
        aborts the list.  last_structure / last_refined / last_overflow of the estimator describe the last chunk of
        at most max_batch pairs.  The slots' own cameras are used when every slot the list names has one, the
        estimator's K when none has; a list that mixes the two is a ValueError."""
        pairs = _check_pairs(pairs, self.capacity, "slot")
        named = self._has_cam[np.unique(pairs)]
        if named.any() and not named.all():
            raise ValueError("FrameStore.estimate: the pair list mixes slots with a camera and slots without one")
        if self._eng is None:
            raise _capi.RpeError("FrameStore: nothing has been put yet")
        eng = self._engine((self._eng.height, self._eng.width))
        return self._est._run_pair_list(eng, pairs, cameras=bool(named.all()))

    def _filled(self):
        if self._eng is None:
            raise _capi.RpeError("FrameStore: nothing has been put yet")
        cnt, _ = self.info(np.arange(self.capacity))
        return np.nonzero(cnt >= 0)[0].astype(np.int32)

    def _slot_list(self, slots, what):
        if slots is None:
            return self._filled()
        a = np.asarray(slots)
        if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu" or (a < 0).any() or (a >= self.capacity).any():
            raise ValueError(f"{what}: expected integers inside [0, {self.capacity})")
        return np.ascontiguousarray(a, np.int32)

    def similar(self, queries=None, targets=None, step=1, max_distance=48, times=None, exclude=-1, min_score=0, k=0, want_scores=True):
        """Similarity of stored frames (ORB + Hamming estimators): a dict with "queries" / "targets" (the slot lists; None
        = all filled slots), "scores" [nq, nt] -- crossCheck matches within max_distance between every step-th descriptor
        of the two frames -- and, with k > 0, "cand" [nq, k] (positions in targets, -1 past "n_cand"), "cand_score",
        "n_cand": the k best targets of a query among those in another slot, more than `exclude` apart in time when
        exclude >= 0, and scoring at least min_score.  times: one time per store slot (frame numbers of a ring); None =
        the slot numbers.  want_scores=False leaves "scores" None (the matrix stays on the GPU)."""
        q, t = self._slot_list(queries, "queries"), self._slot_list(targets, "targets")
        eng = self._engine((self._eng.height, self._eng.width))
        q_time = t_time = None
        if times is not None:
            times = np.asarray(times)
            if times.shape != (self.capacity,) or times.dtype.kind not in "iu":
                raise ValueError(f"times: expected {self.capacity} integers, one per slot")
            q_time, t_time = times[q], times[t]
        out = eng.frames_similar(q, t, step=step, max_distance=max_distance, q_time=q_time, t_time=t_time, exclude=exclude,
                                 min_score=min_score, k=k, want_scores=want_scores)
        out["queries"], out["targets"] = q, t
        return out

    def propose_pairs(self, k=3, exclude=-1, min_score=0, step=1, max_distance=48, queries=None, targets=None, times=None):
        """(pairs i32[P, 2], scores i32[P]): the slot pairs worth estimating -- every query's k most similar targets (see
        similar), each unordered pair once as (min, max), score descending then pair ascending: a pair list for
        estimate.  max_distance = 48 is what the synthetic loop scene supports, not a value tuned on real
        imagery."""
        if int(k) < 1:
            raise ValueError("propose_pairs: k must be >= 1")
        s = self.similar(queries, targets, step=step, max_distance=max_distance, times=times, exclude=exclude, min_score=min_score, k=k,
                         want_scores=False)
        return geometry.pairs_of_candidates(s["queries"], s["targets"], s["cand"], s["cand_score"])

    def info(self, slots):
        """(keypoint counts, OVF_* flags) of the slots; count -1 = never filled"""
        slots = np.asarray(slots)
        if slots.ndim != 1 or slots.size == 0 or slots.dtype.kind not in "iu" or (slots < 0).any() or (slots >= self.capacity).any():
            raise ValueError(f"info: slots must be integers inside [0, {self.capacity})")
        if self._eng is None:
            return np.full(slots.size, -1, np.int32), np.zeros(slots.size, np.uint32)
        return self._engine((self._eng.height, self._eng.width)).frames_info(slots)

    def close(self):
        eng, self._eng = self._eng, None
        if eng is not None and eng.h is not None and getattr(eng, "_store_owner", None) is self:
            eng.frames_reserve(0)
            eng._store_owner = None


class PoseEstimator:
    def __init__(self,
                 camera_matrix,
                 feature_method="ORB",
                 norm_type="Hamming",
                 max_matches=500,
                 nfeatures=4000,
                 use_vp_refinement=False,
                 vp_max_lines=120,
                 vp_max_pairs=3000,
                 vp_acc_min=8e5,
                 vp_vp2_min=8000.0,
                 vp_iters=12,
                 vp_lm_lambda=1e-2,
                 vp_cost_improve_eps=1e-3,
                 device=0,
                 max_batch=1,
                 ratio=None,
                 keypoint_order="libstdc++",
                 *,
                 dist_coeffs=None):
        self.K = np.asarray(camera_matrix, dtype=np.float64)
        # dist_coeffs (cv2 order, 4 / 5 / 8 values; NOT in the reference): every estimate runs the camera path with
        # Camera(K, dist_coeffs) for every frame.  None = the single-K calls, untouched.
        self._camera = None if dist_coeffs is None else _capi.Camera(self.K, dist_coeffs)
        if self._camera is not None and use_vp_refinement:
            raise ValueError("use_vp_refinement works on image lines, which a lens bends: it cannot be combined with dist_coeffs")
        self.feature_method = feature_method
        self.norm_type = norm_type
        self.max_matches = max_matches
        self.nfeatures = nfeatures
        self.use_vp_refinement = use_vp_refinement
        self.vp_max_lines = vp_max_lines
        self.vp_max_pairs = vp_max_pairs
        self.vp_acc_min = vp_acc_min
        self.vp_vp2_min = vp_vp2_min
        self.vp_iters = vp_iters
        self.vp_lm_lambda = vp_lm_lambda
        self.vp_cost_improve_eps = vp_cost_improve_eps
        self.device = device
        self.max_batch = max_batch
        self.ratio = ratio            # None = the reference's crossCheck matcher; a float = knnMatch(k=2) + Lowe ratio (extension)
        # same validation order and messages as _create_feature_extractor / _create_matcher
        method = self.feature_method.upper()
        if method == "ORB":
            self._feature = _capi.FEATURE_ORB
        elif method == "SIFT":
            self._feature = _capi.FEATURE_SIFT
        else:
            raise ValueError(f"Unknown feature extraction method: {method}")
        norm = self.norm_type.upper()
        if norm == "HAMMING":
            self._norm = _capi.NORM_HAMMING
        elif norm == "L2":
            self._norm = _capi.NORM_L2
        else:
            raise ValueError(f"Unknown norm type: {norm}")
        # cv2 builds the SIFT + NORM_HAMMING matcher too (pose_estimator.py:131) and only its match() (:144) raises, on the
        # float descriptors: so does this class -- construction succeeds, the first estimate raises (_check_runnable)
        self._unrunnable = (self._feature, self._norm) == (_capi.FEATURE_SIFT, _capi.NORM_HAMMING)
        if keypoint_order not in ("libstdc++", "msvc"):
            raise ValueError(f"Unknown keypoint order: {keypoint_order}")
        self.keypoint_order = keypoint_order
        self._engines = {}

    def _check_runnable(self):
        if self._unrunnable:
            # cv2.error is not a RuntimeError; the text is batchDistance's (core/batch_distance.cpp): type CV_32F = 5,
            # dtype CV_32S = 4, NORM_HAMMING = 6
            raise RuntimeError("OpenCV: (-210:Unsupported format or combination of formats) The combination of type=5, dtype=4 "
                               "and normType=6 is not supported in function 'batchDistance'")

    def _engine(self, height, width, batch):
        self._check_runnable()
        key = (height, width)
        eng = self._engines.get(key)
        if eng is None or eng.max_batch < batch:
            if eng is not None:
                eng.close()
            # SIFT: the reference's cv2.SIFT_create() takes no arguments (pose_estimator.py:93-94; nfeatures is documented
            # "ORB only", :41), so nothing is removed by response: nfeatures = 0 asks the library for exactly that.  The
            # arrays hold SIFT_UNCAPPED_CAPACITY keypoints per image; an image with more carries OVF_SIFT_KEYPOINTS.
            sift = self._feature == _capi.FEATURE_SIFT
            nf = 0 if sift else self.nfeatures
            cap = (_capi.SIFT_UNCAPPED_CAPACITY if sift else nf) + 64
            # max_matches=None is the reference's "no truncation" (pose_estimator.py:150-151): every cross-checked
            # match is kept, at most one per keypoint = the keypoint capacity (the RANSAC tables stop at 8064 matches)
            mm = min(self.max_matches if self.max_matches is not None else cap, cap, _capi.MAX_MATCHES_LIMIT)
            eng = _capi.Engine(width, height, max_batch=max(batch, self.max_batch), nfeatures=nf,
                               max_matches=mm, device=self.device, feature_method=self._feature, norm_type=self._norm,
                               match_mode=_capi.MATCH_RATIO if self.ratio is not None else _capi.MATCH_CROSSCHECK,
                               match_ratio=float(self.ratio) if self.ratio is not None else 0.75,
                               stl_runtime=_capi.STL_MSVC if self.keypoint_order == "msvc" else _capi.STL_LIBSTDCXX)
            self._engines[key] = eng
        return eng

    @staticmethod
    def _raise_for(status, n_matches):
        if status == _capi.PAIR_NO_DESCRIPTORS:
            raise RuntimeError("Could not compute descriptors for one of the images.")
        if status == _capi.PAIR_INSUFFICIENT_MATCHES:
            raise RuntimeError(f"Insufficient matches: {n_matches} (minimum 5 required)")
        if status == _capi.PAIR_NO_ESSENTIAL:
            raise RuntimeError("Could not estimate Essential matrix.")
        if status == _capi.PAIR_AMBIGUOUS_ESSENTIAL:
            # exactly 5 matches, several five-point models: cv2.findEssentialMat returns them stacked (3n x 3) and the
            # reference's cv2.recoverPose(E, ...) call (pose_estimator.py:533) raises cv2.error with this assertion
            raise RuntimeError("OpenCV: (-215:Assertion failed) E.cols == 3 && E.rows == 3 in function 'decomposeEssentialMat' "
                               "(findEssentialMat returned several stacked models for exactly 5 matches)")

    @staticmethod
    def _gray(img):
        img = np.asarray(img)
        if img.ndim != 2 or img.dtype != np.uint8:
            raise ValueError("expected a 2-D uint8 grayscale image")
        return img

    def _run_batch(self, eng, imgs1, imgs2, cameras1=None, cameras2=None):
        """one engine batch: the single-K call, or the camera call when cameras are given or the estimator has dist_coeffs"""
        if cameras1 is None and cameras2 is None and self._camera is None:
            return eng.estimate_batch(imgs1, imgs2, self.K)
        default = self._camera if self._camera is not None else _capi.Camera(self.K)
        return eng.estimate_batch_cameras(imgs1, imgs2, default if cameras1 is None else cameras1,
                                          default if cameras2 is None else cameras2)

    def estimate_batch(self, imgs1, imgs2, cameras1=None, cameras2=None):
        """(R[B,3,3], t[B,3,1], inliers[B], status[B]); a failing pair never aborts the batch.  cameras1 / cameras2: a
        Camera per image (or one for all) of imgs1 / imgs2; a side left None uses the estimator's own camera."""
        imgs1 = np.ascontiguousarray(imgs1, np.uint8); imgs2 = np.ascontiguousarray(imgs2, np.uint8)
        B, H, W = imgs1.shape
        if cameras1 is not None:
            cameras1 = _capi.camera_records(cameras1, B)                 # ValueError before any device call
        if cameras2 is not None:
            cameras2 = _capi.camera_records(cameras2, B)
        eng = self._engine(H, W, B)
        R, t, inl, nm, st = self._run_batch(eng, imgs1, imgs2, cameras1, cameras2)
        self._last_n_matches = nm
        self._last_engine, self._last_pairs = eng, B
        return R, t, inl, st

    def _run_pair_list(self, eng, pairs, cameras=False):
        """pairs [P, 2] int32 of store slots, in chunks of at most max_batch; cameras: on the slots' cameras"""
        P = pairs.shape[0]
        R = np.zeros((P, 3, 3)); t = np.zeros((P, 3, 1))
        inl = np.zeros(P, np.int32); nm = np.zeros(P, np.int32); st = np.zeros(P, np.int32)
        for a in range(0, P, eng.max_batch):
            b = min(a + eng.max_batch, P)
            if cameras:
                R[a:b], t[a:b], inl[a:b], nm[a:b], st[a:b] = eng.estimate_pairs_cameras(pairs[a:b, 0], pairs[a:b, 1])
            else:
                R[a:b], t[a:b], inl[a:b], nm[a:b], st[a:b] = eng.estimate_pairs(pairs[a:b, 0], pairs[a:b, 1], self.K)
            self._last_n_matches, self._last_engine, self._last_pairs = nm[a:b].copy(), eng, b - a
        return R, t, inl, nm, st

    def estimate_pairs(self, frames, pairs):
        """Relative poses over an arbitrary pair list (not in the reference): frames [F, H, W] uint8 gray (or
        [F, H, W, 3] BGR, converted with cv2's weights on the GPU), pairs [P, 2] integer frame indices -- any frames,
        repeats, reversed and self pairs.  Every frame is extracted once, whatever the number of pairs that name it
        (a window of k successors per frame costs F extractions, not 2 k F); pair (a, b) returns the bits estimate_batch
        returns for (frames[a], frames[b]).  Returns (R[P,3,3], t[P,3,1], inliers[P], n_matches[P], status[P]); a failing
        pair never aborts the list.  The frames are put in chunks of at most 2*max_batch and the list runs in chunks of
        at most max_batch (plan_pairs); last_structure(), last_refined() and last_overflow() describe the LAST chunk of
        pairs, as they do for estimate_batch.  Needs F store slots of GPU memory, which stay with the engine and are reused by the next call
        (INTEGRATION.md section 7)."""
        frames = self._check_frames(frames)
        pairs = _check_pairs(pairs, frames.shape[0], "frame")
        eng = self._fill_store(frames, pairs.shape[0])
        return self._run_pair_list(eng, pairs, cameras=self._camera is not None)

    @staticmethod
    def _check_frames(frames):
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[-1] != 3) or frames.shape[0] < 1:
            raise ValueError(f"frames: expected uint8 [F, H, W] or [F, H, W, 3], got {frames.dtype} {frames.shape}")
        return frames

    def _fill_store(self, frames, n_pairs):
        """estimate_pairs' store: frame f extracted into slot f of the engine of the frames' size, which is returned"""
        F, H, W = frames.shape[:3]
        eng = self._engine(H, W, 1)
        if getattr(eng, "_store_owner", None) is not None:
            raise _capi.RpeError("the engine of this image size serves a FrameStore: use its estimate(), or close it first")
        puts, _ = plan_pairs(F, n_pairs, eng.max_batch)
        if eng.frames_capacity() < F:         # a store left by an earlier call is reused when it is large enough
            eng.frames_reserve(0)
            eng.frames_reserve(F)
        for a, b in puts:
            chunk = frames[a:b]
            gray = eng.bgr_to_gray(chunk) if chunk.ndim == 4 else chunk
            eng.frames_put(gray, np.arange(a, b, dtype=np.int32))
        if self._camera is not None:
            eng.frames_set_cameras(np.arange(F, dtype=np.int32), self._camera)
        return eng

    def close_loops(self, frames, R_abs, T_abs, frame_group, loop_pairs=None, k=3, exclude=8, min_score=0, huber=2.0, **solver):
        """Loop closure over a chain (not in the reference): the poses of the loop pairs, the pose graph of the chain with
        those pairs as loop edges, and its optimisation on the GPU (_capi.Engine.optimise_graphs).  frames as in
        estimate_pairs; R_abs [F, 3, 3], T_abs [F, 3], frame_group [F]: a chain and its scale groups, as estimate_trajectory
        and geometry.frame_groups give them (estimate_trajectory itself is unchanged: its result feeds this call).
        loop_pairs [P, 2]: the frame pairs that see the same place again; None: proposed from the frames themselves --
        every frame's k most similar frames more than `exclude` frames away scoring at least min_score (frames_similar
        over the store estimate_pairs fills, frame f in slot f, time = frame) -- which needs an ORB + Hamming estimator:
        others raise ValueError without the list.  The graph: geometry.chain_edges, loop_edges and graphs_of_groups with
        their default sigmas; loop pairs across groups are dropped.  huber and solver (max_iters, cg_iters, cg_tol) go to
        optimise_graphs; the default bound of 2 keeps a wrong loop edge from bending the chain.
        Returns a dict: 'R_abs_graph' [F, 3, 3], 'T_abs_graph' [F, 3], 'centers_graph' [F, 3]: the chain with the frames
        of every graph whose code is GRAPH_OK replaced; 'graph': the solver's dict with 'graphs' and 'edges' (what it was
        given) and 'dropped' (indices of loop pairs that became no edge) added; 'loop_pairs' [P, 2]; and the pair results
        'R', 't', 'inliers', 'n_matches', 'status' of the loop pairs."""
        frames = self._check_frames(frames)
        F = frames.shape[0]
        R_abs = np.asarray(R_abs, np.float64).reshape(-1, 3, 3); T_abs = np.asarray(T_abs, np.float64).reshape(-1, 3)
        group = np.asarray(frame_group).reshape(-1)
        if not (R_abs.shape[0] == T_abs.shape[0] == group.size == F):
            raise ValueError("close_loops: R_abs, T_abs and frame_group hold one entry per frame")
        if loop_pairs is None and (self._feature, self._norm) != (_capi.FEATURE_ORB, _capi.NORM_HAMMING):
            raise ValueError("close_loops: pairs are proposed on ORB + Hamming estimators only; pass loop_pairs")
        if loop_pairs is not None:
            loop_pairs = _check_pairs(loop_pairs, F, "frame")
        eng = self._fill_store(frames, F if loop_pairs is None else loop_pairs.shape[0])
        if loop_pairs is None:
            every = np.arange(F, dtype=np.int32)
            s = eng.frames_similar(every, every, exclude=exclude, min_score=min_score, k=k, want_scores=False)
            loop_pairs, _ = geometry.pairs_of_candidates(every, every, s["cand"], s["cand_score"])
        if loop_pairs.shape[0]:
            R, t, inl, nm, st = self._run_pair_list(eng, loop_pairs, cameras=self._camera is not None)
        else:
            R, t = np.zeros((0, 3, 3)), np.zeros((0, 3, 1))
            inl = nm = st = np.zeros(0, np.int32)
        chain = geometry.chain_edges(R_abs, T_abs, group)
        loops, dropped = geometry.loop_edges(loop_pairs, R, t, st, group)
        graphs = geometry.graphs_of_groups(group)
        edges = geometry.edges_of_graphs(graphs, chain, loops)
        res = eng.optimise_graphs(R_abs, T_abs, graphs, edges, huber=huber, **solver)
        Rg, Tg = R_abs.copy(), T_abs.copy()
        for g, fr in enumerate(graphs):
            if res['code'][g] == _capi.GRAPH_OK:
                Rg[fr] = res['R'][g]; Tg[fr] = res['T'][g]
        res.update({'graphs': graphs, 'edges': edges, 'dropped': dropped})
        return {'R_abs_graph': Rg, 'T_abs_graph': Tg, 'centers_graph': -np.einsum("fji,fj->fi", Rg, Tg), 'graph': res,
                'loop_pairs': loop_pairs, 'R': R, 't': t, 'inliers': inl, 'n_matches': nm, 'status': st}

    def frame_store(self, capacity):
        """A FrameStore of `capacity` slots on this estimator's engine (created for the size of the first frame put)."""
        self._check_runnable()
        return FrameStore(self, capacity)

    def last_overflow(self):
        """OVF_* capacity flags (see _capi) of the pairs of the last estimate_batch / estimate_sequence call: nonzero
        where a fixed-size GPU workspace truncated a list cv2 would have kept whole (status stays OK)."""
        return self._last_engine.fetch_overflow(self._last_pairs)

    def last_structure(self):
        """Per-match results of the pairs of the last estimate_batch / estimate_sequence call: one dict per pair with
        arrays trimmed to the pair's match count -- 'ransac_mask' (n,) bool, findEssentialMat's inlier mask;
        'pose_mask' (n,) bool, recoverPose's cheirality mask of the returned pose (its sum is the pair's inlier count);
        'points3d' (n, 3), the triangulated point of every match in the camera-1 frame on the |t| = 1 scale.  All zero
        for pairs whose status is not OK.  Raises RpeError after a chunked host batch, which keeps no per-match
        results."""
        eng, B = self._last_engine, self._last_pairs
        rm, pm, pts = eng.fetch_structure(B)
        out = []
        for p in range(B):
            n = int(self._last_n_matches[p])
            out.append({'ransac_mask': rm[p, :n].copy(), 'pose_mask': pm[p, :n].copy(), 'points3d': pts[p, :n].copy()})
        return out

    def last_refined(self, max_iters=10):
        """Refined poses of the pairs of the last estimate_batch / estimate_sequence call (not in the reference):
        Levenberg-Marquardt on the Sampson error over findEssentialMat's inliers, started from the returned (R, t), on
        the GPU.  Returns (R[B,3,3], t[B,3,1], inliers[B], status[B], info[B,4], rms[B,2]): the shape of estimate_batch
        plus info = (_capi.REFINE_* code, iterations run, residuals used, accepted steps) and rms = (before, after) in
        pixels.  Pairs that were skipped or rejected carry the unrefined pose.  Raises RpeError after a chunked host
        batch, which keeps no per-match results."""
        eng, B = self._last_engine, self._last_pairs
        R, t, inl, info, rms = eng.refine_poses(B, max_iters)
        return R, t, inl, eng.fetch_results(B)[4], info, rms

    def last_scale_links(self, links, min_shared=8):
        """Relative scale of pairs of the last estimate_sequence / estimate_pairs / FrameStore.estimate call that share
        a frame (not in the reference; _capi.Engine.scale_links).  links: integer array [L, 3] of (pair_a, pair_b, side)
        over the pairs of that call (of its LAST chunk when the call ran in several), side bit 0 / bit 1 = the shared
        frame is image 2 (else image 1) of pair_a / pair_b: consecutive pairs (i, i + 1) of a sequence are (i, i + 1, 1).
        Returns (stats[L, 3], n_shared[L], code[L]): lower quartile, median and upper quartile of the baseline of pair_b
        in units of the baseline of pair_a, the number of shared keypoints, and the _capi.LINK_* code.  Raises RpeError
        after estimate_batch (its pairs share no frame) and when a link names a frame the two pairs do not share."""
        a = np.asarray(links)
        if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
            raise ValueError(f"links: expected an integer array of shape [L, 3] (pair_a, pair_b, side), got {a.dtype} {a.shape}")
        return self._last_engine.scale_links(a[:, 0], a[:, 1], a[:, 2], min_shared)

    def last_link_poses(self, links, iters=256, threshold_px=None, min_shared=8, refine_iters=10):
        """Pose of pair_b's other frame against the points pair_a triangulated, for links over the last
        estimate_sequence / estimate_pairs / FrameStore.estimate call (not in the reference;
        _capi.Engine.link_poses): pair_b's relative pose on pair_a's scale, from pair_b's matches alone -- it needs
        neither pair_b's essential matrix nor any parallax in pair_b.  links as in last_scale_links.  Returns
        (R[L, 3, 3], t[L, 3], mask[L, mm], counts[L, 2], info[L, 4], rms[L, 2])."""
        a = np.asarray(links)
        if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
            raise ValueError(f"links: expected an integer array of shape [L, 3] (pair_a, pair_b, side), got {a.dtype} {a.shape}")
        return self._last_engine.link_poses(a[:, 0], a[:, 1], a[:, 2], iters, threshold_px, min_shared, refine_iters)

    def last_link_bundles(self, links, threshold_px=None, min_shared=8, max_iters=10):
        """Bundle adjustment of the three views of every link over the last estimate_sequence / estimate_pairs /
        FrameStore.estimate call (not in the reference; _capi.Engine.link_bundles): the link poses first
        (last_link_poses with its defaults and this min_shared), then both pairs' poses and the points they share refined
        together.  A link whose link pose is not LINKPOSE_OK comes back BUNDLE_SKIPPED.  links as in last_scale_links.
        Returns (R_a[L, 3, 3], t_a[L, 3], R_b[L, 3, 3], t_b[L, 3], points[L, mm, 3], views[L, mm], counts[L, 2], info[L, 4],
        rms[L, 2])."""
        a = np.asarray(links)
        if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
            raise ValueError(f"links: expected an integer array of shape [L, 3] (pair_a, pair_b, side), got {a.dtype} {a.shape}")
        eng = self._last_engine
        R0, t0 = eng.link_poses(a[:, 0], a[:, 1], a[:, 2], min_shared=min_shared)[:2]
        return eng.link_bundles(a[:, 0], a[:, 1], a[:, 2], R0, t0, threshold_px, min_shared, max_iters)

    def last_tracks(self, edge_rule=_capi.TRACK_EDGES_USABLE, min_len=2, use_pair=None):
        """Feature tracks over the pairs of the last estimate_sequence / estimate_pairs / FrameStore.estimate call (of its
        LAST chunk when the call ran in several; not in the reference; _capi.Engine.build_tracks): which keypoint of which
        frame is the same scene point, at most one keypoint per frame and at least min_len frames per track.  A frame is
        its index in the sequence, or its store slot (estimate_pairs: its index in `frames`).  Returns the dict of
        build_tracks.  Raises RpeError after an estimate_batch of two or more pairs (its pairs share no frame); a batch of
        one pair -- estimate() -- is the stream of its two images: frame 0 is image 1, frame 1 is image 2."""
        return self._last_engine.build_tracks(use_pair, edge_rule, min_len)

    def last_track_points(self, R_abs, T_abs, frame_group=None, tracks=None, **gates):
        """One scene point per track from all its views under the absolute poses R_abs [F, 3, 3], T_abs [F, 3]
        (x = R X + T; not in the reference; _capi.Engine.triangulate_tracks, whose dict it returns).  tracks: a dict of
        last_tracks / build_tracks, None = last_tracks() with its defaults; a frame of the tracks indexes the poses.
        frame_group: see geometry.frame_groups.  The camera is the estimator's: its K, or its Camera (one for all frames)
        when it was built with dist_coeffs.  gates: threshold_px, min_views, max_cos, max_iters of triangulate_tracks."""
        if tracks is None:
            tracks = self.last_tracks()
        cam = {'cameras': self._camera} if self._camera is not None else {'K': self.K}
        return self._last_engine.triangulate_tracks(tracks, R_abs, T_abs, frame_group=frame_group, **cam, **gates)

    def last_window_bundles(self, R_abs, T_abs, points=None, tracks=None, size=8, overlap=2, **kw):
        """Bundle adjustment of sliding windows over the tracks of the last sequence under the absolute poses R_abs
        [F, 3, 3], T_abs [F, 3] (not in the reference; _capi.Engine.bundle_windows, whose dict it returns with 'windows', the
        list of frame lists, added).  points: a dict of last_track_points over the same poses (its 'points' are the start
        points, its 'obs_flag' selects the observations, its codes TRACKPT_OK the tracks, its 'frame_group' if present the
        groups); None = last_track_points(R_abs, T_abs, tracks=tracks) with its defaults, all frames in one group.  The
        windows are geometry.windows_of_groups(frame_group, size, overlap).  kw: max_points, min_obs, max_iters of
        bundle_windows.  The camera is the estimator's, as in last_track_points."""
        if tracks is None:
            tracks = self.last_tracks()
        if points is None:
            points = self.last_track_points(R_abs, T_abs, tracks=tracks)
        F = np.asarray(R_abs).reshape(-1, 9).shape[0]
        group = points.get('frame_group')
        windows = geometry.windows_of_groups(np.zeros(F, np.int32) if group is None else group, size, overlap)
        cam = {'cameras': self._camera} if self._camera is not None else {'K': self.K}
        out = self._last_engine.bundle_windows(tracks, points['points'], R_abs, T_abs, windows, obs_use=points['obs_flag'],
                                               point_use=(np.asarray(points['code']) == _capi.TRACKPT_OK).astype(np.uint8), **cam, **kw)
        out['windows'] = windows
        return out

    def estimate_trajectory(self, frames, min_shared=8, register=False, bundle=False, tracks=False, points=False, window=0):
        """estimate_sequence plus what relates its poses (not in the reference): the scale link of every two consecutive
        pairs and the chained trajectory (geometry.chain_trajectory).  Returns a dict: 'R', 't', 'inliers', 'status' of
        the F - 1 pairs; 'ratio_stats' [F-2, 3], 'n_shared' [F-2], 'link_code' [F-2] of the links; 'R_abs' [F, 3, 3],
        'T_abs' [F, 3], 'centers' [F, 3], 'baseline' [F-1], 'segment' [F-1].  Distances share a scale only inside a
        segment; the unit is the baseline of the segment's first pair.
        register=True adds the link pose of every link (last_link_poses with its defaults and this min_shared): 'R_link'
        [F-2, 3, 3], 't_link' [F-2, 3], 'link_pose_code' [F-2], 'link_pose_counts' [F-2, 2], and 'R_abs_reg' [F, 3, 3],
        'centers_reg' [F, 3]: chain_trajectory again with pair i + 1 taken from link i where its code is LINKPOSE_OK
        (R_link, t_link / |t_link|, ratio |t_link|, status 0) and from the pair's own pose and scale link elsewhere.
        bundle=True implies register and adds the link bundle of every link fed with those link poses
        (_capi.Engine.link_bundles with its defaults and this min_shared): 'R_bundle' [F-2, 3, 3], 't_bundle' [F-2, 3]
        (pair i + 1's pose on pair i's scale), 'bundle_code' [F-2], 'bundle_counts' [F-2, 2], and 'R_abs_ba' [F, 3, 3],
        'centers_ba' [F, 3]: the registered chain with the bundle's pose where its code is BUNDLE_OK, the link pose
        elsewhere.
        tracks=True adds 'tracks': the feature tracks of the sequence (last_tracks with its defaults).
        points=True implies tracks and adds 'points': the dict of last_track_points (its defaults) over those tracks under
        the best chain built, plus 'chain', the key of that chain's rotations ('R_abs_ba' with bundle, else 'R_abs_reg'
        with register, else 'R_abs'), and the 'T_abs' [F, 3] and 'frame_group' [F] (geometry.frame_groups of that chain)
        it was run with.  Points of different groups are on unrelated scales.
        window=W (2 .. 8) implies points and adds 'window': the dict of last_window_bundles over those points and that chain
        with windows of W frames (overlap min(2, W - 1)), and the chain the OK windows fuse into
        (geometry.chain_windows): 'R_abs_win' [F, 3, 3], 'T_abs_win' [F, 3], 'centers_win' [F, 3]."""
        if self._camera is not None:
            raise ValueError("estimate_trajectory: the camera path has no stream form; use estimate_pairs and last_scale_links")
        R, t, inl, st = self.estimate_sequence(frames)
        P = len(st)
        i = np.arange(P - 1, dtype=np.int32)
        stats, n_shared, code = self._last_engine.scale_links(i, i + 1, np.ones(P - 1, np.int32), min_shared)
        R_abs, T_abs, centers, baseline, segment = geometry.chain_trajectory(R, t, st, stats[:, 1], code)
        out = {'R': R, 't': t, 'inliers': inl, 'status': st, 'ratio_stats': stats, 'n_shared': n_shared, 'link_code': code,
               'R_abs': R_abs, 'T_abs': T_abs, 'centers': centers, 'baseline': baseline, 'segment': segment}
        best = ('R_abs', T_abs, st, segment)      # the chain the points are triangulated under: key, T, status, segment
        if register or bundle:
            Rl, tl, _, counts, info, _ = self._last_engine.link_poses(i, i + 1, np.ones(P - 1, np.int32), min_shared=min_shared)
            Rr, tr, sr, ratio, cr = geometry.registered_chain_inputs(R, t, st, stats[:, 1], code, Rl, tl, info[:, 0])
            reg = geometry.chain_trajectory(Rr, tr, sr, ratio, cr)
            out.update({'R_link': Rl, 't_link': tl, 'link_pose_code': info[:, 0], 'link_pose_counts': counts,
                        'R_abs_reg': reg[0], 'centers_reg': reg[2]})
            best = ('R_abs_reg', reg[1], sr, reg[4])
        if bundle:
            one = np.ones(P - 1, np.int32)
            ba = self._last_engine.link_bundles(i, i + 1, one, Rl, tl, min_shared=min_shared)
            ok = ba[7][:, 0] == 0
            Rb = np.where(ok[:, None, None], ba[2], Rl); tb = np.where(ok[:, None], ba[3], tl)
            ba_in = geometry.registered_chain_inputs(R, t, st, stats[:, 1], code, Rb, tb, info[:, 0])
            chain = geometry.chain_trajectory(*ba_in)
            out.update({'R_bundle': ba[2], 't_bundle': ba[3], 'bundle_code': ba[7][:, 0], 'bundle_counts': ba[6],
                        'R_abs_ba': chain[0], 'centers_ba': chain[2]})
            best = ('R_abs_ba', chain[1], ba_in[2], chain[4])
        if tracks or points or window:
            out['tracks'] = self._last_engine.build_tracks()
        if points or window:
            group = geometry.frame_groups(best[2], best[3])
            out['points'] = self.last_track_points(out[best[0]], best[1], group, out['tracks'])
            out['points'].update({'chain': best[0], 'T_abs': best[1], 'frame_group': group})
        if window:
            win = self.last_window_bundles(out[best[0]], best[1], out['points'], out['tracks'], size=window, overlap=min(2, window - 1))
            fused = geometry.chain_windows(win['windows'], win['R'], win['T'], win['code'], out[best[0]], best[1])
            out.update({'window': win, 'R_abs_win': fused[0], 'T_abs_win': fused[1], 'centers_win': fused[2]})
        return out

    def estimate_sequence(self, frames):
        """Relative poses of consecutive frames (frame i -> i+1): the pair loop of the reference's
        BatchProcessor.process_sequence (batch_processor.py:71-109) with features extracted once
        per frame.  Returns (R[F-1,3,3], t[F-1,3,1], inliers[F-1], status[F-1])."""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W = frames.shape
        eng = self._engine(H, W, F - 1)
        if self._camera is not None:
            # the camera path has no stream form: the same pairs as a batch (frame i, frame i + 1), same results
            R, t, inl, nm, st = eng.estimate_batch_cameras(frames[:-1], frames[1:], self._camera, self._camera)
        else:
            R, t, inl, nm, st = eng.estimate_stream(frames, self.K)
        self._last_n_matches = nm
        self._last_engine, self._last_pairs = eng, F - 1
        return R, t, inl, st

    def _vp_refine(self, R_rel, R_prev, img1, img2):
        """pose_estimator.py:536-567: (R_rel', vp_used, vp_debug)"""
        return vp_refinement.refine_relative_rotation(
            R_rel, R_prev, img1, img2, self.K, max_lines=self.vp_max_lines, max_pairs=self.vp_max_pairs,
            acc_min=self.vp_acc_min, vp2_min=self.vp_vp2_min, iters=self.vp_iters, lm_lambda=self.vp_lm_lambda,
            cost_improve_eps=self.vp_cost_improve_eps)

    def estimate(self, img1, img2, R_prev=None):
        img1 = self._gray(img1); img2 = self._gray(img2)
        eng = self._engine(img1.shape[0], img1.shape[1], 1)
        R, t, inl, nm, st = self._run_batch(eng, img1[None], img2[None])
        self._last_n_matches, self._last_engine, self._last_pairs = nm, eng, 1
        self._raise_for(int(st[0]), int(nm[0]))
        R_rel = R[0]
        if self.use_vp_refinement and R_prev is not None:
            R_rel, _, _ = self._vp_refine(R_rel, R_prev, img1, img2)
        return R_rel, t[0]

    def estimate_with_debug(self, img1, img2, R_prev=None):
        img1 = self._gray(img1); img2 = self._gray(img2)
        eng = self._engine(img1.shape[0], img1.shape[1], 1)
        R, t, inl, nm, st = self._run_batch(eng, img1[None], img2[None])
        self._last_n_matches, self._last_engine, self._last_pairs = nm, eng, 1
        self._raise_for(int(st[0]), int(nm[0]))
        p1, p2 = eng.fetch_matched_points(1)
        n = int(nm[0])
        info = {
            'R': R[0],
            't': t[0],
            'num_matches': n,
            'pts1': p1[0, :n].copy(),
            'pts2': p2[0, :n].copy(),
            'inliers': int(inl[0]),
            'vp_used': False,
            'vp_debug': {},
        }
        if self.use_vp_refinement and R_prev is not None:
            R_rel, used, dbg = self._vp_refine(R[0], R_prev, img1, img2)
            info['vp_debug'] = dbg
            if used:
                info['R'] = R_rel
                info['vp_used'] = True
        return info

    def estimate_with_structure(self, img1, img2):
        """estimate_with_debug's pose, matches and inlier count plus the per-match results the pose rests on:
        'ransac_mask' (n,) bool = findEssentialMat's inlier mask (pose_estimator.py:522-527), 'pose_mask' (n,) bool =
        recoverPose's cheirality mask (:533, distanceThresh 50; its sum is 'inliers') and 'points3d' (n, 3) =
        recoverPose's triangulatedPoints dehomogenised: the point of every match in the camera-1 frame, |t| = 1 scale
        (points behind a camera included).  Raises what estimate raises.  VP refinement is never applied: the
        structure belongs to the five-point pose, and a refined R would not be the pose the masks and points
        describe."""
        img1 = self._gray(img1); img2 = self._gray(img2)
        eng = self._engine(img1.shape[0], img1.shape[1], 1)
        R, t, inl, nm, st = self._run_batch(eng, img1[None], img2[None])
        self._last_n_matches, self._last_engine, self._last_pairs = nm, eng, 1
        self._raise_for(int(st[0]), int(nm[0]))
        p1, p2 = eng.fetch_matched_points(1)
        rm, pm, pts = eng.fetch_structure(1)
        n = int(nm[0])
        return {
            'R': R[0],
            't': t[0],
            'num_matches': n,
            'pts1': p1[0, :n].copy(),
            'pts2': p2[0, :n].copy(),
            'inliers': int(inl[0]),
            'ransac_mask': rm[0, :n].copy(),
            'pose_mask': pm[0, :n].copy(),
            'points3d': pts[0, :n].copy(),
        }

    def estimate_refined(self, img1, img2, max_iters=10):
        """estimate_with_debug's dict (the unrefined pose stays under 'R', 't', 'inliers'; VP refinement is never
        applied) plus the non-linear refinement of that pose over findEssentialMat's inliers (not in the reference):
        'R_refined', 't_refined', 'inliers_refined' (cheirality count), 'refine_code' (_capi.REFINE_*),
        'refine_iters', 'rms_before', 'rms_after' (Sampson distance in pixels).  Raises what estimate raises."""
        info = self.estimate_with_debug(img1, img2)
        R, t, inl, rinfo, rms = self._last_engine.refine_poses(1, max_iters)
        info.update(R_refined=R[0], t_refined=t[0], inliers_refined=int(inl[0]), refine_code=int(rinfo[0, 0]),
                    refine_iters=int(rinfo[0, 1]), rms_before=float(rms[0, 0]), rms_after=float(rms[0, 1]))
        return info

    def last_guided(self, R=None, t=None, gate_px=None, max_distance=None):
        """Guided matches of the pairs of the last estimate / estimate_batch / estimate_sequence / estimate_pairs call
        (of its last chunk when it ran in several; not in the reference; _capi.Engine.guided_matches, or
        guided_matches_l2 for an estimator with NORM_L2): the mutual nearest neighbours among the keypoint pairs within
        gate_px (Sampson distance in pixels, None = the estimator's RANSAC threshold) of a pose and within max_distance
        of each other (None = no bound: 256 for Hamming, +inf for L2).  R, t None: the call's own poses, pairs that failed get no matches;
        R[B,3,3], t[B,3(,1)]: poses to gate with (refined poses, a prior from a trajectory), every pair matched.
        Returns one dict per pair, arrays trimmed to the pair's guided count: 'qidx', 'tidx' (keypoint indices in image
        1 / 2), 'dist' (int32 Hamming distances, or the matcher's f32 distances under NORM_L2), 'pts1', 'pts2' (n, 2)
        pixels."""
        eng, B = self._last_engine, self._last_pairs
        if self._norm == _capi.NORM_L2:
            q, ti, d, p1, p2, nm = eng.guided_matches_l2(B, R, t, gate_px, max_distance)
        else:
            q, ti, d, p1, p2, nm = eng.guided_matches(B, R, t, gate_px, 256 if max_distance is None else max_distance)
        return [{'qidx': q[p, :nm[p]].copy(), 'tidx': ti[p, :nm[p]].copy(), 'dist': d[p, :nm[p]].copy(),
                 'pts1': p1[p, :nm[p]].copy(), 'pts2': p2[p, :nm[p]].copy()} for p in range(B)]

    def estimate_guided(self, img1, img2, gate_px=None, max_distance=None, refine_iters=10):
        """estimate, then the guided matches at that pose (last_guided), then the non-linear refinement of the pose over
        all of them (rpe_refine_pose_points with a mask of ones; not in the reference).  Returns a dict: 'R', 't' the
        refined pose (the five-point pose when the refinement was skipped or rejected), 'R_initial', 't_initial',
        'num_guided', 'pts1', 'pts2' (the guided matches), 'inliers' (cheirality count of the returned pose),
        'refine_code' (_capi.REFINE_*), 'refine_iters', 'rms_before', 'rms_after'.  Raises what estimate raises."""
        R0, t0 = self.estimate(img1, img2)
        eng = self._last_engine
        g = self.last_guided(gate_px=gate_px, max_distance=max_distance)[0]
        n = len(g['qidx'])
        ones = [np.ones(n, bool)]
        if self._camera is not None:
            R, t, inl, rinfo, rms = eng.refine_pose_points_cameras([R0], [t0], [g['pts1']], [g['pts2']], ones, self._camera,
                                                                   self._camera, refine_iters)
        else:
            R, t, inl, rinfo, rms = eng.refine_pose_points([R0], [t0], [g['pts1']], [g['pts2']], ones, self.K, refine_iters)
        return {'R': R[0], 't': t[0], 'R_initial': R0, 't_initial': t0, 'num_guided': n, 'pts1': g['pts1'], 'pts2': g['pts2'],
                'inliers': int(inl[0]), 'refine_code': int(rinfo[0, 0]), 'refine_iters': int(rinfo[0, 1]),
                'rms_before': float(rms[0, 0]), 'rms_after': float(rms[0, 1])}

    def last_homographies(self, iters=256, threshold_px=None):
        """The second geometric model of the pairs of the last estimate / estimate_batch / estimate_sequence /
        estimate_pairs call (of its last chunk when it ran in several; not in the reference;
        _capi.Engine.pair_homographies): a homography by RANSAC (`iters` samples, transfer gate threshold_px pixels, None =
        the RANSAC threshold), the rotation fitted to its inliers, and the inlier counts.  Returns a dict of arrays over
        the B pairs: 'H' [B, 3, 3] (normalised coordinates; geometry.pixel_homography gives pixels), 'R_rot' [B, 3, 3],
        'mask' [B, max_matches] bool, 'n_H', 'n_rot', 'n_E' [B], 'n_matches' [B], 'code' [B] (_capi.HOMOGRAPHY_*),
        'iteration' [B], 'n_valid' [B].  geometry.classify_pair turns the counts into a name."""
        eng, B = self._last_engine, self._last_pairs
        H, R, mask, counts, info = eng.pair_homographies(B, iters, threshold_px)
        return {'H': H, 'R_rot': R, 'mask': mask, 'n_H': counts[:, 0].copy(), 'n_rot': counts[:, 1].copy(),
                'n_E': counts[:, 2].copy(), 'n_matches': np.asarray(self._last_n_matches, np.int32)[:B].copy(),
                'code': info[:, 0].copy(), 'iteration': info[:, 1].copy(), 'n_valid': info[:, 2].copy()}

    def estimate_with_geometry(self, img1, img2, iters=256, threshold_px=None, rotation_ratio=0.7, planar_ratio=0.8):
        """estimate, then last_homographies and geometry.classify_pair (not in the reference).  Returns
        (R, t, inliers, geom): the five-point pose and its cheirality count exactly as estimate_with_debug reports them,
        and geom = {'H', 'R_rot', 'n_H', 'n_rot', 'n_E', 'n_matches', 'mask' (n_matches,) bool, 'code', 'kind'}, kind =
        "rotation" / "planar" / "general" under the two ratios (caller policy: geometry.classify_pair).  A "rotation"
        pair has no usable baseline: t is noise there and R_rot is the rotation to use.  Raises what estimate raises."""
        d = self.estimate_with_debug(img1, img2)
        g = self.last_homographies(iters, threshold_px)
        n = int(g['n_matches'][0])
        geom = {'H': g['H'][0], 'R_rot': g['R_rot'][0], 'n_H': int(g['n_H'][0]), 'n_rot': int(g['n_rot'][0]),
                'n_E': int(g['n_E'][0]), 'n_matches': n, 'mask': g['mask'][0, :n].copy(), 'code': int(g['code'][0])}
        geom['kind'] = geometry.classify_pair(n, geom['n_E'], geom['n_H'], geom['n_rot'], rotation_ratio, planar_ratio)
        return d['R'], d['t'], d['inliers'], geom

    def close(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}


def estimate_relative_pose(img1, img2, K, **kwargs):
    """north_star's call surface: (R, t, inliers) for one image pair."""
    est = PoseEstimator(K, **kwargs)
    try:
        d = est.estimate_with_debug(img1, img2)
    finally:
        est.close()
    return d['R'], d['t'], d['inliers']
