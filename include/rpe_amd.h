/*
 * rpe_amd.h -- C-ABI of the MI355X-native relative-pose engine.
 *
 * Drop-in boundary for ONE path of ofekm5/relative-pose-estimation:
 *   PoseEstimator.estimate(img1, img2)  (reference src/core/pose_estimator.py:487-569)
 *     = ORB detectAndCompute x2        (:85-91, :108, :505-506)
 *     -> BFMatcher(HAMMING, crossCheck=True).match + sorted + [:max_matches]  (:131, :144-151)
 *     -> gather matched points                                         (:518-519)
 *     -> cv2.findEssentialMat(RANSAC, 0.999, 1.0)                       (:522-527)
 *     -> cv2.recoverPose                                               (:533)
 *
 * The reference has no FFI (it is Python calling cv2); the entry points below
 * are what a ctypes binding for that path binds (INTEGRATION.md shows the
 * stub).  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *  - every function returns an int status: 0 = OK, <0 = library error
 *    (rpe_last_error() gives text).  Per-pair outcomes are reported in the
 *    status[] output array (RPE_PAIR_*), never as a failed call: a batch
 *    does not abort on one bad pair (the reference raises RuntimeError,
 *    pose_estimator.py:508-509,514-515,529-530; the Python wrapper maps the
 *    per-pair code back to the same exception text).
 *  - a handle owns one HIP device, one stream and its workspaces; it is not
 *    thread-safe; different handles are independent (one per GPU).
 *  - pointers named h_* are host memory, d_* are device (HBM) memory.
 *  - images are uint8 gray, row-major, tightly packed H x W, one after another.
 *  - matrices are row-major doubles: K[9], R[9] per pair, t[3] per pair.
 *  - results are bit-deterministic run to run (integer atomics only).
 */
#ifndef RPE_AMD_H
#define RPE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPE_ABI_VERSION 3
#define RPE_ORB_LEVELS 12

/* per-pair status codes (status[] outputs) */
enum {
    RPE_PAIR_OK = 0,
    RPE_PAIR_NO_DESCRIPTORS = 1,       /* pose_estimator.py:508-509 */
    RPE_PAIR_INSUFFICIENT_MATCHES = 2, /* pose_estimator.py:514-515 */
    RPE_PAIR_NO_ESSENTIAL = 3,         /* pose_estimator.py:529-530 */
    /* exactly 5 matches and the five-point solver returned more than one model: cv2.findEssentialMat then
     * returns all of them stacked (3n x 3, ptsetreg.cpp count == modelPoints) and the reference's
     * cv2.recoverPose(E, ...) call (pose_estimator.py:533) fails its `E.cols == 3 && E.rows == 3` assertion */
    RPE_PAIR_AMBIGUOUS_ESSENTIAL = 4
};

/* Capacity flags of the last batch (rpe_fetch_overflow): a fixed-size workspace truncated a list that cv2
 * would have kept whole, so the pair's features differ from the reference's although status is RPE_PAIR_OK. */
enum {
    RPE_OVF_ORB_CANDIDATES = 1 << 0,   /* a pyramid level had more FAST corners than clamp(w h / 64, 1024, 8192), or more than 4*quota+256 survived retainBest(2*quota) (score ties) */
    RPE_OVF_ORB_KEYPOINTS  = 1 << 1,   /* more than nfeatures+64 keypoints after the Harris retainBest (ties) */
    RPE_OVF_SIFT_SEEDS     = 1 << 4,   /* more scale-space extrema than base_pixels/16 */
    RPE_OVF_SIFT_RAW       = 1 << 5,   /* more oriented keypoints than the raw list holds */
    RPE_OVF_SIFT_PREFILTER = 1 << 6,   /* response ties overflowed the pre-sort window */
    RPE_OVF_SIFT_CAP       = 1 << 7,   /* the nfeatures cap removed keypoints: differs from the reference's uncapped SIFT_create() (pose_estimator.py:93-94).
                                          The kept set is retainBest's, reported sorted; cv2 keeps std::nth_element's order, which
                                          changes R / t in 6 of 16 configs[2] pairs */
    RPE_OVF_SIFT_KEYPOINTS = 1 << 8    /* more than nfeatures+64 keypoints after retainBest (ties), or more than RPE_SIFT_UNCAPPED_CAPACITY+64 without a cap */
};

/* library error codes (function return values) */
enum {
    RPE_OK = 0,
    RPE_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    RPE_ERR_HIP = -2,       /* HIP runtime failure (no device, OOM, launch error) */
    RPE_ERR_CAPACITY = -3   /* batch larger than the handle's max_batch */
};

enum { RPE_FEATURE_ORB = 0, RPE_FEATURE_SIFT = 1 };
#define RPE_SIFT_UNCAPPED_CAPACITY 16320   /* keypoints per image held when SIFT runs without a cap (nfeatures = 0) */
enum { RPE_NORM_HAMMING = 0, RPE_NORM_L2 = 1 };
/* RPE_MATCH_CROSSCHECK = the reference (BFMatcher(norm, crossCheck=True).match, pose_estimator.py:131,144).
 * RPE_MATCH_RATIO = opt-in extension named by the project brief, NOT in the reference: knnMatch(k=2) + Lowe's
 * ratio test (best < ratio * second best), no cross check; then the same sort / top-max_matches. */
enum { RPE_MATCH_CROSSCHECK = 0, RPE_MATCH_RATIO = 1 };
/* Which C++ runtime's std::nth_element / std::partition orders the ORB keypoints inside a pyramid level.  cv2's
 * KeyPointsFilter::retainBest (called twice per level by ORB, orb.cpp computeKeyPoints) leaves its vector in the
 * order those two library calls happen to produce, descriptor rows follow that order, and BFMatcher ties / the
 * reference's stable sort before the top-500 cut (pose_estimator.py:147-151) / the fixed-seed RANSAC then depend on
 * it.  The reference's committed result files pin it row by row: RPE_STL_LIBSTDCXX reproduces the Salah and phone
 * files (Linux wheels; the reference's Dockerfile is python:3.9-slim), RPE_STL_MSVC the simulator file (a Windows
 * wheel produced it).  The keypoint SET is the same under both. */
enum { RPE_STL_LIBSTDCXX = 0, RPE_STL_MSVC = 1 };

/* Mirrors PoseEstimator.__init__ kwargs (pose_estimator.py:19-32) plus the
 * constants hard-coded at the reference's cv2 call sites. */
typedef struct rpe_config {
    int32_t abi_version;      /* RPE_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    int32_t width, height;    /* image size served by this handle */
    int32_t max_batch;        /* max pairs per call */
    int32_t feature_method;   /* RPE_FEATURE_ORB        (pose_estimator.py:22) */
    int32_t norm_type;        /* RPE_NORM_HAMMING       (pose_estimator.py:23) */
    int32_t max_matches;      /* default 500            (pose_estimator.py:24); 5 .. 8064; >= nfeatures+64 (the keypoint capacity) = "no truncation" (:150-151) */
    int32_t nfeatures;        /* default 4000           (pose_estimator.py:25): ORB 1 .. 8000.  SIFT: 0 = no cap, what the reference's
                                 cv2.SIFT_create() (pose_estimator.py:93-94) does -- arrays then hold RPE_SIFT_UNCAPPED_CAPACITY
                                 keypoints per image and RPE_OVF_SIFT_KEYPOINTS reports an image that has more; 1 .. 16320 = SIFT_create(nfeatures) */
    int32_t fast_threshold;   /* 15                     (pose_estimator.py:89) */
    int32_t ransac_max_iters; /* 1000 (cv2 default maxIters) */
    double  ransac_prob;      /* 0.999                  (pose_estimator.py:525) */
    double  ransac_threshold; /* 1.0 px                 (pose_estimator.py:526) */
    int32_t match_mode;       /* RPE_MATCH_CROSSCHECK   (pose_estimator.py:131) */
    int32_t stl_runtime;      /* RPE_STL_LIBSTDCXX: cv2's keypoint order on the reference's Linux wheels (see above) */
    double  match_ratio;      /* Lowe ratio for RPE_MATCH_RATIO (default 0.75; unused by the reference mode) */
} rpe_config;

typedef struct rpe_handle rpe_handle;

/* ORB keypoint record returned by the stage API (cv2.KeyPoint fields the path uses) */
typedef struct rpe_keypoint {
    float x, y;          /* kp.pt  (level coordinates * level scale) */
    float angle;         /* kp.angle, degrees */
    float response;      /* kp.response (Harris) */
    int32_t octave;      /* kp.octave */
    int32_t lx, ly;      /* integer coordinates inside the pyramid level */
} rpe_keypoint;

/* SIFT keypoint record (cv2.KeyPoint fields), stage API */
typedef struct rpe_sift_keypoint {
    float x, y;          /* kp.pt in input-image coordinates */
    float size;          /* kp.size */
    float angle;         /* kp.angle, degrees */
    float response;      /* kp.response = |contrast| */
    int32_t octave;      /* kp.octave, OpenCV's packed (octave | layer<<8 | offset<<16) form */
} rpe_sift_keypoint;

/* ------------------------------------------------------------ lifecycle */
void rpe_default_config(rpe_config *cfg);
/* replaces PoseEstimator.__init__ / _create_feature_extractor / _create_matcher
 * (pose_estimator.py:19-69, :75-96, :115-131) */
int rpe_create(const rpe_config *cfg, rpe_handle **out);
void rpe_destroy(rpe_handle *h);
const char *rpe_last_error(const rpe_handle *h); /* h may be NULL: last create error */
int rpe_device_count(void);
/* capacity of per-image keypoint arrays used by the stage API */
int rpe_keypoint_capacity(const rpe_handle *h);

/* ------------------------------------------------------- device buffers */
/* thin wrappers so a ctypes host can keep image batches resident in HBM */
int rpe_device_malloc(rpe_handle *h, size_t bytes, void **d_ptr);
int rpe_device_free(rpe_handle *h, void *d_ptr);
int rpe_memcpy_h2d(rpe_handle *h, void *d_dst, const void *h_src, size_t bytes);
int rpe_memcpy_d2h(rpe_handle *h, void *h_dst, const void *d_src, size_t bytes);
int rpe_synchronize(rpe_handle *h);
/* page-locked host memory for image batches handed to rpe_estimate_batch / rpe_estimate_stream (the reference's callers
 * hold numpy arrays from cv2.imread, src/utils/image_loader.py:23-28): uploads from pinned memory do not block the
 * calling thread and run at the full PCIe rate.  rpe_host_register pins a buffer the caller already owns. */
int rpe_host_alloc(rpe_handle *h, size_t bytes, void **h_ptr);
int rpe_host_free(rpe_handle *h, void *h_ptr);
int rpe_host_register(rpe_handle *h, void *h_ptr, size_t bytes);
int rpe_host_unregister(rpe_handle *h, void *h_ptr);

/* ------------------------------------------------------------- hot path */
/* replaces PoseEstimator.estimate (pose_estimator.py:487-533) for B pairs.
 * h_imgs1/h_imgs2: B images each (host).  Outputs (host, caller-allocated):
 * R[B*9], t[B*3], inliers[B] (= recoverPose return value, :621),
 * n_matches[B] (= len(matches), :627; may be NULL), status[B].
 * Large host batches (B >= 512 and >= 64 MiB per image set) are processed in four chunks whose uploads run on a
 * copy stream behind the kernels of the previous chunk; results are identical, but the per-pair debug arrays
 * (rpe_fetch_matched_points) then hold nothing usable and that call reports an error. */
int rpe_estimate_batch(rpe_handle *h, const uint8_t *h_imgs1, const uint8_t *h_imgs2, int B,
                       const double K[9], double *R, double *t, int32_t *inliers,
                       int32_t *n_matches, int32_t *status);
/* same, images already resident in HBM (the timed configuration) */
int rpe_estimate_batch_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B,
                              const double K[9], double *R, double *t, int32_t *inliers,
                              int32_t *n_matches, int32_t *status);
/* asynchronous form: enqueue on the handle's stream, results stay on the
 * device until rpe_fetch_results(); lets the host overlap the next upload.
 * The image batches are READ IN PLACE by the ORB kernels (level 0 of the pyramid is the input itself when the
 * width is a multiple of 16 and the batches are 16-byte aligned; other shapes are copied first): they must stay
 * valid and unmodified until rpe_fetch_results() / rpe_synchronize() returns -- and until rpe_orb_debug_fetch()
 * if that is called afterwards. */
int rpe_enqueue_batch_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B,
                             const double K[9]);
int rpe_fetch_results(rpe_handle *h, int B, double *R, double *t, int32_t *inliers,
                      int32_t *n_matches, int32_t *status);
/* RPE_OVF_* flags of the last batch / stream, one word per pair (the OR of its two images' flags) */
int rpe_fetch_overflow(rpe_handle *h, int n_pairs, uint32_t *flags);
/* Consecutive-frame stream = the pair loop of BatchProcessor.process_sequence (reference
 * src/core/batch_processor.py:71-109): F frames -> F-1 relative poses (frame i -> i+1), features
 * extracted once per frame.  F <= 2*max_batch, F-1 <= max_batch.  Outputs sized F-1. */
int rpe_estimate_stream(rpe_handle *h, const uint8_t *h_frames, int F, const double K[9],
                        double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status);
int rpe_enqueue_stream_device(rpe_handle *h, const uint8_t *d_frames, int F, const double K[9]);

/* ---------------------------------------------------------- frame store */
/* Extraction separated from pairing (NOT in the reference, whose only shapes are the pair and the consecutive-frame
 * sequence): per-frame features -- keypoint points, count, descriptors, the L2 matcher's norm words, RPE_OVF_* flags --
 * stay resident in HBM slots across calls, and a pair list names two slots per pair.  Windowed matching (frame i
 * against i+1 .. i+k), loop-closure candidates (rpe_frames_similar below proposes them) and online use (put the new
 * frame, pair it with the ring of the last k) extract every frame once.  The store is created on demand and survives every other call on the handle (batch,
 * stream, stage API, refinement); rpe_destroy frees it.  Bytes per slot:
 * (nfeatures + 64) * (descriptor bytes + 8 + N) + 8, descriptor bytes = 32 (ORB) or 128 (SIFT), N = 8 for NORM_L2 handles
 * of either match mode (the crossCheck matcher and rpe_guided_matches_l2 read the norm words) and 0 for Hamming handles,
 * nfeatures = RPE_SIFT_UNCAPPED_CAPACITY for uncapped SIFT.
 * rpe_frames_reserve: n_slots = 0 frees; growing or shrinking keeps the slots below the new size (it waits for the
 * handle's stream) and ends the pair list's claim on rpe_fetch_overflow, which is refused until the next batch, stream or
 * pair list.  RPE_ERR_HIP when the device cannot hold the new store: the old one is kept. */
int rpe_frames_reserve(rpe_handle *h, int n_slots);
int rpe_frames_capacity(const rpe_handle *h);
/* extracts n frames (n <= 2*max_batch) and keeps them in slots[0..n) (host array, distinct, inside the store); a slot
 * filled before is replaced.  The keypoint order of rpe_config.stl_runtime is a property of the extraction and so of
 * the slot.  _device form: asynchronous on the handle's stream; the frames are read in place like
 * rpe_enqueue_batch_device's and must stay valid until the next synchronising call.  rpe_frames_put stages host frames
 * through the handle's own upload buffers.  slots[] may be reused as soon as the call returns.  Like a stage-API call,
 * a put overwrites the extraction workspace: rpe_fetch_overflow / rpe_fetch_structure / rpe_refine_poses are refused
 * until the next batch, stream or pair list.
 * RPE_ERR_INVALID: no store, slot outside the store, a slot twice in one put.  RPE_ERR_CAPACITY: n > 2*max_batch. */
int rpe_frames_put_device(rpe_handle *h, const uint8_t *d_frames, int n, const int32_t *slots);
int rpe_frames_put(rpe_handle *h, const uint8_t *h_frames, int n, const int32_t *slots);
/* keypoint count (-1 = slot never filled; 0 = a frame without keypoints) and RPE_OVF_* flags of n slots; either
 * output may be NULL.  Synchronises the handle's stream. */
int rpe_frames_info(rpe_handle *h, int n, const int32_t *slots, int32_t *counts, uint32_t *flags);
/* hot path over the store: P pairs (P <= max_batch), pair p = (slot1[p], slot2[p]); any slots, repeats, reversed and
 * self pairs allowed.  match -> findEssentialMat -> recoverPose exactly as a batch runs them: the result of pair (a, b)
 * is bit for bit what rpe_estimate_batch_device returns for the frame put into slot a against the frame put into
 * slot b.  Afterwards the pair list is "the last batch" of rpe_fetch_results(P), rpe_fetch_matched_points,
 * rpe_fetch_structure, rpe_refine_poses, rpe_gather_poses and rpe_fetch_overflow (flags of slot1[p] | slot2[p]).
 * A frame without keypoints gives its pairs RPE_PAIR_NO_DESCRIPTORS.  slot1 / slot2 may be reused as soon as the call
 * returns.  rpe_get_stage_ms reports match / ransac / pose and zero for the extraction stages.
 * RPE_ERR_INVALID: no store, slot outside the store, empty slot.  RPE_ERR_CAPACITY: P > max_batch.  Nothing is
 * launched and the handle stays usable after either. */
int rpe_enqueue_pairs(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P, const double K[9]);
int rpe_estimate_pairs(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P, const double K[9],
                       double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status);

/* ---------------------------------------------------------- camera models */
/* Per-frame camera: pinhole intrinsics plus cv2's Brown-Conrady / rational lens (NOT in the reference, which has one K
 * and pinhole points).  The geometry stages of the *_cameras calls below normalise every matched point p (f32 pixel,
 * converted to f64 first) with the camera of ITS frame: xd = (p.x - cx) / fx, yd = (p.y - cy) / fy, then -- unless all
 * eight coefficients are zero -- cv2.undistortPoints' fixed-point iteration started at (xd, yd), exactly
 * RPE_UNDISTORT_ITERS times, in f64 and in this operation order:
 *     r2  = x*x + y*y
 *     icd = (1 + r2*(k4 + r2*(k5 + r2*k6))) / (1 + r2*(k1 + r2*(k2 + r2*k3)))
 *     dx  = 2*p1*x*y + p2*(r2 + 2*x*x);   dy = p1*(r2 + 2*y*y) + 2*p2*x*y
 *     x   = (xd - dx) * icd;              y  = (yd - dy) * icd
 * A camera whose dist is all zero skips the iteration: its normalised point is bit for bit the single-K path's.  The
 * count is fixed (cv2's default criterion; results stay bit-deterministic): after five iterations the residual at the
 * corner of a VGA image is 1e-4 px for (k1, k2, p1, p2, k3) = (-0.12, 0.03, 0.0008, -0.0005, 0) and 0.035 px for
 * (-0.28, 0.09, 0.001, -0.0008, -0.01).  Where a focal length is a scale -- the RANSAC threshold
 * (ransac_threshold / f) and the pixel scale of the refinement -- a pair uses the mean of its two cameras,
 * f = (((fx1 + fy1) / 2) + ((fx2 + fy2) / 2)) / 2, which for equal cameras is the single-K value exactly.
 * All images of a handle have one size; cameras differ in parameters only.  Triangulated points stay in the camera-1
 * frame at |t| = 1.  Every call validates its cameras before anything is launched: a non-finite field, fx <= 0 or
 * fy <= 0 is RPE_ERR_INVALID and leaves the handle usable. */
#define RPE_UNDISTORT_ITERS 5
typedef struct rpe_camera {      /* 96 bytes */
    double fx, fy, cx, cy;       /* K[0], K[4], K[2], K[5]; skew is ignored, as everywhere in this library */
    double dist[8];              /* cv2 order: k1 k2 p1 p2 k3 k4 k5 k6; all zero = pinhole */
} rpe_camera;

/* cameras of n frame-store slots (host arrays; slots inside the store, filled or not).  A slot keeps its camera across
 * calls, across a later put of the same slot and across rpe_frames_reserve (slots below the new size); a slot never
 * given one has no camera.  Ends the claim of a camera pair list on rpe_fetch_structure / rpe_refine_poses. */
int rpe_frames_set_cameras(rpe_handle *h, int n, const int32_t *slots, const rpe_camera *cams);
/* rpe_enqueue_pairs / rpe_estimate_pairs with every pair on the cameras of its two slots, resolved on the device.
 * RPE_ERR_INVALID, nothing launched, handle usable, when a named slot has no camera.  (rpe_enqueue_pairs itself ignores
 * slot cameras.)  Afterwards the list is "the last batch" exactly as after rpe_enqueue_pairs; rpe_fetch_matched_points
 * returns the raw, distorted pixels of the matches. */
int rpe_enqueue_pairs_cameras(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P);
int rpe_estimate_pairs_cameras(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P,
                               double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status);
/* the batch forms with cam1[B] (cameras of imgs1) and cam2[B] (of imgs2) in place of K; plain launches for every B (no
 * graph replay).  Afterwards the batch is "the last batch" of rpe_fetch_results, rpe_fetch_matched_points (raw,
 * distorted pixels), rpe_fetch_structure, rpe_refine_poses, rpe_gather_poses and rpe_fetch_overflow.
 * rpe_estimate_batch_cameras (host images) does not chunk: a batch large enough for rpe_estimate_batch's chunked upload
 * (B >= 512 and >= 64 MiB per image set) is refused with RPE_ERR_INVALID; upload it and call the _device form. */
int rpe_enqueue_batch_cameras_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B,
                                     const rpe_camera *cam1, const rpe_camera *cam2);
int rpe_estimate_batch_cameras_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B,
                                      const rpe_camera *cam1, const rpe_camera *cam2, double *R, double *t,
                                      int32_t *inliers, int32_t *n_matches, int32_t *status);
int rpe_estimate_batch_cameras(rpe_handle *h, const uint8_t *h_imgs1, const uint8_t *h_imgs2, int B,
                               const rpe_camera *cam1, const rpe_camera *cam2, double *R, double *t,
                               int32_t *inliers, int32_t *n_matches, int32_t *status);
/* stage forms for callers with their own matches.  rpe_undistort_points: n f32 pixels (x, y) of one camera ->
 * out_xy[2n] f64 normalised, undistorted coordinates (host arrays), the values the geometry stages work on.  The other
 * three are rpe_find_essential / rpe_recover_pose / rpe_refine_pose_points with cam1[B], cam2[B] for K. */
int rpe_undistort_points(rpe_handle *h, const float *h_pts, int n, const rpe_camera *cam, double *h_out_xy);
int rpe_find_essential_cameras(rpe_handle *h, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                               const rpe_camera *cam1, const rpe_camera *cam2, double *E, uint8_t *mask,
                               int32_t *found, int32_t *info);
int rpe_recover_pose_cameras(rpe_handle *h, const double *h_E, const float *h_pts1, const float *h_pts2,
                             const int32_t *m, int B, const rpe_camera *cam1, const rpe_camera *cam2,
                             double *R, double *t, int32_t *inliers);
int rpe_refine_pose_points_cameras(rpe_handle *h, const double *h_R0, const double *h_t0, const float *h_pts1,
                                   const float *h_pts2, const uint8_t *h_mask, const int32_t *m, int B,
                                   const rpe_camera *cam1, const rpe_camera *cam2, int max_iters, double *R, double *t,
                                   int32_t *inliers, int32_t *info, double *rms);

/* Image ingest, the step before the path (reference src/utils/image_loader.py:23-28:
 * cv2.imread -> BGR, cv2.cvtColor(BGR2GRAY)): interleaved 3-channel uint8 images -> gray with cv2's
 * fixed-point weights, gray = (B*3735 + G*19235 + R*9798 + 16384) >> 15, on the handle's stream.
 * order: RPE_ORDER_BGR (cv2.imread layout) or RPE_ORDER_RGB (PIL layout).  n_pixels = total pixels
 * of all images (tightly packed).  The *_device form is asynchronous: its output can be handed
 * straight to rpe_enqueue_batch_device / rpe_enqueue_stream_device. */
enum { RPE_ORDER_BGR = 0, RPE_ORDER_RGB = 1 };
int rpe_bgr_to_gray_device(rpe_handle *h, const uint8_t *d_bgr, size_t n_pixels, int order, uint8_t *d_gray);
int rpe_bgr_to_gray(rpe_handle *h, const uint8_t *h_bgr, size_t n_pixels, int order, uint8_t *h_gray);

/* VP-refinement post-step (pose_estimator.py:160-175 _detect_lsd_lines): line segments of one gray image,
 * cv2.createLineSegmentDetector(LSD_REFINE_STD).detect(gray) restated (csrc/lsd_host.cpp).  Host code:
 * the reference runs this step on the CPU after the pose, and so does this library; it needs no handle.
 * h_lines[capacity*4] receives (x1, y1, x2, y2) per segment; *n_lines is the number found (may exceed
 * capacity: only the first `capacity` are stored). */
int rpe_lsd_detect(const uint8_t *h_gray, int width, int height, float *h_lines, int capacity, int32_t *n_lines);

/* matched point arrays of the last batch (estimate_with_debug's pts1/pts2,
 * pose_estimator.py:606-607,628-629): pts[B*max_matches*2] f32 */
int rpe_fetch_matched_points(rpe_handle *h, int B, float *pts1, float *pts2);

/* Per-match results of the last rpe_estimate_batch / rpe_estimate_batch_device / rpe_enqueue_batch_device /
 * rpe_estimate_stream / rpe_enqueue_stream_device call, pair p at offset p*max_matches (points: *3).
 * ransac_mask: findEssentialMat's inlier mask (pose_estimator.py:522-527); pose_mask: recoverPose's cheirality
 * mask of the returned (R, t), distanceThresh 50 (:533), sum == inliers[p]; points: triangulated point of every
 * match, camera-1 frame, |t| = 1 scale.  Zero past n_matches[p] and for pairs whose status is not OK.
 * Any output may be NULL.  RPE_ERR_INVALID after a chunked host batch, after a stage-API call, or for
 * B > pairs of the last batch. */
int rpe_fetch_structure(rpe_handle *h, int B, uint8_t *ransac_mask, uint8_t *pose_mask, double *points);

/* per-pair outcome of a refinement (info[4 * p]) */
enum {
    RPE_REFINE_OK = 0,        /* refined pose returned */
    RPE_REFINE_SKIPPED = 1,   /* pair status not OK, or fewer than 6 RANSAC inliers: input pose returned */
    RPE_REFINE_REJECTED = 2   /* refined pose lost cheirality inliers or was not finite: input pose returned */
};

/* Non-linear refinement of the poses of the last batch / stream (same validity rules as rpe_fetch_structure):
 * Levenberg-Marquardt on the Sampson error of E = [t]x R over findEssentialMat's inliers, starting from
 * recoverPose's (R, t); 5 parameters (rotation increment, step of t on the unit sphere), at most max_iters
 * (1 ... 100) iterations, the cost never increases.  NOT in the reference.  Does not modify the batch's own
 * results: rpe_fetch_results / rpe_fetch_structure / rpe_gather_poses afterwards still return the unrefined pose.
 * Bit-deterministic run to run like every other call (no floating-point atomics).
 * Outputs (host, any may be NULL): R[B*9], t[B*3], inliers[B] (cheirality count of the returned pose),
 * info[B*4] = {RPE_REFINE_* code, iterations run, residuals used, accepted steps},
 * rms[B*2] = {before, after} root-mean-square Sampson distance in pixels (the scale of
 * rpe_config.ransac_threshold) of the input and of the returned pose over the residuals used.
 * RPE_ERR_INVALID after a chunked host batch, after a stage-API call, for B > pairs of the last batch and for
 * max_iters outside 1 ... 100. */
int rpe_refine_poses(rpe_handle *h, int B, int max_iters, double *R, double *t, int32_t *inliers,
                     int32_t *info, double *rms);

/* ------------------------------------------------------------ scale links */
/* keypoint indices of the matches of the last batch / stream / pair list: qidx into image 1's keypoints, tidx into
 * image 2's, [B * max_matches], -1 past n_matches[p].  Validity rules of rpe_fetch_matched_points.  Either output may be
 * NULL.  (A pair list's keypoints are those of its two slots; rpe_fetch_matched_points returns their coordinates.) */
int rpe_fetch_match_indices(rpe_handle *h, int B, int32_t *qidx, int32_t *tidx);

/* Relative scale of two pairs of the last run that share a frame (NOT in the reference, which never relates two of its
 * estimates): every pose comes back with |t| = 1, so the poses of pairs (i, i+1) and (i+1, i+2) of a stream, or of the
 * pairs of a window, cannot be composed.  A keypoint of the shared frame that both pairs matched and triangulated lies
 * at distance d_a from the frame's camera centre on pair a's scale and d_b on pair b's; d_a / d_b is the baseline of
 * pair b in units of the baseline of pair a.
 * L links over the last run.  Link l joins pairs pair_a[l] != pair_b[l] of that run at a frame they share:
 * side[l] bit 0 = the shared frame is image 2 of pair_a (else image 1), bit 1 = the same for pair_b.
 * stats[3 l .. 3 l + 2] = lower quartile, median, upper quartile of d_a / d_b over the shared keypoints
 *   = baseline of pair_b in units of the baseline of pair_a;
 * n_shared[l]; code[l] = RPE_LINK_*.  Any output may be NULL.
 *  - usable match: match i of a pair is usable when the pair's status is RPE_PAIR_OK, i < n_matches, and both
 *    ransac_mask[i] and pose_mask[i] (rpe_fetch_structure) are set.  Its key is its keypoint index on the shared frame:
 *    qidx when that frame is the pair's image 1, tidx when it is image 2.
 *  - duplicate keys (RPE_MATCH_RATIO lets several matches of a pair name one train keypoint): the usable match with the
 *    lowest match index wins, in both pairs.
 *  - shared set: the keys that have a usable match in both pairs.
 *  - distance: X = the match's triangulated point (camera-1 frame of its pair, |t| = 1).  (x, y, z) = X when the shared
 *    frame is the pair's image 1, R X + t when it is image 2, each row summed as ((r0*X + r1*Y) + r2*Z) + t;
 *    d = sqrt((x*x + y*y) + z*z); the ratio is d_a / d_b.  f64, no contraction.
 *  - order statistics: r[0 .. n) = the ratios sorted ascending; the outputs are r[(n-1)/4], r[(n-1)/2], r[(3*(n-1))/4]
 *    (integer division): elements of the set, never an average.
 *  - codes: RPE_LINK_PAIR_FAILED when either pair's status is not OK (n_shared = 0, stats zero); RPE_LINK_TOO_FEW when
 *    n_shared < min_shared (n_shared reported, stats zero); otherwise RPE_LINK_OK.
 * Validity rules of rpe_fetch_structure (refused after a chunked host batch, a stage call, a put, ...); the structure
 * kernels are launched when the per-match buffers do not hold their results yet.  Changes none of the run's results:
 * rpe_fetch_results / rpe_fetch_structure / rpe_refine_poses / rpe_gather_poses return the same bits afterwards.
 * Bit-deterministic.  Works unchanged after the *_cameras runs: the triangulated points are in normalised coordinates.
 * Argument checks are host-side; nothing is launched and the handle stays usable after a refusal.  RPE_ERR_INVALID: an
 * index outside the last run, pair_a[l] == pair_b[l], side outside 0 .. 3, min_shared < 1, L < 0, a frame that is not
 * shared -- pair list: slot (side bit ? slot2 : slot1) of the two pairs must be equal (refused once the store was
 * resized); stream: pair_a + (side & 1) == pair_b + (side >> 1) -- and any link over a batch, whose pairs share no
 * frame.  RPE_ERR_CAPACITY: L > 4 * max_batch. */
enum { RPE_LINK_OK = 0, RPE_LINK_PAIR_FAILED = 1, RPE_LINK_TOO_FEW = 2 };
int rpe_scale_links(rpe_handle *h, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side,
                    int min_shared, double *stats, int32_t *n_shared, int32_t *code);

/* ------------------------------------------------------- guided matching */
/* Matches of the last batch / stream / pair list again, under the epipolar gate of a pose (guided matching; NOT in the
 * reference, whose only match rule is the brute-force crossCheck): the mutual nearest neighbour among the keypoint
 * pairs that are consistent with (R, t).  rpe_guided_matches / rpe_match_hamming_guided serve Hamming handles only (ORB +
 * RPE_NORM_HAMMING); L2 handles have rpe_guided_matches_l2 / rpe_match_l2_guided below, whose distance is an f32 and whose
 * bound is a double.  Either match_mode of a handle is served: the guided rule is always the mutual one.
 * The rule, for a pair with pose (R, t), images 1 and 2, keypoints i < n1, j < n2 (n = min(count, capacity)); all
 * arithmetic f64, no contraction:
 *  1. x1_i = (x, y) = the f32 keypoint pixel of i normalised with the camera of image 1 as the geometry stages do it
 *     (((double)p.x - cx) / fx, ((double)p.y - cy) / fy, then the undistortion of "camera models"); x2_j for image 2.
 *  2. E = [t]x R: E[r][c] = t[(r+1)%3] * R[(r+2)%3][c] - t[(r+2)%3] * R[(r+1)%3][c].
 *  3. per query i: l_k = (E[k][0]*x + E[k][1]*y) + E[k][2], k = 0, 1, 2; s1_i = l_0*l_0 + l_1*l_1.
 *     per train j: m_k = (E[0][k]*x + E[1][k]*y) + E[2][k], k = 0, 1; s2_j = m_0*m_0 + m_1*m_1.
 *  4. gate (Sampson, findEssentialMat's inlier test): v = (l_0*x2 + l_1*y2) + l_2; (i, j) is admissible iff
 *     v*v <= thr2 * (s1_i + s2_j) and hamming(i, j) <= max_distance, thr = gate_px / f, thr2 = thr*thr, f = the focal
 *     scale RANSAC uses ((fx + fy) / 2, or the mean of that over the pair's two cameras).  A comparison with a NaN is
 *     false.
 *  5. NNt(i) = the admissible j with the least (hamming, j), NNq(j) = the admissible i with the least (hamming, i);
 *     (i, NNt(i)) is a match iff NNq(NNt(i)) == i.  Output: the matches sorted ascending by (hamming, i), the first
 *     max_matches of them.
 * With no effective gate (gate_px = 1e9, max_distance = 256) this is the crossCheck result bit for bit, and a
 * crossCheck match that is admissible is always a guided match before truncation.
 * R[B*9], t[B*3] (host): the poses to gate with -- refined poses, a prior from a trajectory -- and every pair is
 * matched whatever its status.  R == t == NULL: the run's own poses; a pair whose status is not RPE_PAIR_OK then gets
 * n_matches = 0.  The cameras are the run's own (its K, or the cameras of a *_cameras run).
 * Outputs (host, any may be NULL), sized like the run's: qidx / tidx / dist [B*max_matches], pts1 / pts2
 * [B*max_matches*2] (the keypoints the indices name), n_matches[B]; -1 (indices, dist) and zero (points) past
 * n_matches[p].  The results live in buffers of their own: rpe_fetch_results, rpe_fetch_matched_points,
 * rpe_fetch_match_indices, rpe_fetch_structure, rpe_refine_poses, rpe_scale_links and rpe_gather_poses return the same
 * bits afterwards.  Bit-deterministic.
 * Validity rules of rpe_fetch_structure: refused after a chunked host batch, a stage call, a put, once the store was
 * resized under a pair list, and for B > pairs of the last run.  RPE_ERR_INVALID as well: an L2 handle, gate_px not
 * finite or <= 0, max_distance outside 0 .. 256, a non-finite entry of R or t, exactly one of R, t NULL.  All checks
 * are host-side; nothing is launched and the handle stays usable after a refusal. */
int rpe_guided_matches(rpe_handle *h, int B, const double *R, const double *t, double gate_px, int max_distance,
                       int32_t *qidx, int32_t *tidx, int32_t *dist, float *pts1, float *pts2, int32_t *n_matches);

/* The same for RPE_NORM_L2 handles (SIFT, or ORB bytes under L2; either match_mode).  Steps 1 - 4 of the rule above hold
 * unchanged as far as the gate goes (the normalisation, E, l_k, s1, s2, v, thr2; a comparison with a NaN is false); the
 * rest reads:
 *  4'. dist(i, j) is the matcher's own distance: the f32 sqrtf((float)S), S the exact integer sum of squared byte
 *      differences of the two descriptors (128 bytes for SIFT handles, 32 for ORB handles created with RPE_NORM_L2).
 *      (i, j) is admissible iff it passes the gate and (double)dist(i, j) <= max_distance.
 *  5'. NNt(i) = the admissible j with the least (dist, j), compared as f32 and then by index; NNq(j) = the admissible i with
 *      the least (dist, i); (i, NNt(i)) is a match iff NNq(NNt(i)) == i.  Output: the matches sorted ascending by
 *      (dist, i), the first max_matches of them.
 * With no effective gate (gate_px = 1e9, max_distance = +inf) this is the crossCheck result of rpe_match_l2 bit for bit,
 * and a crossCheck match that is admissible is always a guided match before truncation.
 * R, t, the run's own poses for R == t == NULL, the cameras and the output shapes are those of rpe_guided_matches; dist is
 * f32.  Past n_matches[p]: -1 (indices), zero (points), and dist holds all-ones bits (0xFFFFFFFF, a NaN: compare the bits
 * or slice by n_matches).  The results live in the same buffers of their own, and every fetch of the run returns the same
 * bits afterwards.  Bit-deterministic.
 * Validity rules of rpe_guided_matches.  RPE_ERR_INVALID as well: a handle that is not RPE_NORM_L2, gate_px not finite or
 * <= 0, max_distance NaN or < 0 (+inf is allowed and means no bound), a non-finite entry of R or t, exactly one of R, t
 * NULL.  All checks are host-side; nothing is launched and the handle stays usable after a refusal. */
int rpe_guided_matches_l2(rpe_handle *h, int B, const double *R, const double *t, double gate_px, double max_distance,
                          int32_t *qidx, int32_t *tidx, float *dist, float *pts1, float *pts2, int32_t *n_matches);

/* ------------------------------------------- homography / rotation-only */
/* A second geometric model over the matches of a pair (NOT in the reference, whose only model is the essential matrix):
 * a homography by RANSAC over the run's own subset stream, and a rotation fitted to the homography's inliers.  Under a
 * pure rotation, or a baseline far below the scene depth, findEssentialMat -> recoverPose is degenerate and reports
 * RPE_PAIR_OK all the same; there the homography explains most matches and the fitted rotation explains as many, while
 * on a general scene both explain few.  counts[] puts the three inlier counts side by side; what ratio of them names a
 * pair "rotation-only" or "planar" is the caller's policy (geometry.classify_pair).
 * The rule, for one pair.  All arithmetic f64, no contraction; a comparison with a NaN is false.
 *  Inputs: matches i < M with the normalised points a_i = (x, y) of image 1 and b_i of image 2 exactly as the geometry
 *   stages use them (normalised with K or, after a *_cameras run, normalised and undistorted with the camera of each
 *   frame).  thr = threshold_px / f, f = the focal scale RANSAC uses ((fx + fy) / 2, or the mean of that over the pair's
 *   two cameras); thr2 = thr * thr (a double; no float cast).
 *  Helpers: p = (x, y, 1); cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0); dot(a, b) = (a0*b0 + a1*b1) + a2*b2;
 *   adj(A) = the matrix with rows cross(c1, c2), cross(c2, c0), cross(c0, c1), c0 c1 c2 the columns of A.
 *  Sample: iteration it < iters takes the first four of the five indices of findEssentialMat's subset stream for M
 *   (ptsetreg.cpp getSubset, RNG seeded (uint64)-1; the stream depends on M alone): points p0 .. p3 of image 1 and
 *   q0 .. q3 of image 2.
 *  Four-point model, closed form, no pivoting:
 *   lambda = (dot(cross(p1, p2), p3), dot(cross(p2, p0), p3), dot(cross(p0, p1), p3)); A = the matrix with columns
 *   lambda_k * p_k (A[r][k] = lambda_k * p_k[r]); mu and B the same from q; J = adj(A);
 *   H[r][c] = (B[r][0]*J[0][c] + B[r][1]*J[1][c]) + B[r][2]*J[2][c]; n = sqrt(the sum of the nine squares H[r][c]*H[r][c],
 *   row-major, added left to right); every entry is divided by n.  The model is invalid when a lambda_k or a mu_k
 *   equals 0 or an entry after the division is not finite.  Gauge: H is negated when
 *   (H[2][0]*x + H[2][1]*y) + H[2][2] < 0 at p0.  G = adj(H) (not divided by the determinant), negated by the same test
 *   at q0.
 *  Transfer test T(F, p -> q): u = (F[0][0]*x + F[0][1]*y) + F[0][2], v and w likewise from rows 1 and 2 at p = (x, y);
 *   dx = u - qx*w, dy = v - qy*w; true iff w > 0 and (dx*dx + dy*dy) <= thr2 * (w*w).  No division.
 *   Match i is an inlier of H iff T(H, a_i -> b_i) and T(G, b_i -> a_i).
 *  Election: all `iters` samples are evaluated (no early stop: the counts do not depend on how the work is launched); the
 *   winner is the valid model with the most inliers, ties to the lowest iteration; mask = the winner's inlier set.
 *  Rotation fit over the winner's inliers: bearings a^ = (x, y, 1) / sqrt((x*x + y*y) + 1), b^ likewise;
 *   C[r][c] = sum of b^_r * a^_c, added in this fixed order: lane l of 256 adds its inliers i = l, l + 256, ... in
 *   ascending order starting from 0; inside each group of 64 lanes the partial sums are combined by the butterfly
 *   v += v(lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; the four group totals are added as ((g0 + g1) + g2) + g3.
 *   C = U S V^T by the library's one-sided Jacobi SVD (recoverPose's), singular values sorted descending, u2 = u0 x u1;
 *   R_rot[r][c] = (u0[r]*v0[c] + u1[r]*v1[c]) + (d*u2[r])*v2[c], d = -1 when the determinant of the matrix with rows
 *   v0 v1 v2 is negative and 1 otherwise (= U diag(1, 1, det(U V^T)) V^T).  n_rot = the number of matches i < M with
 *   T(R_rot, a_i -> b_i) and T(R_rot^T, b_i -> a_i), no gauge step, evaluated with exactly the bits of R_rot that are
 *   returned.  A non-finite R_rot is returned as zeros with n_rot = 0.
 *  Codes (info[4 p]): RPE_HOMOGRAPHY_OK; RPE_HOMOGRAPHY_SKIPPED: M < 6 (the subset stream starts at 6) or, batch form, a
 *   pair whose status is not RPE_PAIR_OK; RPE_HOMOGRAPHY_NONE: no valid model.  H, R_rot, mask, n_H, n_rot and the rest
 *   of info are zero for the last two.
 * Outputs (host, any may be NULL): H[B*9] in normalised coordinates (pixels: K2 H K1^-1), unit Frobenius norm, in the gauge
 * above; R_rot[B*9]; mask[B*max_matches], zero past M; counts[B*3] = {n_H, n_rot, n_E}, n_E = findEssentialMat's inlier
 * count of the run (the sum of rpe_fetch_structure's ransac_mask; -1 in the stage form, which runs no essential RANSAC);
 * info[B*4] = {RPE_HOMOGRAPHY_* code, winning iteration, number of valid models, 0}.
 * rpe_pair_homographies: over the first B pairs of the last batch / stream / pair list / *_cameras run.  Validity rules of
 * rpe_fetch_structure: refused after a chunked host batch, a stage call, a put, once the store was resized under a pair
 * list, and for B > pairs of the last run.  The results live in buffers of their own: rpe_fetch_results,
 * rpe_fetch_structure, rpe_refine_poses, rpe_scale_links, rpe_guided_matches(_l2) and rpe_gather_poses return the same bits
 * afterwards.  rpe_find_homography: stage form over the caller's matches (pts as in rpe_find_essential), one K; goes
 * through the workspace like every stage call.
 * RPE_ERR_INVALID: iters outside 1 .. rpe_config.ransac_max_iters, threshold_px not finite or <= 0.  All checks are
 * host-side; nothing is launched and the handle stays usable after a refusal.  Bit-deterministic (no floating-point
 * atomics). */
enum { RPE_HOMOGRAPHY_OK = 0, RPE_HOMOGRAPHY_SKIPPED = 1, RPE_HOMOGRAPHY_NONE = 2 };
int rpe_pair_homographies(rpe_handle *h, int B, int iters, double threshold_px,
                          double *H, double *R_rot, uint8_t *mask, int32_t *counts, int32_t *info);
int rpe_find_homography(rpe_handle *h, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                        const double K[9], int iters, double threshold_px,
                        double *H, double *R_rot, uint8_t *mask, int32_t *counts, int32_t *info);

/* ------------------------------------------------------------ link poses */
/* Absolute pose of a frame against the structure of a linked pair (NOT in the reference, which has no 2D-3D path): for a
 * link (pair a, pair b, shared frame S) pair a's triangulated points are the map, pair b's matches the observations in
 * b's other frame C, and the pose of C is solved by P3P RANSAC.  The result is pair b's relative pose on pair a's scale
 * (|t| is the baseline of pair b in units of the baseline of pair a); it uses pair b's matches only -- neither b's
 * essential matrix nor any parallax in b: a rotation-only pair b gets its rotation and |t| ~ 0.
 * Links: exactly those of rpe_scale_links -- the same side bits, validity rules and refusals (one argument head serves
 * both calls); the structure kernels are launched when the per-match buffers do not hold their results yet.
 * The rule, for one link.  All arithmetic f64, + - * / sqrt only, no contraction; a comparison with a NaN is false;
 * dot(a, b) = (a0*b0 + a1*b1) + a2*b2; cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0); |a| = sqrt(dot(a, a));
 * finite(v) = fabs(v) <= DBL_MAX.
 *  Map side (pair a): pair a's status must be RPE_PAIR_OK, else RPE_LINKPOSE_PAIR_FAILED.  A usable match is as in
 *   rpe_scale_links (i < n_matches, ransac_mask and pose_mask set); its key is its keypoint index on S; the lowest match
 *   index wins a duplicate key.  Its 3D point is the triangulated point (X, Y, Z) taken into S's camera frame by the
 *   expression of "scale links": itself when S is a's image 1, ((r0*X + r1*Y) + r2*Z) + t per row when S is a's image 2.
 *  Observation side (pair b): every match i < n_matches takes part whatever b's masks say; the lowest match index wins
 *   a duplicate key.  Pair b need not be RPE_PAIR_OK: every status leaves n_matches, the match indices and the matched
 *   points defined (the matcher writes them before any status is decided: RPE_PAIR_NO_DESCRIPTORS has n_matches = 0,
 *   RPE_PAIR_INSUFFICIENT_MATCHES fewer than 5 -- both end as RPE_LINKPOSE_TOO_FEW -- and RPE_PAIR_NO_ESSENTIAL /
 *   RPE_PAIR_AMBIGUOUS_ESSENTIAL keep their full match list and are solved like an OK pair), so no status of pair b is
 *   RPE_LINKPOSE_PAIR_FAILED.  The observation q = (qx, qy) is b's point on C (image 2 of b when S is its image 1, else
 *   image 1) in the normalised coordinates the geometry stages use (K, or undistorted with C's camera after a *_cameras
 *   run): the same expression, the same bits.  thr = threshold_px / f, f = pair b's RANSAC focal scale as
 *   rpe_pair_homographies takes it; thr2 = thr * thr (a double).
 *  Correspondences: the keys with an entry on both sides, numbered c = 0 .. n-1 in ascending order of pair b's match
 *   index.  n < max(min_shared, 6): RPE_LINKPOSE_TOO_FEW, n reported, the rest zero.
 *  Sample: iteration it < iters takes the first three of the five indices of findEssentialMat's subset stream for M = n:
 *   points P1 P2 P3 (3D) and q1 q2 q3.
 *  Minimal solver:
 *   bearings j_k = (x/m, y/m, 1/m), m = sqrt((x*x + y*y) + 1) at q_k;
 *   a2 = dot(P2-P3, P2-P3), b2 = dot(P1-P3, P1-P3), c2 = dot(P1-P2, P1-P2); ca = dot(j2, j3), cb = dot(j1, j3),
 *   cg = dot(j1, j2).  With the depths s2 = u s1, s3 = v s1 (ascending coefficients, index = power of v):
 *   Q = (1, q1, 1), q1 = -(2*cb);  m = a2 - c2;  N = (b2 + m, m*q1, m - b2);  D = (d0, d1), d0 = (2*b2)*cg,
 *   d1 = -((2*b2)*ca);  u = N(v) / D(v), and v is a root of b2 N^2 - 2 b2 cg N D + (b2 - c2 Q) D^2, formed as
 *   NN = (n0*n0, 2*(n0*n1), 2*(n0*n2) + n1*n1, 2*(n1*n2), n2*n2);  ND = (n0*d0, n0*d1 + n1*d0, n1*d1 + n2*d0, n2*d1);
 *   DD = (d0*d0, 2*(d0*d1), d1*d1);  W = (b2 - c2, -(c2*q1), -c2);
 *   WD = (w0*dd0, w0*dd1 + w1*dd0, (w0*dd2 + w1*dd1) + w2*dd0, w1*dd2 + w2*dd1, w2*dd2);
 *   c_i = (b2*nn_i - d0*nd_i) + wd_i for i = 0 .. 3, c_4 = b2*nn_4 + wd_4.
 *   Degree = the highest i with c_i != 0 (none or 0: no root); the real roots come from the library's derivative-chain
 *   finder (Fujiwara bound from the binary exponents, sign-change brackets between the roots of the derivative,
 *   safeguarded Newton, Estrin evaluation: findEssentialMat's), ascending, root index r = 0, 1, ...
 *   A root v is a candidate iff v > 0, Dv = d0 + d1*v != 0, u = Nv / Dv > 0 with Nv = (n0 + n1*v) + n2*(v*v),
 *   Qv = (1 + q1*v) + v*v > 0, and every entry of the R and t below is finite.
 *   Depths s1 = sqrt(b2 / Qv), s2 = u*s1, s3 = v*s1; Y_k = s_k * j_k.  Frames: e1 = (P2-P1) / |P2-P1|,
 *   e3 = cross(e1, P3-P1) / |cross(e1, P3-P1)|, e2 = cross(e3, e1); f1 f2 f3 the same from Y1 Y2 Y3;
 *   R[r][c] = (f1[r]*e1[c] + f2[r]*e2[c]) + f3[r]*e3[c]; t[r] = Y1[r] - ((R[r][0]*P1[0] + R[r][1]*P1[1]) + R[r][2]*P1[2]).
 *   Collinear or repeated points give non-finite entries and so no candidate.
 *  Score: y = R X + t, each row ((R[r][0]*X + R[r][1]*Y) + R[r][2]*Z) + t[r]; dx = y0 - qx*y2, dy = y1 - qy*y2;
 *   correspondence c is an inlier iff y2 > 0 and (dx*dx + dy*dy) <= thr2 * (y2*y2).  No division.
 *  Election: all `iters` samples are evaluated; the winner is the candidate with the most inliers, ties to the lowest
 *   iteration, then to the lowest root index.  No candidate at all: RPE_LINKPOSE_NONE.
 *  Polish (refine_iters > 0): Levenberg-Marquardt on the reprojection residuals in pixels, two per correspondence,
 *   (f*(y0/y2 - qx), f*(y1/y2 - qy)), over the winner's inlier set, which stays fixed; six parameters (w, d):
 *   R <- exp([w]x) R, t <- t + d; the conventions of rpe_refine_poses (initial damping 1e-3, the step solves
 *   (J'J + lambda diag J'J) step = -J'r by Cholesky and a matrix that is not positive definite counts as a rejection, a
 *   step is accepted only when it strictly lowers the cost, damping / 10 after an accepted step and * 10 after a
 *   rejected one, the same stop tolerances on the cost decrease and the step length, at most refine_iters iterations;
 *   the sums over the inliers in the fixed order of "homography": lane partials, butterfly, wave totals).  The polished pose is
 *   returned only if a step was accepted, it is finite and its inlier count over all n correspondences is not below the
 *   winner's; otherwise the minimal pose is returned.  refine_iters = 0 returns the minimal pose.
 *  Outputs (host, any may be NULL): R[L*9], t[L*3] in pair b's own convention (image 1 -> image 2 of pair b) on pair a's
 *   scale: the solved pose (S -> C) when S is b's image 1; when S is b's image 2 its inverse, R_out[r][c] = R[c][r],
 *   t_out[r] = -((R[0][r]*t[0] + R[1][r]*t[1]) + R[2][r]*t[2]).  mask[L*max_matches], indexed by pair b's match index:
 *   the inliers of the returned pose (scored in the solved form), zero elsewhere.  counts[L*2] = {n, inliers of the
 *   returned pose}.  info[L*4] = {RPE_LINKPOSE_* code, winning iteration, winning root index, polish: the iterations run
 *   when the polished pose is returned, 0 when there was no polish or no accepted step, -1 when the polished pose was
 *   rejected}.  rms[L*2] = root mean square over the winner's m inliers of the residual length in pixels,
 *   sqrt(sum(rx*rx + ry*ry) / m), of the minimal pose and of the returned pose.  For every code but RPE_LINKPOSE_OK
 *   everything except the code and n is zero.
 * The results live in buffers of their own: rpe_fetch_results, rpe_fetch_structure, rpe_refine_poses, rpe_scale_links,
 * rpe_pair_homographies, rpe_guided_matches(_l2) and rpe_gather_poses return the same bits afterwards.  Bit-deterministic
 * (no atomics decide an order, no floating-point atomics).
 * RPE_ERR_INVALID / RPE_ERR_CAPACITY: every refusal of rpe_scale_links, and iters outside 1 .. rpe_config.ransac_max_iters,
 * threshold_px not finite or <= 0, refine_iters outside 0 .. 100.  All checks are host-side; nothing is launched and the
 * handle stays usable after a refusal. */
enum { RPE_LINKPOSE_OK = 0, RPE_LINKPOSE_PAIR_FAILED = 1, RPE_LINKPOSE_TOO_FEW = 2, RPE_LINKPOSE_NONE = 3 };
int rpe_link_poses(rpe_handle *h, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side,
                   int iters, double threshold_px, int min_shared, int refine_iters,
                   double *R, double *t, uint8_t *mask, int32_t *counts, int32_t *info, double *rms);

/* ---------------------------------------------------------- link bundles */
/* Bundle adjustment of the three views of a link (NOT in the reference): for a link (pair a, pair b, shared frame S) with
 * A = pair a's other frame and C = pair b's other frame, the poses S -> A and S -> C and the points both pairs see are
 * refined together on one reprojection cost.  S is the gauge (identity, never moved) and |t_A| = 1 the unit of scale.
 * Links: exactly those of rpe_scale_links / rpe_link_poses (one argument head serves the three calls).
 * The rule, for one link.  All arithmetic f64, + - * / sqrt only (sin for a rotation increment, as rpe_refine_poses), no
 * contraction; a comparison with a NaN is false; finite(v) = fabs(v) <= DBL_MAX.
 *  Codes, tested in this order: pair a not RPE_PAIR_OK: RPE_BUNDLE_PAIR_FAILED, counts {0, 0}.  All nine entries of the
 *   link's R0 zero (what rpe_link_poses returns for every code but OK): RPE_BUNDLE_SKIPPED, counts {n2, 0}.
 *   n3 < max(min_shared, 6): RPE_BUNDLE_TOO_FEW, counts {n2, n3}.  For these three everything else is zero.
 *  Points: the usable matches of pair a as in rpe_scale_links (i < n_matches, ransac_mask and pose_mask set; key = keypoint
 *   index on S; the lowest match index wins a duplicate key), numbered j = 0 .. n2-1 in ascending order of pair a's match
 *   index.  Point j starts at pair a's triangulated point taken into S's frame by the link_point expression of "link
 *   poses".  Its observations on S and on A are pair a's matched points in the normalised coordinates of the geometry
 *   stages (camera path included).  It has an observation on C when its key has a match in pair b (every match
 *   i < n_matches of b takes part whatever b's masks or status say, the lowest index wins) and that correspondence passes
 *   the Score test of "link poses" (y2 > 0, dx*dx + dy*dy <= thr2 * (y2*y2), thr = threshold_px / f_c) under the INPUT
 *   pose of C; n3 counts these points.  The sets are fixed for the whole optimisation.
 *  Start: A from pair a's own (R, t), C from the caller's R0[L*9], t0[L*3] in pair b's own convention on pair a's scale
 *   (what rpe_link_poses returns); each is taken to the solved form (S -> other frame) by the inverse expression of "link
 *   poses" when S is that pair's image 2.
 *  Parameters: 11 for the cameras, d = (wA[3], bA[2], wC[3], dC[3]), and 3 per point.  R_A <- exp([wA]x) R_A,
 *   t_A <- normalise(t_A + bA0*b1 + bA1*b2) with (b1, b2) the tangent basis of rpe_refine_poses at t_A;
 *   R_C <- exp([wC]x) R_C, t_C <- t_C + dC;  X_j <- X_j + dp_j.
 *  Residuals, in pixels, rows in the order S x, S y, A x, A y, C x, C y: f*(y0/y2 - qx), f*(y1/y2 - qy) with y = X on S,
 *   y = R_V X + t_V (each row ((r0*X + r1*Y) + r2*Z) + t) on A and C; f = f_a (pair a's RANSAC focal scale, as
 *   rpe_pair_homographies takes it) on S and A, f_c (pair b's) on C.  A point without the C observation has zero C rows.
 *   cost = sum over the points of ((e0*e0 + e1*e1) + (e2*e2 + e3*e3)) + (e4*e4 + e5*e5).
 *  Derivatives of a row with y = R X + t, a = R X, u = y0/y2 (or y1/y2), s = f/y2: by w as in "link poses" polish, by t:
 *   (s, 0, -s*ux) / (0, s, -s*uy) = Jt; by the tangent step: (Jt . b1, Jt . b2); by X: Jt R (column k:
 *   (Jt0*R[0][k] + Jt1*R[1][k]) + Jt2*R[2][k]); on S, Jt itself.
 *  LM: the conventions of rpe_refine_poses: lambda0 = 1e-3; a step that does not strictly lower the cost (or that cannot
 *   be solved) multiplies lambda by 10, an accepted one divides it by 10; the same two stop tolerances (cost decrease
 *   <= 1e-6 of the cost, |d| of the 11 camera parameters <= 1e-9); at most max_iters iterations.  The step solves
 *   (J'J + lambda diag J'J) step = -J'r exactly by eliminating the points:
 *    per point V = Jp'Jp (rows added in order) with V_ii <- V_ii + lambda*V_ii; its inverse by the adjugate divided by
 *    det = (v00*c00 + v01*c01) + v02*c02; det > 0 and finite, else the step is rejected; g_p = Jp'e; W = Jc'Jp (11 x 3, the
 *    A rows x A block, the C rows x C block); Y = W V^-1;
 *    U = sum Jc'Jc (block diagonal: no residual sees both cameras), g_c = sum Jc'e;
 *    H = (U + lambda diag U) - sum Y W', g = g_c - sum Y g_p;  H d = -g by the Cholesky of rpe_refine_poses (not positive
 *    definite: rejected);  dp_j = -V^-1 (g_p + W' d), W' d added to g_p in ascending parameter order.
 *   All sums over points run in the fixed order of "homography": lane l of 256 adds its points l, l + 256, ... in
 *   ascending order, then the butterfly, then the four wave totals.  No atomics: bit-deterministic run to run.
 *  Result: the bundled state is returned (RPE_BUNDLE_OK) only if a step was accepted, every pose entry and point
 *   coordinate is finite and every point has positive depth in every view that observes it.  Otherwise
 *   RPE_BUNDLE_REJECTED with the input poses and the input points.
 *  Outputs (host, any may be NULL): R_a[L*9], t_a[L*3]: pair a's pose in pair a's own convention, |t_a| = 1;  R_b, t_b:
 *   pair b's pose in its own convention on pair a's scale (the inverse expression of "link poses" where S is image 2);
 *   points[L*max_matches*3] indexed by pair a's match index, in pair a's camera-1 frame (X itself when S is a's image 1,
 *   R_A X + t_A when it is image 2), the layout of rpe_fetch_structure, zeros for a match that is not a point;
 *   views[L*max_matches]: 0 not a point, 1 seen by S and A, 3 also by C;  counts[L*2] = {n2, n3};
 *   info[L*4] = {RPE_BUNDLE_* code, iterations begun, accepted steps, 0};  rms[L*2] = sqrt(cost / (2*n2 + n3)), the root
 *   mean square residual length in pixels over all observations, of the input state and of the returned state.
 * The results live in buffers of their own, created on first use: every fetch of the run, rpe_refine_poses,
 * rpe_scale_links, rpe_link_poses, rpe_pair_homographies and rpe_guided_matches(_l2) return the same bits afterwards.
 * RPE_ERR_INVALID / RPE_ERR_CAPACITY: every refusal of rpe_scale_links; threshold_px not finite or <= 0; max_iters outside
 * 1 .. 100; exactly one of R0 / t0 NULL, both NULL with L > 0, or a non-finite entry in either.  All checks are host-side;
 * nothing is launched and the handle stays usable after a refusal.
 *
 * rpe_bundle_three_view is the stage form: B problems (B <= max_batch) of n[p] <= max_matches points each, arrays laid out
 * [B][max_matches]: normalised observations obs_s / obs_a / obs_c (two doubles per point; obs_c is read where has_c is
 * set), start points X0 (three doubles, S's frame), start poses in the solved form (Ra0, ta0 with |ta0| = 1: S -> A;
 * Rc0, tc0: S -> C), one focal scale per view pair for the whole call.  No join and no gate: has_c is the caller's, and
 * n3 < 6 is RPE_BUNDLE_TOO_FEW.  Outputs as above, in the solved form and S's frame, points indexed by point number.  It
 * uses the bundle buffers only: the last run stays as it was. */
enum { RPE_BUNDLE_OK = 0, RPE_BUNDLE_PAIR_FAILED = 1, RPE_BUNDLE_TOO_FEW = 2, RPE_BUNDLE_SKIPPED = 3, RPE_BUNDLE_REJECTED = 4 };
int rpe_link_bundles(rpe_handle *h, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side,
                     const double *R0, const double *t0, double threshold_px, int min_shared, int max_iters,
                     double *R_a, double *t_a, double *R_b, double *t_b, double *points, uint8_t *views,
                     int32_t *counts, int32_t *info, double *rms);
int rpe_bundle_three_view(rpe_handle *h, int B, const int32_t *n, const double *obs_s, const double *obs_a,
                          const double *obs_c, const uint8_t *has_c, const double *X0, const double *Ra0, const double *ta0,
                          const double *Rc0, const double *tc0, double f_a, double f_c, int max_iters,
                          double *R_a, double *t_a, double *R_c, double *t_c, double *points, uint8_t *views,
                          int32_t *counts, int32_t *info, double *rms);

/* ------------------------------------------------------ multi-view tracks */
/* Feature tracks of a run (NOT in the reference, which never relates more than two frames): which keypoint of which frame
 * is the same scene point, over all frames of the last stream or pair list, as the connected components of the match
 * graph, with the standard consistency filter (a track holds at most one keypoint per frame).  Integers only.
 * The rule.  KC = rpe_keypoint_capacity(h), P = the pairs of the run, mm = max_matches.
 *  Frames: in a pair list a frame is its slot number and n_frames = rpe_frames_capacity(h); in a stream pair p joins
 *   frames p and p + 1 and n_frames = P + 1.  A batch of two or more pairs is refused: its pairs share no frame.  A batch
 *   of ONE pair cannot be told from a stream of two frames and is served as one: frame 0 is its image 1, frame 1 its
 *   image 2 (rpe_scale_links draws the same line).
 *  Node: (frame f, keypoint index k), 0 <= k < KC; its id is f * KC + k.
 *  Edge: match i of pair p is an edge when (use_pair == NULL or use_pair[p] != 0) and i < n_matches[p] and edge_rule
 *   admits it:
 *    RPE_TRACK_EDGES_USABLE: the usable match of rpe_scale_links: status[p] == RPE_PAIR_OK and both ransac_mask[i] and
 *     pose_mask[i] of rpe_fetch_structure set.
 *    RPE_TRACK_EDGES_RANSAC: ransac_mask[i] of rpe_fetch_structure set.  That mask is findEssentialMat's inlier set of
 *     the one essential matrix of a pair whose status is RPE_PAIR_OK and zero for every other status:
 *     RPE_PAIR_NO_DESCRIPTORS and RPE_PAIR_INSUFFICIENT_MATCHES run no RANSAC, RPE_PAIR_NO_ESSENTIAL has no model and
 *     RPE_PAIR_AMBIGUOUS_ESSENTIAL (exactly five matches, several models) has no single one.  So RPE_PAIR_OK is the only
 *     status that leaves it valid.  The rule for rotation-only pairs, which are RPE_PAIR_OK and whose cheirality mask keeps
 *     next to nothing.
 *    RPE_TRACK_EDGES_ALL: every match i < n_matches[p], whatever the pair's status.
 *   The edge joins node (frame of image 1, qidx[i]) and node (frame of image 2, tidx[i]); its id is p * mm + i.
 *  Component: a connected component of the nodes that have at least one edge (a self pair (a, a) with qidx == tidx gives a
 *   component of one node).  It conflicts when it holds two nodes of one frame: a wrong match anywhere on a cycle, two
 *   matches of a RPE_MATCH_RATIO pair that name one train keypoint, a self pair with qidx != tidx.  A conflicting
 *   component is dropped and counted, whatever its length.  A conflict-free component with fewer than min_len nodes
 *   (min_len >= 2) is dropped and counted as short.  Every other component is a track.
 *  Order: tracks by ascending smallest node id; a track's observations by ascending node id (frame first, then keypoint).
 *  Outputs (host, any may be NULL; the caller sizes them by the bound track_start[P*mm + 1], obs_*[2*P*mm],
 *   match_track[P*mm]; only the used prefix of track_start and obs_* is written, match_track is written whole):
 *   counts[6] = {n_tracks, n_obs, n_edges, dropped_conflict, dropped_short, frames with at least one observation};
 *   track_start[n_tracks + 1]: CSR offsets into the observation arrays;  obs_frame[n_obs], obs_kp[n_obs]: frame and
 *   keypoint index of each observation;  obs_xy[2 * n_obs]: the keypoint's f32 pixel coordinates, the bits
 *   rpe_fetch_matched_points returns for the edge with the lowest id among those that name the node (image 1's point when
 *   that edge names the node on both sides);  match_track[P*mm]: the track index of the edge's component, -1 for a
 *   non-edge, an edge of a dropped component and past n_matches -- it ties a track to rpe_fetch_structure's points and masks.
 * The run's own results are untouched: every fetch of the run, rpe_refine_poses, rpe_scale_links, rpe_link_poses,
 * rpe_link_bundles, rpe_pair_homographies and rpe_guided_matches(_l2) return the same bits afterwards.  Bit-deterministic:
 * integer atomics only (min, add, compare-and-swap towards the smaller id), and no result depends on their order.
 * rpe_build_tracks: over all pairs of the last stream / pair list (use_pair[P] switches pairs off); P is
 * rpe_last_run_pairs(h), the count every output bound above is taken from.  Validity rules of
 * rpe_scale_links (refused after a chunked host batch, a stage call, a put, once the store was resized under a pair list,
 * and after a batch of two or more pairs); the structure kernels are launched when edge_rule reads masks that are not current.
 * RPE_ERR_INVALID as well: edge_rule outside 0 .. 2, min_len < 2.
 * rpe_tracks_from_matches: the stage form over the caller's own matches: P pairs (0 .. max_batch; RPE_ERR_CAPACITY above),
 * pair p joins frames frame1[p] and frame2[p] of n_frames and has m[p] matches; qidx / tidx / edge at p * mm (edge == NULL:
 * every match is an edge), pts1 / pts2 at (p * mm) * 2 (both NULL: obs_xy is zero).  It uses buffers of its own, created on
 * first use: the last run stays fetchable.  RPE_ERR_INVALID: n_frames < 1 or n_frames * KC >= 2^31, a frame index outside
 * 0 .. n_frames - 1, m[p] outside 0 .. mm, an index outside 0 .. KC - 1 among the first m[p], exactly one of pts1 / pts2
 * NULL, min_len < 2.  P == 0 returns all-zero counts.
 * All checks are host-side; nothing is launched and the handle stays usable after a refusal. */
enum { RPE_TRACK_EDGES_USABLE = 0, RPE_TRACK_EDGES_RANSAC = 1, RPE_TRACK_EDGES_ALL = 2 };
/* pairs of the last batch / stream / pair list of the handle (a chunked host batch: of the whole batch); 0 before any run,
 * after rpe_frames_put* and for h == NULL.  What rpe_build_tracks sizes its outputs by. */
int rpe_last_run_pairs(const rpe_handle *h);
int rpe_build_tracks(rpe_handle *h, const uint8_t *use_pair, int edge_rule, int min_len,
                     int32_t *counts, int32_t *track_start, int32_t *obs_frame, int32_t *obs_kp, float *obs_xy,
                     int32_t *match_track);
int rpe_tracks_from_matches(rpe_handle *h, int P, int n_frames, const int32_t *frame1, const int32_t *frame2, const int32_t *m,
                            const int32_t *qidx, const int32_t *tidx, const uint8_t *edge, const float *pts1, const float *pts2,
                            int min_len, int32_t *counts, int32_t *track_start, int32_t *obs_frame, int32_t *obs_kp,
                            float *obs_xy, int32_t *match_track);

/* ----------------------------------------------------------- track points */
/* The sparse map of a run (NOT in the reference): one scene point per track, triangulated from ALL the views of the track
 * under absolute poses, with a verdict on every observation.  A stage-form call over the caller's arrays: the tracks as
 * rpe_build_tracks writes them (track_start[n_tracks + 1], obs_frame[n_obs], obs_xy[2 * n_obs] f32 pixels, n_obs =
 * track_start[n_tracks]); world-to-camera poses x = R X + T per frame, R_abs[9 * n_frames] row-major, T_abs[3 * n_frames];
 * frame_group[n_frames]: frames with the same value >= 0 share one scale (one segment of a chained trajectory), a negative
 * value is a frame without a pose, NULL puts every frame in group 0; and exactly one of K[9] (one camera for all frames)
 * and cams[n_frames] (one per frame, normalised and undistorted as in "camera models"; K is the camera {K[0], K[4], K[2],
 * K[5], no lens}, so K and cams filled with that pinhole give the same bits).
 * The rule, for one track with observations o = s .. e-1 (s = track_start[k], e = track_start[k + 1]).  All arithmetic
 * f64, + - * / sqrt only, no contraction; a comparison with a NaN is false; every sum over observations starts from 0 and
 * adds the observations in ascending o, left to right; a 3-vector dot product is (a0*b0 + a1*b1) + a2*b2.
 *  Per observation, with (R, T) and the camera of its frame: (x, y) = the normalised, undistorted point; v = R'(x, y, 1):
 *   v_k = (R[0][k]*x + R[1][k]*y) + R[2][k];  bearing d = v / sqrt(v.v);  centre c_k = -((R[0][k]*T0 + R[1][k]*T1) +
 *   R[2][k]*T2);  f = (fx + fy) / 2.
 *  1 Group and used set.  G = the group of the first observation whose frame has a group >= 0; U = the observations whose
 *   frame has group G.  No such observation, or |U| < min_views: RPE_TRACKPT_TOO_FEW.
 *  2 Midpoint start over a selection S (first S = U): M = I - d d', m_ij = (i == j ? 1 : 0) - d_i*d_j;  A = sum M (upper
 *   triangle), b_i = sum ((m_i0*c0 + m_i1*c1) + m_i2*c2);  A X = b by the Cholesky of rpe_refine_poses at lambda = 0
 *   (pivot s of column j: L_jj minus the squares of the row so far; s > 0 and finite, else not positive definite).  Not
 *   positive definite: RPE_TRACKPT_DEGENERATE.  Depth of X in a view: z = y2, y = R X + T, each row ((r0*X0 + r1*X1) +
 *   r2*X2) + t.  A view of S without z > 0: RPE_TRACKPT_BEHIND.
 *  3 Levenberg-Marquardt on X over S.  Residual of a view, in pixels: u = y0/y2, w = y1/y2, e0 = f*(u - x), e1 = f*(w - y);
 *   cost = sum (e0*e0 + e1*e1).  With q = f/y2, a = q*u, b = q*w the two Jacobian rows are J0_k = q*R[0][k] - a*R[2][k],
 *   J1_k = q*R[1][k] - b*R[2][k];  H_ij = sum (J0_i*J0_j + J1_i*J1_j) (upper triangle), g_i = sum (J0_i*e0 + J1_i*e1).
 *   The loop is rpe_refine_poses': lambda0 = 1e-3; at most max_iters iterations, each solving (H + lambda diag H) step = -g
 *   (not positive definite: lambda * 10, next iteration) and trying X + step; a trial with a view of S without z > 0 has
 *   infinite cost; a trial whose cost is finite and strictly lower is accepted (lambda / 10) and ends the loop when it
 *   lowered the cost by no more than 1e-6 of it or sqrt((s0*s0 + s1*s1) + s2*s2) <= 1e-9; any other trial: lambda * 10.
 *   max_iters = 0 leaves the midpoint.
 *  4 Classify, over all of U at X: a view with z > 0 has err = sqrt(e0*e0 + e1*e1) and is an inlier when err <=
 *   threshold_px; a view without z > 0 is an outlier with err = -1.  All of U inliers: step 5.  Else, after the first pass
 *   and with at least min_views inliers: steps 2 and 3 once more with S = the inliers, then U is classified again at the
 *   new X; there is exactly one such reselection.  Fewer than min_views inliers at the end: RPE_TRACKPT_OUTLIERS.
 *  5 Parallax.  r = c - X per inlier view; min_cos = the smallest of 1 and, for every inlier view but the first,
 *   (r1 . r) / (sqrt(r1 . r1) * sqrt(r . r)) with r1 that of the first inlier view.  min_cos > max_cos:
 *   RPE_TRACKPT_LOW_PARALLAX (max_cos = 1 switches the gate off), else RPE_TRACKPT_OK.
 *  Outputs (host, any may be NULL): points[3 * n_tracks], in the frame of the poses; info[4 * n_tracks] = {RPE_TRACKPT_*
 *   code, |U|, inliers, LM iterations begun over both rounds}; rms[n_tracks] = sqrt((sum over the inliers of (e0*e0 +
 *   e1*e1)) / inliers), pixels; min_cos[n_tracks]; obs_flag[n_obs]: 0 not used, 1 inlier, 2 outlier; obs_err[n_obs]: err,
 *   0 where not used.  By code: OK and LOW_PARALLAX return everything.  OUTLIERS returns the last X, the flags, err and rms
 *   (0 without an inlier) and min_cos = 0.  BEHIND (either round) returns the midpoint it was found at, flags 2 for all of
 *   U, and zero err, rms, min_cos and inlier count.  TOO_FEW and DEGENERATE (either round) return zeros: point, flags,
 *   err, rms, min_cos, inlier count.
 * Bit-deterministic: one thread walks a track's observations in order, so there is no reduction tree and no atomic.  The
 * call uses device buffers of its own, created on the first call and grown to the largest call; neither the workspace nor
 * the record of the last run is touched: every fetch of the run and every call behind it returns the same bits afterwards.
 * RPE_ERR_INVALID: n_tracks < 0; a NULL input that is read (n_tracks > 0: track_start, R_abs, T_abs; n_obs > 0: obs_frame,
 * obs_xy); track_start[0] != 0 or track_start decreasing; n_frames < 1; a frame index outside 0 .. n_frames - 1; both or
 * neither of K / cams; a camera with a non-finite field, fx <= 0 or fy <= 0; threshold_px not finite or <= 0; min_views < 2;
 * max_cos outside (-1, 1]; max_iters outside 0 .. 100; a non-finite pose entry of a frame whose group is >= 0.  All checks
 * are host-side; nothing is launched and the handle stays usable after a refusal.  n_tracks == 0 passes the scalar checks,
 * succeeds and writes nothing. */
enum { RPE_TRACKPT_OK = 0, RPE_TRACKPT_TOO_FEW = 1, RPE_TRACKPT_DEGENERATE = 2, RPE_TRACKPT_BEHIND = 3, RPE_TRACKPT_OUTLIERS = 4,
       RPE_TRACKPT_LOW_PARALLAX = 5 };
int rpe_triangulate_tracks(rpe_handle *h, int n_tracks, const int32_t *track_start, const int32_t *obs_frame, const float *obs_xy,
                           int n_frames, const double *R_abs, const double *T_abs, const int32_t *frame_group, const double *K,
                           const rpe_camera *cams, double threshold_px, int min_views, double max_cos, int max_iters,
                           double *points, int32_t *info, double *rms, double *min_cos, uint8_t *obs_flag, double *obs_err);

/* --------------------------------------------------------- window bundles */
/* Bundle adjustment of windows of 2 .. RPE_WINDOW_MAX_VIEWS frames (NOT in the reference): the poses of a window's frames
 * and the points of the tracks they see are refined together on one reprojection cost.  A stage-form call over the caller's
 * arrays: tracks, poses and one K or cams exactly as rpe_triangulate_tracks takes them; points0[3 * n_tracks]: a start point
 * per track in the frame of the poses (what rpe_triangulate_tracks returns); point_use[n_tracks] (NULL: every track; a
 * track is used when its byte is not 0); obs_use[n_obs] (NULL: every observation; an observation is selected when its
 * byte is exactly 1, so rpe_triangulate_tracks' obs_flag can be passed as it is); windows in CSR form: window w is the
 * frames win_frame[win_start[w] .. win_start[w + 1]), W of them, distinct, in any order; windows may overlap, each is
 * solved on its own from the caller's poses and points.
 * The rule, for one window with frames F_0 .. F_(W-1) ("position" p = 0 .. W-1).  All arithmetic f64, + - * / sqrt only
 * (sin for a rotation increment, as rpe_refine_poses), no contraction; a comparison with a NaN is false; finite(v) =
 * fabs(v) <= DBL_MAX; a 3-vector dot product is (a0*b0 + a1*b1) + a2*b2.
 *  Per observation: (x, y) = the normalised, undistorted point and f = (fx + fy) / 2 of its frame's camera, as in "track
 *   points".
 *  Points: track k's observation at position p is the lowest o in its segment with obs_frame[o] == F_p that is selected.
 *   A used track with observations at two or more positions is a candidate.  Candidates are numbered j = 0, 1, .. in
 *   ascending track order; the first max_points are the window's points, the rest are dropped and counted.  The sets
 *   are fixed for the whole optimisation; there is no robust kernel.
 *  Gauge: with (R_p, T_p) the caller's pose of F_p, the pose of position p relative to position 0 is
 *   Q_p[r][c] = (R_p[r][0]*R_0[c][0] + R_p[r][1]*R_0[c][1]) + R_p[r][2]*R_0[c][2],
 *   s_p[r] = T_p[r] - ((Q_p[r][0]*T_0[0] + Q_p[r][1]*T_0[1]) + Q_p[r][2]*T_0[2]);  n_p = s_p . s_p is the squared distance
 *   of the two centres.  The anchor A is the position >= 1 with the largest n_p (a later position wins only when strictly
 *   larger); l = sqrt(n_A) is the unit of scale.  The problem is solved in position 0's coordinates scaled by 1 / l:
 *   t_p[r] = s_p[r] / l and, per point, X[r] = (((R_0[r][0]*P0 + R_0[r][1]*P1) + R_0[r][2]*P2) + T_0[r]) / l with P the start
 *   point.  Position 0 is the identity and never moves; t_A moves on the unit sphere only.
 *  Codes, tested in this order: l not > 0 or not finite: RPE_WINDOW_NO_BASELINE.  A position p >= 1 with fewer than
 *   max(min_obs, 6) observations of points: RPE_WINDOW_TOO_FEW.  After the loop RPE_WINDOW_REJECTED or RPE_WINDOW_OK (Result).
 *  Parameters: position p >= 1 has the block (w[3], d[3]), the anchor (w[3], a[2]); the blocks follow each other in
 *   ascending position: 6 W - 7 camera parameters.  Q_p <- exp([w]x) Q_p; t_p <- t_p + d; t_A <- normalise((t_A + a0*b1) +
 *   a1*b2) with (b1, b2) the tangent basis of rpe_refine_poses at t_A;  X_j <- X_j + dp_j, three parameters per point.
 *  Rows of a view, in pixels: at position 0, y = X; else a = Q_p X (each row (q0*X0 + q1*X1) + q2*X2), y = a + t_p.
 *   u = y0/y2, v = y1/y2, e0 = f*(u - x), e1 = f*(v - y), s = f/y2.  Derivatives as in "link bundles": by w as in "link
 *   poses" polish; Jt = (s, 0, -s*u) / (0, s, -s*v) by t; (Jt . b1, Jt . b2) by the tangent step; by X: Jt Q_p (column k:
 *   (Jt0*Q[0][k] + Jt1*Q[1][k]) + Jt2*Q[2][k]), at position 0 Jt itself.  A point's cost is the sum over its views in
 *   ascending position, from 0, of (e0*e0 + e1*e1); cost = the sum over the points.
 *  The step at damping lambda solves (J'J + lambda diag J'J) step = -J'r exactly by eliminating the points.  Per point,
 *   over its views in ascending position, x row before y row: V = Jp'Jp (upper triangle), g_p = Jp'e; V_ii <- V_ii +
 *   lambda*V_ii; its inverse by the adjugate divided by det = (v00*c00 + v01*c01) + v02*c02 as in "link bundles"; det > 0
 *   and finite, else the step is rejected.  Per view at p >= 1: W_p[k][i] = Jc0[k]*Jx0[i] + Jc1[k]*Jx1[i] (k: the
 *   block's parameters, Jc the two rows by them, Jx by the point), Y_p[k][i] = (Vi[i][0]*W_p[k][0] + Vi[i][1]*W_p[k][1]) +
 *   Vi[i][2]*W_p[k][2].  Over the points: U_p[k][m] = sum (Jc0[k]*Jc0[m] + Jc1[k]*Jc1[m]), g_c,p[k] = sum (Jc0[k]*e0 +
 *   Jc1[k]*e1), v_p[k] = sum Y_p[k] . g_p over the points position p sees; S_pq[k][m] = sum Y_p[k] . W_q[m] over the
 *   points positions p <= q both see.  H = (U + lambda diag U) - S with U block diagonal (0 - S elsewhere), g = g_c - v;
 *   H step_c = -g by the Cholesky of rpe_refine_poses at lambda = 0 (not positive definite: rejected);
 *   dp = -Vi (g_p + W' step_c): u_i = g_p[i], then u_i <- u_i + W_p[k][i]*step_c[block p, k] over the point's views in
 *   ascending position and k ascending; dp_i = -((Vi[i][0]*u0 + Vi[i][1]*u1) + Vi[i][2]*u2).
 *  Sums over points: U, g_c, v, S of one pair of positions: lane l of 64 adds its points j = l, l + 64, .. in ascending
 *   order, then the butterfly (partner lane ^ 32, 16, .. 1).  The cost: lane l of 256 likewise, the butterfly, then the
 *   four wave totals ((w0 + w1) + w2) + w3.  No atomics decide a value: bit-deterministic run to run.
 *  LM: the conventions of rpe_refine_poses: lambda0 = 1e-3; at most max_iters iterations, each building the step at the
 *   current state; a rejected step or a trial whose cost is not finite or not strictly lower: lambda * 10; an accepted
 *   one: lambda / 10, and the loop ends when it lowered the cost by no more than 1e-6 of it or the length of step_c (its
 *   squares added in ascending order) is <= 1e-9.  A start cost that is not finite runs no iteration.
 *  Result: the bundled state is returned (RPE_WINDOW_OK) only if a step was accepted, every pose entry and point
 *   coordinate is finite and every point has y2 > 0 in every view that observes it; otherwise RPE_WINDOW_REJECTED.  Back to
 *   the caller's frame: R_out[r][c] = (Q_p[r][0]*R_0[0][c] + Q_p[r][1]*R_0[1][c]) + Q_p[r][2]*R_0[2][c], T_out[r] =
 *   l*t_p[r] + ((Q_p[r][0]*T_0[0] + Q_p[r][1]*T_0[1]) + Q_p[r][2]*T_0[2]); point: m_r = l*X[r] - T_0[r], P_out[c] =
 *   (R_0[0][c]*m0 + R_0[1][c]*m1) + R_0[2][c]*m2.  Position 0 returns its input bits.  For every code but OK all poses and
 *   points are the input bits.
 *  Outputs (host, any may be NULL): R_out[9 * n], T_out[3 * n] with n = win_start[n_win], laid out like win_frame;
 *   points[n_win * max_points * 3] (zeros past the count); point_track[n_win * max_points]: the track of point j, -1 past
 *   the count; counts[n_win * 4] = {W, points, observations of points, candidates dropped by max_points};
 *   info[n_win * 4] = {RPE_WINDOW_* code, iterations begun, steps accepted, anchor position}; rms[n_win * 2] = sqrt(cost /
 *   observations) of the input state and of the returned state (both 0 for NO_BASELINE and TOO_FEW).
 * The call uses device buffers of its own, created on the first call and grown to the largest call; neither the workspace
 * nor the record of the last run is touched: every fetch of the run and every call behind it returns the same bits.
 * RPE_ERR_INVALID: the refusals of rpe_triangulate_tracks on the shared arguments (n_tracks, track_start, obs_frame, obs_xy,
 * n_frames, R_abs, T_abs, K / cams); n_win < 0; a NULL win_start or win_frame with n_win > 0; win_start[0] != 0 or
 * decreasing; a window of fewer than 2 or more than RPE_WINDOW_MAX_VIEWS frames; a frame index outside 0 .. n_frames - 1 or
 * repeated inside a window; a non-finite pose of a frame some window names; points0 NULL with n_tracks > 0, or a non-finite
 * start point of a used track; max_points < 1; min_obs < 0; max_iters outside 1 .. 100.  RPE_ERR_CAPACITY: max_points >
 * RPE_WINDOW_MAX_POINTS.  All checks are host-side; nothing is launched and the handle stays usable after a refusal.
 * n_win == 0 passes the scalar checks, succeeds and writes nothing. */
#define RPE_WINDOW_MAX_VIEWS 8
#define RPE_WINDOW_MAX_POINTS 16384
enum { RPE_WINDOW_OK = 0, RPE_WINDOW_NO_BASELINE = 1, RPE_WINDOW_TOO_FEW = 2, RPE_WINDOW_REJECTED = 3 };
int rpe_bundle_windows(rpe_handle *h, int n_tracks, const int32_t *track_start, const int32_t *obs_frame, const float *obs_xy,
                       const double *points0, const uint8_t *point_use, const uint8_t *obs_use,
                       int n_frames, const double *R_abs, const double *T_abs, const double *K, const rpe_camera *cams,
                       int n_win, const int32_t *win_start, const int32_t *win_frame, int max_points, int min_obs, int max_iters,
                       double *R_out, double *T_out, double *points, int32_t *point_track, int32_t *counts, int32_t *info,
                       double *rms);

/* ------------------------------------------------------------ pose graphs */
/* Pose-graph optimisation (NOT in the reference): the poses of a chain are moved onto relative-pose measurements between
 * its frames, so that a revisit (a loop edge) takes out the drift the chain has integrated.  A stage-form call over the
 * caller's arrays: n_frames poses R_abs[9 * n_frames], T_abs[3 * n_frames] in the convention of the chain, X_f = R_f X +
 * T_f; graphs in CSR form: graph g is the frames graph_frame[graph_start[g] .. graph_start[g + 1]), F of them, distinct;
 * graphs may share frames, each is solved on its own from the caller's poses; fixed[graph_start[n_graphs]] bytes laid out
 * like graph_frame (NULL: none; not 0: the frame does not move; position 0 of every graph is fixed whatever its byte);
 * edges in CSR form: graph g owns the edges edge_start[g] .. edge_start[g + 1); edge e joins the frames edge_i[e] and
 * edge_j[e] (frame indices; both frames of its graph, different) with the measurement X_j = M X_i + m, M = edge_R[9 e ..],
 * m = edge_t[3 e ..], the weights (w_rot, w_trans) = edge_w[2 e ..] and edge_kind[e]: RPE_EDGE_METRIC (m on the graph's
 * scale) or RPE_EDGE_DIRECTION (only the direction of m is measured).
 * The rule, for one graph.  All arithmetic f64, + - * / sqrt only -- no sin or cos anywhere: the rotation update is the
 * Cayley map -- no contraction; a comparison with a NaN is false; finite(v) = fabs(v) <= DBL_MAX; a 3-vector dot product is
 * (a0*b0 + a1*b1) + a2*b2; EVERY other sum starts at +0.0 and adds its terms in ascending order ("sum").  The GPU result
 * equals a scalar evaluation of this rule bit for bit on every output.
 *  Active set (host): a frame is fixed at position 0 or where its byte is set.  A frame is active when a path of the graph's
 *   edges joins it to a fixed frame (a fixed frame is active); it is free when it is active and not fixed.  An edge is used
 *   when both ends are active and at least one is free.  Free frames are numbered k = 0, 1, .. in ascending graph position,
 *   used edges u = 0, 1, .. in ascending position in the graph's edge list.  A frame that is not free returns its input bits.
 *  Codes, tested in this order: no used edge: RPE_GRAPH_NO_EDGES.  A free frame none of whose used edges has w_trans > 0:
 *   RPE_GRAPH_UNDERDETERMINED.  After the loop RPE_GRAPH_REJECTED or RPE_GRAPH_OK (Result).
 *  Rows of an edge (12) at the state (R, T): Q[r][c] = R_j[r] . R_i[c] (rows), q[r] = Q[r] . T_i, p[r] = T_j[r] - q[r],
 *   D[r][c] = Q[r] . M[c] (rows: D = Q M'), a = w_rot / sqrt(2).  Rotation rows 3 k + r = a * (D[r][k] - (r == k ? 1 : 0)),
 *   k = 0 .. 2: the columns of D - I, the chordal distance, monotone up to 180 degrees.  Translation rows 9 + r, metric:
 *   w_trans * (p[r] - m[r]); direction: n = sqrt(p . p); where n is not > 0 the three rows and their derivatives are +0;
 *   else u = p / n, w_trans * (u[r] - m[r] / sqrt(m . m)).
 *  Parameters of a free frame: (w[3], d[3]): R <- C(w) R, T <- T + d, with the Cayley map C(w): a = w / 2 (each
 *   component), n2 = a . a, f = 2 / (1 + n2), C[r][r] = 1 + f*(a_r*a_r - n2), C[0][1] = f*(a0*a1 - a2), C[0][2] = f*(a0*a2 +
 *   a1), C[1][0] = f*(a1*a0 + a2), C[1][2] = f*(a1*a2 - a0), C[2][0] = f*(a2*a0 - a1), C[2][1] = f*(a2*a1 + a0); (C R)[r][c]
 *   = (C[r][0]*R[0][c] + C[r][1]*R[1][c]) + C[r][2]*R[2][c].  C is a rotation for every w and agrees with exp to second order.
 *  Derivatives.  Rotation rows by d: structurally zero, not part of any sum.  Rotation row 3 k + r by w_j: with v = a *
 *   (column k of D): (0, v2, -v1), (-v2, 0, v0), (v1, -v0, 0) for r = 0, 1, 2; by w_i, column c: a * (D[r][k2]*M[k1][c] -
 *   D[r][k1]*M[k2][c]) with k1 = (k + 1) % 3, k2 = (k + 2) % 3 (that is a D [e_k]x M).  p by w_j: Pj = [q]x = (0, -q2, q1),
 *   (q2, 0, -q0), (-q1, q0, 0); by w_i: Pi[r] = (Q[r][2]*Ti1 - Q[r][1]*Ti2, Q[r][0]*Ti2 - Q[r][2]*Ti0, Q[r][1]*Ti0 -
 *   Q[r][0]*Ti1) (that is -Q [T_i]x); by d_j: I; by d_i: -Q.  Metric rows: w_trans * Pj[r][c], w_trans * Pi[r][c], by d_j
 *   (r == c ? w_trans : 0), by d_i -(w_trans * Q[r][c]).  Direction rows: N[r][c] = ((r == c ? 1 : 0) - u[r]*u[c]) / n;
 *   w_trans * (N[r] . column c of Pj), w_trans * (N[r] . column c of Pi), by d_j w_trans * N[r][c], by d_i
 *   -(w_trans * (N[r] . column c of Q)).
 *  Huber: s2 = sum of the 12 squared rows, s = sqrt(s2).  huber == 0 or s <= huber: weight h = 1, cost term s2; else
 *   h = huber / s, cost term (2*huber)*s - huber*huber.  Weights are recomputed at every linearisation; the trial cost uses
 *   the same terms.  cost = the reduction (below) of the used edges' terms.
 *  Normal equations, formed explicitly.  Per used edge, with J = (the three w columns | the three d columns): entry [a][b]
 *   of h Ji'Ji, h Jj'Jj, h Ji'Jj = h * sum over the rows of Ja[row]*Jb[row] -- all 12 rows when a and b are both w
 *   columns, rows 9 .. 11 otherwise -- and entry a of h Ji'r, h Jj'r = h * sum of J[row][a]*r[row] likewise.  Per free
 *   frame: its 6 x 6 block H_kk and gradient g_k = the sums over its used edges in ascending used-edge number of the
 *   edge's block and gradient of the frame's side (a gather per frame: no atomics decide a value).  Damping: H_kk[a][a] <-
 *   H_kk[a][a] + lambda*H_kk[a][a].
 *  Preconditioner: the Cholesky factor of each damped H_kk by columns, L[c][c] = sqrt(H[c][c] - L[c][0]^2 - .. ), L[r][c]
 *   = (H[r][c] - L[r][0]*L[c][0] - ..) / L[c][c], every product subtracted serially in ascending k; a pivot that is not
 *   > 0 or not finite rejects the step.  z = M^-1 r: y_i = (r_i - L[i][0]*y_0 - ..) / L[i][i] ascending, then z_i = (y_i -
 *   L[i+1][i]*z_(i+1) - ..) / L[i][i] descending, the products of a row subtracted in ascending k.
 *  Step: preconditioned conjugate gradients on H x = -g.  x = 0, r_k = -g_k, z = M^-1 r, p = z, rz = rz0 = r.z.  At most
 *   cg_iters times: (H p)_k[a] = sum_b H_kk[a][b]*p_k[b]; then over the frame's used edges in ascending number whose other
 *   end o is free, (H p)_k[a] <- (H p)_k[a] + sum_b A[a][b]*p_o[b] where the frame is the edge's i, + sum_b A[b][a]*p_o[b]
 *   where it is its j, A = h Ji'Jj.  pHp = p.Hp; not > 0: stop (before the first update: the step is rejected).  alpha = rz
 *   / pHp; x <- x + alpha*p; r <- r - alpha*Hp; z = M^-1 r; rzn = r.z: one PCG iteration is counted; rzn <= (cg_tol*cg_tol)
 *   * rz0: stop; beta = rzn / rz; p <- z + beta*p; rz = rzn.  A dot product of two 6-vectors is the sum of the six products.
 *  Reductions: p.Hp, r.z, the squared step length x.x (items: the free frames, each item the dot product of its 6-vectors)
 *   and the cost (items: the used edges): lane l of 256 adds its items l, l + 256, .. in ascending order, then the
 *   butterfly (partner lane ^ 32, 16, .. 1 inside each wave of 64), then the four wave totals ((w0 + w1) + w2) + w3.
 *  Trial: every free frame R <- C(x[0..2]) R, T <- T + x[3..5]; its cost as above.
 *  LM: the conventions of rpe_refine_poses: lambda0 = 1e-3; at most max_iters iterations, each building the step at the
 *   current state; a rejected step or a trial whose cost is not finite or not strictly lower: lambda * 10; an accepted one:
 *   lambda / 10, and the loop ends when it lowered the cost by no more than 1e-6 of it or the step length sqrt(x.x) is <=
 *   1e-9.  A start cost that is not finite runs no iteration.
 *  Result: the optimised state is returned (RPE_GRAPH_OK) only if a step was accepted and every entry of every free frame's
 *   pose is finite; otherwise RPE_GRAPH_REJECTED.  For every code but OK all poses are the input bits.
 *  Outputs (host, any may be NULL): R_out[9 * n], T_out[3 * n] with n = graph_start[n_graphs], laid out like graph_frame;
 *   counts[n_graphs * 4] = {frames, free frames, used edges, unused edges}; info[n_graphs * 4] = {RPE_GRAPH_* code,
 *   iterations begun, steps accepted, PCG iterations in total}; cost[n_graphs * 2]: of the input state and of the returned
 *   state; edge_chi[2 * n_edges]: the length s of each used edge's rows at the input state and at the returned state, 0 for
 *   an unused edge -- how a caller finds the loop edge to drop; edge_used[n_edges] bytes.
 * The call uses device buffers of its own, created on the first call and grown to the largest call; neither the workspace
 * nor the record of the last run is touched: every fetch of the run and every call behind it returns the same bits.
 * RPE_ERR_INVALID: a NULL handle; n_frames < 1; n_graphs < 0; huber negative or not finite; max_iters outside 1 .. 100;
 * cg_iters outside 1 .. 1000; cg_tol outside [0, 1); with n_graphs > 0: a NULL R_abs, T_abs, graph_start, graph_frame or
 * edge_start, or a NULL edge array with edges; a CSR array not starting at 0 or decreasing; a graph of fewer than 2 frames;
 * a frame index outside 0 .. n_frames - 1 or repeated inside a graph; an edge end that is no frame of its graph; i == j; a
 * non-finite pose of a frame some graph names; a non-finite measurement or weight; w_rot not > 0 or w_trans < 0; an edge_R
 * whose M M' differs from I by more than 1e-6 in an entry; an unknown kind; a direction edge with m = 0.  RPE_ERR_CAPACITY:
 * a graph of more than RPE_GRAPH_MAX_FRAMES frames or RPE_GRAPH_MAX_EDGES edges.  All checks are host-side; nothing is
 * launched and the handle stays usable after a refusal.  n_graphs == 0 passes the scalar checks, succeeds and writes nothing. */
#define RPE_GRAPH_MAX_FRAMES 4096
#define RPE_GRAPH_MAX_EDGES 65536
enum { RPE_EDGE_METRIC = 0, RPE_EDGE_DIRECTION = 1 };
enum { RPE_GRAPH_OK = 0, RPE_GRAPH_NO_EDGES = 1, RPE_GRAPH_UNDERDETERMINED = 2, RPE_GRAPH_REJECTED = 3 };
int rpe_optimise_graphs(rpe_handle *h, int n_frames, const double *R_abs, const double *T_abs,
                        int n_graphs, const int32_t *graph_start, const int32_t *graph_frame, const uint8_t *fixed,
                        const int32_t *edge_start, const int32_t *edge_i, const int32_t *edge_j, const double *edge_R,
                        const double *edge_t, const double *edge_w, const int32_t *edge_kind,
                        double huber, int max_iters, int cg_iters, double cg_tol,
                        double *R_out, double *T_out, int32_t *counts, int32_t *info, double *cost, double *edge_chi,
                        uint8_t *edge_used);

/* --------------------------------------------------------- pair proposals */
/* Which frames see the same place (NOT in the reference): an exact similarity score between stored frames and a top-k
 * candidate selection, both on the GPU, so that a pair list for rpe_enqueue_pairs (loop closures, windows of far-apart
 * frames) can come from the library itself.  Hamming handles only (ORB + RPE_NORM_HAMMING).
 *
 * The score.  The SAMPLE of a frame with n keypoints under a stride step >= 1 is its descriptors 0, step, 2 step, ...:
 * M = ceil(n / step) of them, sample index k being keypoint k * step.  score(a, b) is the number of mutual nearest
 * neighbours between the two samples whose Hamming distance is <= max_distance (0 .. 256); "mutual nearest" is cv2's
 * crossCheck rule, both argmins taking the lowest index among equal distances (the rule of rpe_match_hamming, without its
 * max_matches cut).  The mutual set of (a, b) is the transpose of that of (b, a), so the score is symmetric; an empty
 * sample gives 0; a self pair is computed like any other.  Exact integers: scores[r * nt + c] = score(frame of query
 * position r, frame of target position c).
 *
 * The candidates.  Column c is eligible for row r iff the two slots differ, |q_time[r] - t_time[c]| > exclude when
 * exclude >= 0, and the score is >= min_score.  A row's candidates are its eligible columns by score descending, then
 * column position ascending, the first k of them: cand[r * k + m] is a column POSITION (an index into t_slots), and
 * cand_score[r * k + m] its score; both are -1 for m >= n_cand[r], the row's count.  A NULL time array means
 * time = slot number (stage form: frame index), which suits callers that put frame f into slot f; callers with a ring
 * pass frame numbers.
 *
 * rpe_frames_similar: over the frame store.  q_slots[nq] / t_slots[nt] are host arrays of filled slots; repeats are
 * allowed within a list, the lists may be as long as the store and may be the same list (identical lists are computed
 * as one triangle and mirrored).  scores may be NULL, and so may cand / cand_score / n_cand (all three or none; k = 0
 * with the three NULL is allowed); at least one output must be asked for.  The call reads the store, writes buffers of
 * its own (created on first use, grown to the largest call) and synchronises the handle's stream; the last run and
 * everything fetched from it afterwards are untouched.
 * rpe_similarity_hamming: the stage form, on the caller's own descriptors h_desc [F][cap][32] (cap =
 * rpe_keypoint_capacity()) with counts n[F], F <= 2*max_batch; q_idx / t_idx index the frames 0 .. F-1 and take the
 * place of the slots.  Like every stage call it overwrites the extraction workspace: the calls behind the last run are
 * refused until the next batch, stream or pair list.
 * RPE_ERR_INVALID, with nothing launched and the handle still usable: a NULL handle or list; no store; a slot outside
 * the store or an empty slot (stage form: F < 1, a count outside 0 .. cap, an index outside 0 .. F-1); step < 1;
 * max_distance outside 0 .. 256; k outside 0 .. RPE_SIMILAR_MAX_K; nq < 1 or nt < 1; no output, or only part of the
 * candidate trio; an L2 or SIFT handle.  RPE_ERR_CAPACITY: nq * nt > 2^31 - 1, F > 2*max_batch.  RPE_ERR_HIP: the
 * device cannot hold the call's buffers (nq * nt scores and the tables); the buffer set is then empty and the next call
 * tries again. */
#define RPE_SIMILAR_MAX_K 32
int rpe_frames_similar(rpe_handle *h, int nq, const int32_t *q_slots, int nt, const int32_t *t_slots,
                       int step, int max_distance, const int32_t *q_time, const int32_t *t_time,
                       int exclude, int min_score, int k,
                       int32_t *scores, int32_t *cand, int32_t *cand_score, int32_t *n_cand);
int rpe_similarity_hamming(rpe_handle *h, const uint8_t *h_desc, const int32_t *n, int F,
                           int nq, const int32_t *q_idx, int nt, const int32_t *t_idx,
                           int step, int max_distance, const int32_t *q_time, const int32_t *t_time,
                           int exclude, int min_score, int k,
                           int32_t *scores, int32_t *cand, int32_t *cand_score, int32_t *n_cand);

/* ---------------------------------------------------------- stage entry */
/* replaces extractor.detectAndCompute(image, None) (pose_estimator.py:108)
 * for n_images images (n_images <= 2*max_batch).  kps[n_images*cap],
 * desc[n_images*cap*32], counts[n_images]; cap = rpe_keypoint_capacity(). */
int rpe_orb_detect_and_compute(rpe_handle *h, const uint8_t *h_imgs, int n_images,
                               rpe_keypoint *kps, uint8_t *desc, int32_t *counts);
/* intermediate images of image `index` of the last rpe_orb_detect_and_compute run, in the ORACLE's
 * packed pyramid layout (levels back to back, total = sum w_l*h_l):
 * which = 0 pyramid, 2 NMS map (FAST score where the pixel survived 3x3 NMS and the 31-px border
 * filter, else 0), 3 blurred pyramid.  (The FAST score map before NMS is never materialised by the
 * fused kernel; which = 1 is rejected.)  ORB handles only. */
int rpe_orb_debug_fetch(rpe_handle *h, int index, int which, uint8_t *h_out);
int64_t rpe_orb_pyramid_pixels(const rpe_handle *h);
/* The smallest number of images of one ORB extraction (2 B of a batch, the frames of a stream, n_images here) that runs
 * detection in level groups: FAST per group of pyramid levels, that of the first group on a second stream beside the
 * resize of the levels above it, the keypoint selection of a finished group on that stream beside FAST of the next.
 * Smaller extractions launch one kernel after the other.  Both schedules give the
 * same bits; only the count decides, and batches small enough to be replayed as a graph are always below it. */
int rpe_orb_group_min_images(void);
/* KeyPointsFilter::retainBest as retain_fast / retain_harris replay it, on n_lists caller-supplied lists in one launch
 * (one workgroup per list, the kernels' own device routine).  kind 0: u32 FAST entries, compared on bits 24..31 (the
 * score); kind 1: u64 Harris entries, compared on the f32 in bits 32..63.  elems[n_lists*cap]: list i at elems + i*cap
 * holds len[i] elements and is reordered in place exactly as retainBest(n_points[i]) of the stl_runtime (RPE_STL_*)
 * leaves it; out_len[i] receives its new size.  RPE_ERR_INVALID, nothing launched: a list longer than cap, cap beyond
 * 8192 elements or 64 KB of LDS (elements + 2 bytes each).  ORB handles only. */
int rpe_orb_debug_retain(rpe_handle *h, int kind, int stl_runtime, void *elems, const int32_t *len, const int32_t *n_points,
                         int n_lists, int cap, int32_t *out_len);

/* replaces matcher.match + sorted + truncate (pose_estimator.py:144-151) for B
 * descriptor-set pairs.  desc1/desc2: B*cap*32 bytes (cap = keypoint
 * capacity), n1/n2: B counts.  Outputs sized B*max_matches. */
int rpe_match_hamming(rpe_handle *h, const uint8_t *h_desc1, const int32_t *n1,
                      const uint8_t *h_desc2, const int32_t *n2, int B,
                      int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_matches);

/* stage form of rpe_guided_matches, the sibling of rpe_match_hamming: the caller's own features.  desc1 / desc2:
 * B*cap*32 bytes, pts1 / pts2: B*cap*2 f32 keypoint pixels, n1 / n2: B counts; one K; R[B*9], t[B*3] required.
 * Outputs sized B*max_matches, -1 past n_matches[p].  Goes through the workspace like every stage call (the last run's
 * per-match results end here).  Same argument checks as rpe_guided_matches. */
int rpe_match_hamming_guided(rpe_handle *h, const uint8_t *h_desc1, const float *h_pts1, const int32_t *n1,
                             const uint8_t *h_desc2, const float *h_pts2, const int32_t *n2, int B,
                             const double K[9], const double *R, const double *t, double gate_px, int max_distance,
                             int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_matches);

/* replaces cv2.SIFT_create().detectAndCompute(image, None) (pose_estimator.py:93-94, :108); the
 * handle must have been created with feature_method = RPE_FEATURE_SIFT, norm_type = RPE_NORM_L2.
 * cfg.nfeatures is the keypoint cap (SIFT_create(nfeatures); BASELINE config 3 uses 2048 -- the
 * reference itself passes no cap).  kps[n_images*cap], desc[n_images*cap*128] f32, counts[n_images]. */
int rpe_sift_detect_and_compute(rpe_handle *h, const uint8_t *h_imgs, int n_images,
                                rpe_sift_keypoint *kps, float *desc, int32_t *counts);
/* Gaussian pyramid of image `index` of the last SIFT run (octave-major, 6 levels per octave, tight
 * rows); returns the float count (out may be NULL to query it) */
int64_t rpe_sift_debug_gauss(rpe_handle *h, int index, float *out);

/* replaces BFMatcher(NORM_L2, crossCheck=True).match + sorted + truncate (pose_estimator.py:127-131,
 * :144-151) for byte-valued descriptors given as f32: SIFT handles B*cap*128 each (cv2 returns SIFT descriptors as
 * integer-valued f32), ORB handles created with NORM_L2 B*cap*32 each.  dist: f32 L2 distances. */
int rpe_match_l2(rpe_handle *h, const float *h_desc1, const int32_t *n1, const float *h_desc2,
                 const int32_t *n2, int B, int32_t *qidx, int32_t *tidx, float *dist, int32_t *n_matches);

/* stage form of rpe_guided_matches_l2, the sibling of rpe_match_l2: the caller's own features.  desc1 / desc2: byte-valued
 * f32 as in rpe_match_l2 (the same conversion and refusal), pts1 / pts2: B*cap*2 f32 keypoint pixels, n1 / n2: B counts;
 * one K; R[B*9], t[B*3] required.  Outputs sized B*max_matches; past n_matches[p] -1 (indices) and all-ones bits (dist).
 * Goes through the workspace like every stage call (the last run's per-match results end here).  Same argument checks
 * as rpe_guided_matches_l2. */
int rpe_match_l2_guided(rpe_handle *h, const float *h_desc1, const float *h_pts1, const int32_t *n1,
                        const float *h_desc2, const float *h_pts2, const int32_t *n2, int B,
                        const double K[9], const double *R, const double *t, double gate_px, double max_distance,
                        int32_t *qidx, int32_t *tidx, float *dist, int32_t *n_matches);

/* replaces cv2.findEssentialMat(pts1, pts2, K, RANSAC, prob, threshold)
 * (pose_estimator.py:522-527).  pts: B*max_matches*2 f32, m[B] counts.
 * Outputs: E[B*9], mask[B*max_matches], found[B], info[B*4] =
 * {best_count, best_iter, best_model, iters_run}. */
int rpe_find_essential(rpe_handle *h, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                       const double K[9], double *E, uint8_t *mask, int32_t *found, int32_t *info);

/* replaces cv2.recoverPose(E, pts1, pts2, K) (pose_estimator.py:533) */
int rpe_recover_pose(rpe_handle *h, const double *h_E, const float *h_pts1, const float *h_pts2,
                     const int32_t *m, int B, const double K[9],
                     double *R, double *t, int32_t *inliers);

/* stage form of rpe_refine_poses, for callers that hold their own matches: pts as in rpe_recover_pose,
 * mask[B*max_matches] (non-zero = use) selects the residuals, (R0[B*9], t0[B*3], |t0| = 1) is the start; inliers
 * counts the cheirality inliers of the returned pose over all m[p] matches.  Overwrites the per-match buffers like
 * every stage call (rpe_fetch_structure / rpe_refine_poses are refused afterwards). */
int rpe_refine_pose_points(rpe_handle *h, const double *h_R0, const double *h_t0, const float *h_pts1,
                           const float *h_pts2, const uint8_t *h_mask, const int32_t *m, int B, const double K[9],
                           int max_iters, double *R, double *t, int32_t *inliers, int32_t *info, double *rms);

/* ------------------------------------------------------------ profiling */
/* Per-stage device time of the last hot-path call, from hipEvents recorded
 * on the handle's stream around each kernel group.  The stages partition the call: their sum is the span from the first
 * event to the last.  An ORB extraction of rpe_orb_group_min_images() images or more also runs kernels on a second stream
 * beside those of the handle's stream, and a stage then covers what ran in its span on either: `pyramid` the resize
 * launches with FAST of the first level group beside the later ones, `fast` the other groups' FAST with the selection
 * of finished groups beside it, `select`, `harris` and `keypoints` the last group's selection, `keypoints` also the wait
 * for the second stream.  Such a stage time is a share of the step, not the cost of its kernels run alone. */
enum {
    RPE_STAGE_PYRAMID = 0, RPE_STAGE_FAST, RPE_STAGE_NMS, RPE_STAGE_SELECT, RPE_STAGE_HARRIS,
    RPE_STAGE_KEYPOINTS, RPE_STAGE_ANGLE, RPE_STAGE_BLUR, RPE_STAGE_DESCRIBE, RPE_STAGE_MATCH,
    RPE_STAGE_RANSAC, RPE_STAGE_POSE, RPE_STAGE_COUNT
};
int rpe_set_profiling(rpe_handle *h, int enable);
int rpe_get_stage_ms(rpe_handle *h, float *ms /* RPE_STAGE_COUNT */);
const char *rpe_stage_name(int stage);

/* ------------------------------------------------------------- multi-GPU */
/* The path shards by independent pairs (the reference never chains estimates, batch_processor.py:82-92): one process
 * and one handle per GPU, no data-path exchange.  The single collective is the final pose gather: every rank contributes
 * per_rank 128-byte records and receives all of them -- ncclAllGather over RCCL / xGMI on the handle's stream.  librccl is
 * loaded lazily by the first rpe_comm_* call.  Bootstrap: rank 0 calls rpe_comm_unique_id and hands the 128 bytes to the
 * other ranks by any means (sharding.py uses a file next to the launcher's MASTER_PORT); every rank then calls
 * rpe_comm_create.  Record layout (RPE_POSE_RECORD_BYTES = 128): double R[9]; double t[3]; int32 inliers, status,
 * n_matches, pair (global pair index, -1 for padding); 16 bytes reserved. */
#define RPE_COMM_ID_BYTES 128
#define RPE_POSE_RECORD_BYTES 128
typedef struct rpe_comm rpe_comm;
int rpe_comm_unique_id(uint8_t id[RPE_COMM_ID_BYTES]);
int rpe_comm_create(rpe_handle *h, int rank, int world, const uint8_t id[RPE_COMM_ID_BYTES], rpe_comm **out);
/* the same in two steps, for launchers that let the ranks agree in between (sharding.PoseComm): rpe_comm_prepare does
 * everything that can fail on one rank alone (dlopen of librccl, device buffers), rpe_comm_connect enters the collective
 * ncclCommInitRank -- a rank whose local step failed never leaves the others waiting inside it */
int rpe_comm_prepare(rpe_handle *h, int rank, int world, rpe_comm **out);
int rpe_comm_connect(rpe_comm *c, const uint8_t id[RPE_COMM_ID_BYTES]);
int rpe_comm_destroy(rpe_comm *c);
const char *rpe_comm_last_error(void);
/* packs the results of the handle's last batch (n_local pairs, global indices first_pair ..) into records on the
 * device, all-gathers per_rank records per rank (n_local <= per_rank <= max_batch; padded with pair = -1) and copies
 * the world * per_rank records to h_records (host, world * per_rank * 128 bytes), rank-major. */
int rpe_gather_poses(rpe_handle *h, rpe_comm *c, int n_local, int per_rank, int first_pair, void *h_records);
/* max over ranks of one host double (step timing); rpe_comm_barrier = the same exchange without a value */
int rpe_comm_allreduce_max(rpe_comm *c, double *value);
int rpe_comm_barrier(rpe_comm *c);

/* ---------------------------------------------------- roofline calibration */
/* Measured vector-instruction ISSUE rate of this device (wave-instructions per second, whole chip) for one
 * instruction kind at `waves_per_simd` (1..8) resident waves per SIMD: the roof bench.py prices the VALU-bound
 * kernels against.  kind: 0 v_xor+v_bcnt (Hamming), 1 v_pk_min/max_i16 (FAST pair test), 2 v_perm_b32,
 * 3 v_dot4_u32_u8, 4 v_min3/v_max3_i32 (FAST score), 5 v_mad_u32_u24, 6 v_mul_f64+v_add_f64 (RANSAC, pose),
 * 7 v_fma_f64, 8 v_fma_f32, 9 v_pk_fma_f32 (the last two only to place the integer / f64 cadence next to the f32 one),
 * 10 v_dot2_u32_u16, 11 v_alignbyte_b32, 12 v_mul_lo_u32, 13 v_mad_u64_u32, 14 v_mul_u32_u24_sdwa, 15 v_pk_mad_u16,
 * 16 v_lerp_u8 (FAST pair test, four byte compares), 17 v_bitop3_b32 (its pair logic)
 * (which instructions are full rate and which are not decides how the integer kernels are written).
 * rpe_calibrate_hbm: measured 16-B-per-lane streaming read rate (bytes/s). */
int rpe_calibrate_valu(rpe_handle *h, int kind, int waves_per_simd, double *wave_insts_per_s);
const char *rpe_calibrate_valu_name(int kind);
int rpe_calibrate_hbm(rpe_handle *h, double *bytes_per_s);

#ifdef __cplusplus
}
#endif
#endif /* RPE_AMD_H */
