// rpe_internal.h -- shared declarations of the MI355X (gfx950) relative-pose engine.
// Host handle, HBM workspace layout and kernel-launcher prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>
#include "../../include/rpe_amd.h"
#include "buf_layout.h"
#include "orb_groups.h"
#include "track_scene.h"

#define RPE_NLEVELS RPE_ORB_LEVELS
#define RPE_EDGE 31            // ORB edgeThreshold (cv2 default; pose_estimator.py:85-91 leaves it)
#define RPE_HALF_PATCH 15      // patchSize 31
#define RPE_RANSAC_CHUNK 64    // solver wave granularity: 64 RANSAC iterations per wave
#define RPE_RANSAC_MAXCHUNK 512 // largest number of iterations evaluated per launch group (8 waves per pair)
#define RPE_MAX_MODELS 10
#define RPE_GRAPH_MAX_PAIRS 16    // batches up to this many pairs are replayed as a captured hipGraph
// ORB detection over this many images and more runs in RPE_ORB_GROUPS level groups (orb_groups.h) on two streams: FAST of
// the first group beside the resize of the levels above it, the selection chain of a group beside FAST of the next
// (run_orb, rpe_api.hip).  The choice is by image count alone.  A captured batch is at most 2 * RPE_GRAPH_MAX_PAIRS
// images, so no hipGraph ever holds a fork: the captured sequences stay linear.
#define RPE_ORB_GROUP_MIN_IMAGES 33
#define RPE_ORB_GROUPS 2          // measured 2 / 3 / 4, either group order, either side-stream priority: DESIGN.md section 4, round 20
static_assert(RPE_ORB_GROUP_MIN_IMAGES > 2 * RPE_GRAPH_MAX_PAIRS, "a captured batch takes the linear schedule");
static_assert(RPE_ORB_GROUPS >= 2 && RPE_ORB_GROUPS <= RPE_ORB_GROUP_MAX, "rpe_orb_groups cuts at most RPE_ORB_GROUP_MAX groups");
#define RPE_MATCH_SPLIT_PAIRS 64   // batches up to this many pairs split a pair's Hamming matching over several workgroups
#define RPE_GUIDED_LDS_UINT4 128    // the guided matcher's part of the first LDS region: 2 x 32 scanned records of 32 bytes
#define RPE_TAB_RING 4            // pinned pieces the slot tables of rpe_frames_put* / rpe_enqueue_pairs rotate through
#define RPE_MAX_MATCHES_LIMIT 8064   // the largest cfg.max_matches rpe_create accepts: the most any kernel's LDS is sized for
#define RPE_MAX_IMAGE_DIM 4095       // the largest cfg.width / cfg.height rpe_create accepts
#define RPE_ORB_MAX_FEATURES 8000    // the largest cfg.nfeatures of an ORB handle
#define RPE_MAX_KCAP (RPE_SIFT_UNCAPPED_CAPACITY + 64)   // the largest keypoint capacity of a handle: uncapped SIFT's
#define RPE_CU_LDS_BYTES (160 * 1024)   // LDS of one gfx950 CU: the most a workgroup can ask for
#define RPE_LDS_DEFAULT_BYTES 65536     // the dynamic LDS a kernel may be launched with before its limit is raised
// A kernel that some handle rpe_create accepts launches with more than RPE_LDS_DEFAULT_BYTES, and the most any such handle
// asks of it.  Each kernel file lists its own, every launched template instance included, next to the layouts the
// ceilings come from (each static_asserted <= RPE_CU_LDS_BYTES); rpe_create raises them all, so no launcher touches the
// attribute.  The limit is per kernel and device and the ceilings depend on the build alone: repeating it is harmless.
struct RpeLdsCeiling { const void *kernel; const char *name; size_t bytes; };
std::vector<RpeLdsCeiling> rpe_orb_lds_ceilings();     // orb_kernels.hip
std::vector<RpeLdsCeiling> rpe_match_lds_ceilings();   // match_kernels.hip
std::vector<RpeLdsCeiling> rpe_geom_lds_ceilings();    // geom_kernels.hip
std::vector<RpeLdsCeiling> rpe_link_lds_ceilings();    // link_kernels.hip
std::vector<RpeLdsCeiling> rpe_similar_lds_ceilings(); // similar_kernels.hip
// one pair's results, section by section of the result block (d_resblk): R, t, inliers, status, n_matches
#define RPE_RESULT_SECTIONS 5
static const size_t kRpeResultElem[RPE_RESULT_SECTIONS] = {9 * sizeof(double), 3 * sizeof(double), sizeof(int), sizeof(int), sizeof(int)};
#define RPE_RESULT_BYTES 108     // their sum
// ---- the one ORB configuration: what the host tables (rpe_api.hip) and the kernels (orb_kernels.hip) share ----
// FAST tile = 64 x FAST_TH output pixels, 4 waves.  FAST is bound by instruction issue, not by latency like the resize
// kernel, and 32-row tiles with two waves only added halo work when they were tried: 4.43 -> 4.79 ms.
constexpr int FAST_TH = 64;
// The FAST tiles of a level start at (FAST_TILE_X0, RPE_EDGE): keypoints survive the border filter on [31, w - 31) x
// [31, h - 31) only, and the x origin is dword aligned.  The kernel loads a 4-pixel halo to the left of and above a tile
// without clamping at 0, which needs both origins >= 4.
constexpr int FAST_TILE_X0 = RPE_EDGE & ~3;
static_assert(FAST_TILE_X0 >= 4 && RPE_EDGE >= 4, "the FAST tile loads do not clamp x0 - 4 and y0 - 4 at 0");
constexpr int RPE_FAST_TILE_CAP = 1024;   // entries of one FAST tile list: the most strict 3x3 maxima a 64 x 64 tile can hold (32 x 32)
// The FAST tiles of a w x h level (build_tables lays them out), and the entries of its raster corner list (build_layout;
// the oracle mirrors this rule: orc_orb_corner_cap)
constexpr int rpe_fast_tiles(int w, int h)
{
    return w > 2 * RPE_EDGE && h > 2 * RPE_EDGE ? ((h - 2 * RPE_EDGE + FAST_TH - 1) / FAST_TH) * ((w - RPE_EDGE - FAST_TILE_X0 + 63) / 64) : 0;
}
constexpr int rpe_corner_cap(int w, int h)
{
    const long long c64 = (long long)w * h / 64;
    return (int)(c64 < 1024 ? 1024 : c64 > 8192 ? 8192 : c64);
}
// Resize tile = PYR_TW x PYR_TH destination pixels, one wave; its source window in the level below is PYR_ROWS rows of
// PYR_DW dwords (336 B = 21 16-byte loads, origin aligned down to 16 B).  build_tables checks every tile of a handle
// against the window at create time.  Why this shape: see pyr_resize_kernel.
constexpr int PYR_TW = 256, PYR_TH = 16;
constexpr int PYR_DW = 84, PYR_ROWS = 23;

// ---- HBM layout of one image's pyramid-shaped buffers ---------------------
// Level l is stored with row pitch align16(w_l) at byte offset off[l] (256-B
// aligned); images are `stride` bytes apart.  The raw pyramid, the FAST score /
// blurred pyramid buffer and the NMS buffer all use this layout.
struct RpeLevel {
    int w, h, pitch;
    int quota;        // features kept on this level (orb.cpp nfeaturesPerLevel)
    int ccap;         // capacity of the level's raster corner list: clamp(w h / 64, 1024, 8192) (cv2 has none: flagged when hit)
    int corner_off;   // offset of this level inside the per-image corner array
    int kcap2;        // capacity of the candidate list after retainBest(2 quota) (FAST-score ties extend it): 4 quota + 256
    int cand_off;     // offset of this level inside per-image candidate arrays
    float scale;      // (float)pow(1.1f, l)
    float inv_scale;  // 1.f / scale (orb.cpp's inv_scale: the level size and the keypoint's level coordinates come from it)
    long long off;    // byte offset inside the per-image pyramid buffer
    int coef_off;     // offset of xo/xa (w entries) then yo/ya (h entries) in the HOST coefficient table
    int dcoef_off;    // device table: [align128(w) packed x][align64(h) packed y], 16-B aligned, last entry replicated (build_tables)
    int tile0, ntile; // this level's run inside the FAST tile table (raster order inside the level)
};

struct RpeDeviceLayout {       // passed by value to kernels
    RpeLevel lv[RPE_NLEVELS];
    long long stride;          // bytes per image in pyramid-shaped buffers
    int corner_total;          // raster corner capacity per image (sum ccap)
    int cand_total;            // candidates capacity per image (sum kcap2)
    int stl;                   // C++ runtime whose nth_element orders the keypoints (rb::RT_LIBSTDCXX / rb::RT_MSVC, cfg.stl_runtime)
    int kcap;                  // keypoints capacity per image
    int fast_thr;
    // level 0 read IN PLACE from the caller's image batches when its pitch equals the image width (width % 16 == 0):
    // slot i < in_na is image i of in_a, the others image i - in_na of in_b (a consecutive-frame stream passes one
    // buffer and in_na = frames).  in_a == nullptr: level 0 was copied into the pyramid buffer like the other levels.
    const uint8_t *in_a, *in_b;
    int in_na, in_img;         // in_img = width * height
};

// base address of level l of image slot img (see in_a above)
__device__ __forceinline__ const uint8_t *rpe_level_base(const uint8_t *pyr, const RpeDeviceLayout &lay, int img, int l)
{
    if (l == 0 && lay.in_a)
        return img < lay.in_na ? lay.in_a + (long long)img * lay.in_img : lay.in_b + (long long)(img - lay.in_na) * lay.in_img;
    return pyr + (long long)img * lay.stride + lay.lv[l].off;
}

// Image slots of pair `pair`.  TAB = false, batch and stream: the rule (pair, img2_base + pair), and the kernel is the one
// those paths always ran.  TAB = true, rpe_enqueue_pairs: entry `pair` of the table, slot numbers of the frame store;
// `pair` comes from the workgroup index and `tab` is a kernel argument, so the lookup is uniform: one 8-byte scalar load
// per workgroup, no vector register, no per-lane load.  The switch is a template parameter and not a test of the
// pointer: the uniform load in front of the count loads cost the fused Hamming matcher 1 % (0.506 -> 0.512 ms per 1024
// pairs, four workgroups per CU one after the other) when the batch path carried it.
template <bool TAB>
__device__ __forceinline__ void rpe_pair_slots(const int2 *__restrict__ tab, int img2_base, int pair, int &img1, int &img2)
{
    if (TAB) { const int2 s = tab[pair]; img1 = s.x; img2 = s.y; }
    else { img1 = pair; img2 = img2_base + pair; }
}

// Camera source of the geometry kernels (rpe_*_cameras calls).  Every kernel that uses intrinsics carries a template
// switch CAM next to this argument, the pattern of rpe_pair_slots: CAM = false reads the shared d_K and is the instance
// every single-K path launches (the argument is then never read); CAM = true takes the two cameras of pair `pair` from
// `cams`: records (pair, img2_base + pair) of a batch's 2 B uploaded cameras, or, with `tab`, the frame store's per-slot
// records named by entry `pair` of the pair list's device table.  `pair` comes from the workgroup index and the rest
// from kernel arguments, so the 96-byte records are read with scalar loads, once per workgroup.
struct RpeCamSrc { const rpe_camera *cams; const int2 *tab; int img2_base; };

__device__ __forceinline__ void rpe_pair_cameras(const RpeCamSrc &src, int pair, const rpe_camera *&c1, const rpe_camera *&c2)
{
    int i1 = pair, i2 = src.img2_base + pair;
    if (src.tab) { const int2 s = src.tab[pair]; i1 = s.x; i2 = s.y; }
    c1 = src.cams + i1; c2 = src.cams + i2;
}

// The focal length used as a scale (RANSAC threshold, pixel scale of the refinement): (fx + fy) / 2 of K, or the mean
// of that over the pair's two cameras -- (a + a) / 2 == a, so equal cameras give the single-K bits
template <bool CAM>
__device__ __forceinline__ double rpe_pair_focal(const double *__restrict__ K, const RpeCamSrc &src, int pair)
{
    if (CAM) {
        const rpe_camera *c1, *c2;
        rpe_pair_cameras(src, pair, c1, c2);
        return (((c1->fx + c1->fy) / 2) + ((c2->fx + c2->fy) / 2)) / 2;
    } else {
        const double fx = K[0], fy = K[4];
        return (fx + fy) / 2;
    }
}

__device__ __forceinline__ bool rpe_camera_has_lens(const rpe_camera *c)
{
    bool lens = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) lens = lens || c->dist[k] != 0.;
    return lens;
}

// Normalised, undistorted coordinates of pixel p (include/rpe_amd.h, "camera models"): the single-K expression, then
// RPE_UNDISTORT_ITERS rounds of cv2.undistortPoints' fixed-point iteration when the camera has a lens.  Operation order
// of tests/camera_model.py; the build has no contraction, so the two agree bit for bit.
__device__ __forceinline__ double2 rpe_camera_normalise(const rpe_camera *c, bool lens, float2 p)
{
    const double xd = ((double)p.x - c->cx) / c->fx, yd = ((double)p.y - c->cy) / c->fy;
    double x = xd, y = yd;
    if (lens) {
        const double k1 = c->dist[0], k2 = c->dist[1], p1 = c->dist[2], p2 = c->dist[3];
        const double k3 = c->dist[4], k4 = c->dist[5], k5 = c->dist[6], k6 = c->dist[7];
#pragma unroll
        for (int it = 0; it < RPE_UNDISTORT_ITERS; ++it) {
            const double r2 = x * x + y * y;
            const double icd = (1 + r2 * (k4 + r2 * (k5 + r2 * k6))) / (1 + r2 * (k1 + r2 * (k2 + r2 * k3)));
            const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
            x = (xd - dx) * icd; y = (yd - dy) * icd;
        }
    }
    return make_double2(x, y);
}

// The normalisation of pair `pair`'s matches, the one every geometry kernel's d_n1 / d_n2 come from.  Built once per
// thread in front of the per-match part: the four scalars of K, or the pair's two cameras and their lens tests
// (workgroup-uniform scalar loads, a uniform branch).  Applied per match: the two pixel points of a match -> the
// normalised (CAM: and undistorted, each with the camera of its own frame) coordinates.
template <bool CAM>
struct RpePairNormalise {
    const rpe_camera *c1, *c2;
    bool lens1, lens2;
    double fx, fy, cx, cy;
    __device__ __forceinline__ RpePairNormalise(const double *__restrict__ K, const RpeCamSrc &src, int pair)
    {
        if (CAM) {
            rpe_pair_cameras(src, pair, c1, c2);
            lens1 = rpe_camera_has_lens(c1); lens2 = rpe_camera_has_lens(c2);
        } else {
            fx = K[0]; fy = K[4]; cx = K[2]; cy = K[5];
        }
    }
    __device__ __forceinline__ void operator()(float2 a, float2 b, double2 &na, double2 &nb) const
    {
        if (CAM) {
            na = rpe_camera_normalise(c1, lens1, a);
            nb = rpe_camera_normalise(c2, lens2, b);
        } else {
            na = make_double2(((double)a.x - cx) / fx, ((double)a.y - cy) / fy);
            nb = make_double2(((double)b.x - cx) / fx, ((double)b.y - cy) / fy);
        }
    }
};

// Inclusive prefix operations over the 64 lanes with DPP row shifts / row broadcasts: 6 v_<op>_dpp instead of 6 rounds of
// ds_bpermute + select + op (~30 vector + LDS instructions).  Shifted-out lanes read the `old` operand, the identity.
// The wave total is the value of lane 63 (__builtin_amdgcn_readlane(x, 63)).
// A lane that is switched off also reads as the identity and is not written: every call site runs with all 64 lanes of
// the wave active (the early returns in front of the SIFT ones -- band / keypoint index, empty band, redo gate -- depend
// on the wave's index only), and a new one must too.
#define RPE_WAVE_SCAN(NAME, OP, IDENT)                                                                            \
    __device__ __forceinline__ int NAME(int v)                                                                    \
    {                                                                                                             \
        v = OP(v, __builtin_amdgcn_update_dpp(IDENT, v, 0x111, 0xF, 0xF, false));      /* row_shr:1 */            \
        v = OP(v, __builtin_amdgcn_update_dpp(IDENT, v, 0x112, 0xF, 0xF, false));      /* row_shr:2 */            \
        v = OP(v, __builtin_amdgcn_update_dpp(IDENT, v, 0x114, 0xF, 0xF, false));      /* row_shr:4 */            \
        v = OP(v, __builtin_amdgcn_update_dpp(IDENT, v, 0x118, 0xF, 0xF, false));      /* row_shr:8 */            \
        v = OP(v, __builtin_amdgcn_update_dpp(IDENT, v, 0x142, 0xA, 0xF, false));      /* row_bcast:15 -> rows 1, 3 */ \
        v = OP(v, __builtin_amdgcn_update_dpp(IDENT, v, 0x143, 0xC, 0xF, false));      /* row_bcast:31 -> rows 2, 3 */ \
        return v;                                                                                                 \
    }
#define RPE_OP_ADD(a, b) ((a) + (b))
#define RPE_OP_MAX(a, b) max((a), (b))
#define RPE_OP_MIN(a, b) min((a), (b))
RPE_WAVE_SCAN(wave_inclusive_sum, RPE_OP_ADD, 0)
RPE_WAVE_SCAN(wave_inclusive_max, RPE_OP_MAX, (int)0x80000000)
RPE_WAVE_SCAN(wave_inclusive_min, RPE_OP_MIN, 0x7FFFFFFF)
__device__ __forceinline__ int wave_sum(int v) { return __builtin_amdgcn_readlane(wave_inclusive_sum(v), 63); }
// exclusive scan over a 256-thread workgroup (all of it takes part: two barriers inside); total = the sum of all 256.
// s_wave: one LDS word per wave
__device__ __forceinline__ int block_excl_scan(int v, int *s_wave /*[4]*/, int &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int inc = wave_inclusive_sum(v);
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { int s = s_wave[k]; if (k < wv) base += s; }
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return base + inc - v;
}
// Cross-wave election over a 256-thread workgroup (all of it takes part: one barrier inside).  Each wave brings its best
// (count, key), key < 0 = none; every thread gets the winner: the largest count, the lowest key among equal counts, or
// (-1, -1) when no wave has a candidate.  s_best: eight LDS words
__device__ __forceinline__ void elect_best(int best_cnt, int best_key, int *s_best /*[8]*/, int &win_cnt, int &win_key)
{
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_best[wv * 2] = best_cnt; s_best[wv * 2 + 1] = best_key; }
    __syncthreads();
    win_cnt = -1; win_key = -1;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = s_best[w * 2], key = s_best[w * 2 + 1];
        if (key >= 0 && (c > win_cnt || (c == win_cnt && key < win_key))) { win_cnt = c; win_key = key; }
    }
}
// the sum of cnt over a 256-thread workgroup, on every thread (all of it takes part: one barrier inside), the waves added
// in wave order.  s_cnt: one LDS word per wave
__device__ __forceinline__ int block_count(int cnt, int *s_cnt /*[4]*/)
{
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    return (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// this thread's index in a one-thread-per-item launch of 256-thread workgroups, -1 past n.  The product is 64-bit, so the
// bound holds for every n an int can be
__device__ __forceinline__ int tk_thread_index(int n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    return i < n ? (int)i : -1;
}

struct RpeTile { short level, tx, ty, pad; };
// destination tile of the resize kernel: its origin, the origin of its source window in the level below, the number of
// source rows its destination rows read (nsrc <= PYR_ROWS; window rows past it are neither loaded nor stored) and the rows
// whose top source row is the row below the previous row's (bit r of reuse, 0 < r < PYR_TH: yo[y0 + r] == yo[y0 + r - 1] + 1).
// One 16-byte scalar load per wave.
struct alignas(16) RpePyrTile { short x0, y0, a0, sy0; unsigned short nsrc, reuse; int pad; };
static_assert(sizeof(RpePyrTile) == 16 && PYR_TH <= 16, "one reuse bit per tile row");
// device y table of the resize kernel: (byte offset of the source row in a window-pitch array) | (bottom-row weight << PYR_YW_SHIFT)
constexpr int PYR_YW_SHIFT = 23;

// per-pair RANSAC state in HBM
struct RpeRansacState {
    int best_count;   // maxGoodCount
    int best_iter;
    int best_model;
    int niters;       // current loop bound
    int next_iter;    // first iteration of the next chunk
    int done;
    int found;
    int M;
    int iters_run;    // loop trip count so far (ptsetreg.cpp `iter` at exit)
    int pad_;
    double E[9];      // best model so far
};

struct RpeSiftState;

// Where the matchers and the status test find the features of pair p: the extraction workspace under the rule
// (p, img2_base + p), or the frame store under a pair table
struct RpeFeatSrc { const uint8_t *desc; const int *count; const float2 *pt; const int2 *norm; const int2 *tab; int img2_base; };

// What one launch sequence operates on.  The entry points build it (rpe_run_batch / rpe_run_stream / rpe_run_list below)
// and hand it to the launchers of match_kernels.hip, geom_kernels.hip and link_kernels.hip, which read nothing of it from
// the handle.
struct RpeRun {
    int pairs;
    RpeFeatSrc feat;
    RpeCamSrc cam;        // cam.cams == nullptr: the shared d_K and the kernels' CAM = false instances
};

// The last run, for the calls that come behind it (the table at last_run_gate, rpe_api.hip, names them and what each needs;
// those that launch again do so on exactly `run`).  Written by last_run_begin, last_run_end, last_run_store_changed and
// last_run_structure (rpe_api.hip) and by nothing else; read through last_run_gate.
struct RpeLastRun {
    enum Kind { NONE, RULE, LIST, CHUNKED };   // nothing / a batch or stream under the rule / a pair list / a host batch run in chunks
    Kind kind = NONE;
    int pairs = 0;                    // CHUNKED: of the whole batch
    RpeRun run{};
    std::vector<int> tab;             // LIST: its (slot1, slot2) entries; emptied when the store is resized
    std::vector<uint32_t> ovf;        // CHUNKED: capacity flags per pair (OR of the pair's two images), collected across the chunks
    bool per_match = false;           // d_pts*, d_n*, d_rstate, d_mask, d_R / d_t still hold the run's per-match data
    int structure = 0;                // pairs [0, structure) of the run have d_mask (status form), d_pose_mask and d_points filled
};

// The device buffers of one first-use feature: one hipMalloc, carved into the fields of the feature's record by rpe_bufset_fit (below)
struct RpeBufSet { uint8_t *block = nullptr; size_t bytes = 0; };

// One job of the track kernels (track_kernels.hip): P pairs over n_frames frames, pair p between frames[p].x and frames[p].y,
// its matches at p * max_matches.  Run form: the run's own match lists, status and masks (rmask / pmask read only under the
// rules that name them), use_pair or null, edge null.  Stage form: the uploaded lists, rule ALL, edge or null.  pts1 == null:
// obs_xy is zero
struct RpeTrackJob {
    int P, n_frames, rule, min_len;
    const int2 *frames;
    const int *m_n, *q, *t;
    const uint8_t *use_pair, *edge;
    const int *status;
    const uint8_t *rmask, *pmask;
    const float2 *pts1, *pts2;
};
#define RPE_TRACK_NODE_WORDS 11   // int arrays of one word per node in RpeTrackBufs::node
static inline int rpe_track_scan_blocks(int N) { return (int)(((long long)N + 2047) / 2048); }   // workgroups of the track scans (2048 nodes each)
// rpe_build_tracks / rpe_tracks_from_matches only (set, fitted to every call's n_frames).  Per match slot [max_batch * max_matches]: the
// edge flag and match_track; the stage form's uploaded lists (q / t / edge / pts1 / pts2) and per pair its match
// count; per pair of either form the frame pair and use_pair.  Outputs: counts[8], track_start [slots + 1], observations
// [2 * slots].  Per node (n_frames * kcap of them): node, RPE_TRACK_NODE_WORDS arrays of one word each, with
// partial (one int2 per scan workgroup); seen [n_frames]: the set's last pieces, so n_frames moves no other
struct RpeTrackBufs {
    uint8_t *eflag = nullptr, *edge = nullptr, *use = nullptr;
    int *mtrack = nullptr, *q = nullptr, *t = nullptr, *m = nullptr, *counts = nullptr;
    int *tstart = nullptr, *oframe = nullptr, *okp = nullptr;
    float2 *oxy = nullptr, *pts1 = nullptr, *pts2 = nullptr;
    int2 *frames = nullptr, *partial = nullptr;
    int *node = nullptr, *seen = nullptr; RpeBufSet set;
    std::vector<int> frame_tab;           // host side of frames: source of its upload
};

// The track scene (track_scene.h) on the device, as scene_upload (rpe_features.hip) left it: the tracks, the poses and the cameras
// (cam_stride 1: one per frame; 0: the one record K became)
struct RpeTrackScene {
    int n_tracks, n_obs, cam_stride;
    const int *track_start, *obs_frame; const float2 *obs_xy;
    const double *R, *T; const rpe_camera *cams;
};

// One job of the track-point kernels (track_point_kernels.hip): the scene and the uploaded groups (null: all 0)
struct RpeTrackPointJob {
    RpeTrackScene scene;
    int min_views, max_iters;
    double threshold_px, max_cos;
    const int *group;
};

// rpe_triangulate_tracks only (set, fitted to every call's tracks, observations and frames), beside the scene.
// Per track: point, info[4], rms, min_cos out.  Per observation: the record between the two kernels (TpObs,
// track_point_kernels.hip), flag and error out.  Per frame: group
#define RPE_TRACK_POINT_OBS_BYTES 80   // one TpObs
struct RpeTrackPointBufs {
    int *group = nullptr, *info = nullptr;
    uint8_t *obs = nullptr;               // [n_obs] records of RPE_TRACK_POINT_OBS_BYTES
    double *points = nullptr, *rms = nullptr, *mincos = nullptr, *oerr = nullptr;
    uint8_t *oflag = nullptr; RpeBufSet set;
};

// One job of the window-bundle kernels (window_kernels.hip): the scene and the uploaded start points, masks (null: all set)
// and windows
struct RpeWindowJob {
    RpeTrackScene scene;
    int n_win, max_points, min_obs, max_iters;
    const double *points0;
    const uint8_t *point_use, *obs_use;
    const int *win_start, *win_frame;
};

// rpe_bundle_windows only (set, fitted to every call's tracks, observations and windows), beside the scene.  The
// uploads of its own (start points, masks, windows); per observation the record of wb_prepare (WbObs, window_kernels.hip);
// per window and point slot [n_win * max_points]: the track, the observation of each window position, the state (X and
// the trial X) and the output point; per window frame the output pose
#define RPE_WINDOW_OBS_BYTES 32       // one WbObs
#define RPE_WINDOW_SLOT_OBS RPE_WINDOW_MAX_VIEWS   // ints of a point slot's observation list: one per window position
#define RPE_WINDOW_STATE_DOUBLES 6    // f64 of a point slot's state: X, then the trial X
struct RpeWindowBufs {
    int *wstart = nullptr, *wframe = nullptr;
    int *ptrack = nullptr, *pobs = nullptr, *counts = nullptr, *info = nullptr, *fcnt = nullptr;
    uint8_t *obs = nullptr;               // [n_obs] records of RPE_WINDOW_OBS_BYTES
    double *points0 = nullptr, *state = nullptr, *points = nullptr;
    double *Rout = nullptr, *Tout = nullptr, *rms = nullptr;
    uint8_t *puse = nullptr, *ouse = nullptr; RpeBufSet set;
};

// One job of the pose-graph kernel (graph_kernels.hip): the caller's poses and measurements as uploaded, the graphs in CSR
// form, and what the host made of them (rpe_optimise_graphs): per graph the offsets of its free frames and used edges and
// the code it already has (-1: solve); per free frame its graph position and its adjacency (adj_start, global offsets into
// adj: x = used edge of the graph << 1 | side, side 1 = the frame is the edge's j; y = free index of the other end or -1),
// per used edge its position in the graph's edge list, per edge the graph positions of its ends
struct RpeGraphJob {
    int n_graphs, max_iters, cg_iters;
    double huber, cg_tol;
    const double *R_abs, *T_abs, *edge_R, *edge_t, *edge_w;
    const int *graph_start, *graph_frame, *edge_start, *free_start, *used_start, *precode;
    const int *free_pos, *adj_start, *used_edge, *edge_i, *edge_j, *edge_kind;
    const int2 *adj;
};

// rpe_optimise_graphs only (set, fitted to every call's frames, graphs and edges).  The uploads: the caller's poses
// and measurements, the CSR arrays and the host's tables (RpeGraphJob); per graph position the state (the output) and the
// trial state; per used edge its blocks, per free frame its block, factor and PCG vectors (the layouts: graph_kernels.hip);
// per edge the two chi, per graph cost and info
#define RPE_GRAPH_EDGE_DOUBLES 120    // f64 of a used edge's blocks (PG_EB)
#define RPE_GRAPH_FRAME_DOUBLES 87    // f64 of a free frame's block, factor and PCG vectors (PG_FB)
struct RpeGraphBufs {
    double *Rabs = nullptr, *Tabs = nullptr, *eR = nullptr, *et = nullptr, *ew = nullptr;
    int *gstart = nullptr, *gframe = nullptr, *estart = nullptr, *fstart = nullptr, *ustart = nullptr;
    int *precode = nullptr, *fpos = nullptr, *astart = nullptr, *uedge = nullptr;
    int *ei = nullptr, *ej = nullptr, *ekind = nullptr, *info = nullptr;
    int2 *adj = nullptr;
    double *Rout = nullptr, *Tout = nullptr, *Rn = nullptr, *Tn = nullptr;
    double *eb = nullptr, *fb = nullptr, *chi = nullptr, *cost = nullptr; RpeBufSet set;
};

// One job of the similarity kernels (similar_kernels.hip): the features (the frame store's, or the workspace's of the stage
// form), the two device tables of slots, the times (the tables themselves when the caller gave none) and where the results go.
// same: the two lists are identical, the triangle is computed and mirrored.  cand == null: no selection
struct RpeSimilarJob {
    const uint8_t *desc;
    const int *count;
    int nq, nt;
    const int *q, *t;
    int step, max_distance;
    bool same;
    const int *q_time, *t_time;
    int exclude, min_score, k;
    int *scores, *cand, *cand_score, *n_cand;
};

// rpe_frames_similar / rpe_similarity_hamming only (set, fitted to every call's lists): the two slot tables (not
// d_pairtab, which holds 2*max_batch entries: a list here may be as long as the store), the times the caller gave, the
// nq * nt scores, and per query row its k candidates, their scores and their count
struct RpeSimilarBufs {
    int *q = nullptr, *t = nullptr, *qtime = nullptr, *ttime = nullptr;
    int *scores = nullptr, *cand = nullptr, *cscore = nullptr, *ncand = nullptr; RpeBufSet set;
};

// One rpe_scale_links link on the device: pairs a and b of the last run, side bit 0 / 1 = the shared frame is image 2 of a / of b
struct RpeLink { int a, b, side, pad; };
// What the link kernels (link_kernels.hip) read of the last run, by value (rpe_link_src fills it from the handle): the link
// table; the run's match lists, status, the two structure masks, points and poses; its normalised points; the capacities
// of a pair's match arrays and of a frame's keypoints.  Everything is indexed from the workgroup's link, so the link, the
// two pairs' status, counts and poses are uniform scalar loads.
struct RpeLinkSrc {
    const RpeLink *links;
    const int *m_q, *m_t, *m_n, *status;
    const uint8_t *ransac_mask, *pose_mask;
    const double *points, *R, *t;
    const double2 *n1, *n2;
    int max_matches, kcap;
};

// The link calls' table (links, created on first use, 4*max_batch links; tab: its host side, the table of the last link
// call and the source of its upload) and rpe_scale_links' outputs (set, fitted on first use)
struct RpeLinkBufs {
    RpeLink *links = nullptr;
    std::vector<RpeLink> tab;
    double *stats = nullptr;              // [link][3] lower quartile, median, upper quartile
    int *n = nullptr, *code = nullptr; RpeBufSet set;
};

// rpe_link_poses only (set, fitted on first use): per link the pose, {n, inliers}, info[4], rms[2] and the inlier mask
// [link][max_matches], 4*max_batch links (the link table is RpeLinkBufs::links); corr [link][RPE_LINK_POSE_CORR_DOUBLES *
// max_matches] holds the correspondence lists of handles above the kernel's LDS cut only (a piece of 0 bytes, null, on the others)
#define RPE_LINK_POSE_CORR_DOUBLES 5  // f64 of one correspondence: X[3], then q[2]
struct RpeLinkPoseBufs {
    double *R = nullptr, *t = nullptr, *rms = nullptr, *corr = nullptr;
    int *counts = nullptr, *info = nullptr;
    uint8_t *mask = nullptr; RpeBufSet set;
};

// rpe_link_bundles / rpe_bundle_three_view only (set, fitted on first use), 4*max_batch problems.  The problems' arrays,
// indexed by pair a's match index (stage form: point number): view code [prob][max_matches], observations
// [prob][max_matches][RPE_BUNDLE_OBS_DOUBLES] (S, A, C), points [prob][max_matches][3] (start points in, results out); per
// problem the scan length, the code decided before the bundle, the start poses in the solved form [RPE_BUNDLE_POSE_DOUBLES]
// and the focal scales [2]; the callers' poses of pair b; the results; state [prob][RPE_BUNDLE_STATE_DOUBLES * max_matches]
// holds the point state of handles above the kernel's LDS cut only (a piece of 0 bytes, null, on the others)
#define RPE_BUNDLE_OBS_DOUBLES 6      // f64 of a point's observations: S x, y, A x, y, C x, y
#define RPE_BUNDLE_POSE_DOUBLES 24    // f64 of a problem's start poses: R, t of S -> A, then of S -> C
#define RPE_BUNDLE_STATE_DOUBLES 6    // f64 of a point's state: X, then the trial X
struct RpeBundleBufs {
    uint8_t *views = nullptr; RpeBufSet set;
    double *obs = nullptr, *points = nullptr, *pose0 = nullptr, *focal = nullptr, *state = nullptr;
    double *Rin = nullptr, *tin = nullptr;
    int *n = nullptr, *pre = nullptr, *counts = nullptr, *info = nullptr;
    double *Ra = nullptr, *ta = nullptr, *Rb = nullptr, *tb = nullptr, *rms = nullptr;
};

// rpe_refine_poses / rpe_refine_pose_points only (set, fitted on first use): refined pose, cheirality count, info[4],
// rms[2] per pair; start pose of the stage form
struct RpeRefineBufs {
    double *R = nullptr, *t = nullptr, *rms = nullptr, *R0 = nullptr, *t0 = nullptr;
    int *inl = nullptr, *info = nullptr; RpeBufSet set;
};

// The guided matchers of either norm only (rpe_guided_matches[_l2], rpe_match_hamming_guided, rpe_match_l2_guided; set,
// fitted on first use): match lists of their own, shaped like the run's d_m_* / d_pts* (d: int32 Hamming distances, or f32
// L2 distances in the same four bytes); the poses gated with when the caller supplies them; per pair and image one 32-byte
// record per keypoint [pair][RPE_GUIDED_SIDES][kcap] and the squared threshold (see guided_records_kernel)
#define RPE_GUIDED_SIDES 2            // record lists of a pair: one per image
struct RpeGuidedBufs {
    int *q = nullptr, *t = nullptr, *d = nullptr, *n = nullptr;
    float2 *pts1 = nullptr, *pts2 = nullptr;
    double *R = nullptr, *tr = nullptr, *thr2 = nullptr;
    double4 *rec = nullptr; RpeBufSet set;
};

// rpe_pair_homographies / rpe_find_homography only (set, fitted on first use): H, R_rot, {n_H, n_rot, n_E} and info[4]
// per pair, the winner's inlier mask [pair][max_matches]
struct RpeHomographyBufs {
    double *H = nullptr, *R = nullptr;
    int *counts = nullptr, *info = nullptr;
    uint8_t *mask = nullptr; RpeBufSet set;
};

// The track scene of rpe_triangulate_tracks and rpe_bundle_windows (set, fitted to every call's tracks, observations and
// frames by scene_upload; either call uploads its own scene, none is kept).  Per track the CSR offsets, per observation
// frame and pixel, per frame R, T and camera (cam_k: the host side of the one record K becomes)
struct RpeSceneBufs {
    int *tstart = nullptr, *oframe = nullptr; float2 *oxy = nullptr;
    double *R = nullptr, *T = nullptr; rpe_camera *cams = nullptr;
    rpe_camera cam_k{}; RpeBufSet set;
};

struct rpe_handle {
    rpe_config cfg;
    RpeSiftState *sift = nullptr;             // SIFT workspace (feature_method == RPE_FEATURE_SIFT)
    int desc_bytes = 32;                      // 32 (rBRIEF) or 128 (SIFT, stored as u8)
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;          // uploads of a chunked host batch (rpe_estimate_batch), created on first use
    hipEvent_t ev_up[8] = {};                   // 'chunk c is resident' events
    // hipGraphs of the whole launch sequence of small batches (rpe_enqueue_batch_device): the drop-in's estimate() is a batch
    // of ONE pair, ~50 launches of a few microseconds each; replaying them as one graph removes the per-launch host cost
    struct GraphEntry { const uint8_t *a, *b; int B; hipGraph_t graph; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    RpeLastRun last;
    std::vector<void *> dev_allocs;             // every device buffer of the handle but the frame store's: workspace, tables, created-on-first-use; rpe_destroy frees them
    RpeDeviceLayout lay{};
    int n_img_cap = 0;              // 2*max_batch
    // tile tables
    RpeTile *d_tiles_fast = nullptr;  int n_tiles_fast = 0;   // tiles covering [28,w-28)x[28,h-28)
    int *d_coef = nullptr;            // resize coefficient tables
    RpePyrTile *d_pyr_tiles = nullptr;  // resize tiles of levels 1..11, level l at pyr_tile_off[l], raster order
    int pyr_tile_off[RPE_NLEVELS] = {}, pyr_tile_cnt[RPE_NLEVELS] = {};
    // the grouped detection schedule of batches of RPE_ORB_GROUP_MIN_IMAGES images and more (run_orb): the level groups
    // (build_tables), the stream that FAST of group 0 and the chains of all groups but the last run on, one event per
    // group ('what group g's side-stream work reads is written') and the 'side stream is done' event; the events carry no timing
    RpeOrbGroup orb_group[RPE_ORB_GROUPS] = {};
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork[RPE_ORB_GROUPS] = {}, ev_join = nullptr;
    // image-shaped buffers
    uint8_t *d_pyr = nullptr;
    unsigned *d_tile_list = nullptr;  // [img][n_tiles_fast][RPE_FAST_TILE_CAP] score << 24 | y << 12 | x
    int *d_tile_cnt = nullptr;        // [img][n_tiles_fast]
    uint8_t *d_stage1 = nullptr, *d_stage2 = nullptr; // staging for host-image API
    // detection
    unsigned *d_corner = nullptr;     // [img][corner_total] raster-ordered FAST corners of a level: score << 24 | y << 12 | x
    int *d_corner_count = nullptr;    // [img][level]
    int *d_kp_lvl_count = nullptr;    // [img][level] keypoints kept per level (head of the level's candidate run)
    unsigned *d_cand_xy = nullptr;    // [img][cand_total]  y<<16|x
    float *d_cand_resp = nullptr;     // [img][cand_total]
    int *d_cand_count = nullptr;      // [img][level]
    unsigned *d_kp_xy = nullptr;      // [img][kcap]  x | y<<12 | level<<24
    float *d_kp_resp = nullptr, *d_kp_angle = nullptr;
    float2 *d_kp_pt = nullptr;
    int *d_kp_count = nullptr;        // [img]
    unsigned *d_ovf = nullptr;        // [img] RPE_OVF_* capacity flags of the last extraction
    int level0_slots = 0;             // image slots of the last ORB run (debug fetch of an in-place level 0)
    uint8_t *d_desc = nullptr;        // [img][kcap][32]
    // debug fetch only: rpe_orb_debug_fetch(which = 3) blurs whole levels of ONE image with blur_kernel
    RpeTile *d_tiles_full = nullptr;  int n_tiles_full = 0;   // 64 x 64 tiles covering every level
    uint8_t *d_bufA = nullptr;        // that image's blurred pyramid
    // matching
    int *d_m_q = nullptr, *d_m_t = nullptr, *d_m_d = nullptr, *d_m_n = nullptr;
    unsigned long long *d_m_best = nullptr;   // L2 matcher: [pair][kcap] per train: packed (f32 dist bits << 18 | queryIdx) of its nearest query
    int *d_m_norm = nullptr;                  // L2 matcher: [img][kcap][2] { |u|^2, |u|^2 + 2 sum(u) }, u = byte - 128, of every descriptor
    unsigned *d_hm_best = nullptr, *d_hm_row = nullptr;   // Hamming matcher, small batches (<= RPE_MATCH_SPLIT_PAIRS pairs): election / own-nearest words in HBM
    unsigned long long *d_m_best2 = nullptr;  // L2 matcher: [pair][kcap] per query: the same key of its nearest train (the ratio mode's only list)
                                              // both lists are scratch of one launch sequence: the guided L2 matcher (rpe_launch_guided_l2) elects into them too
    float2 *d_pts1 = nullptr, *d_pts2 = nullptr;   // [pair][max_matches]
    // RANSAC
    unsigned short *d_subsets = nullptr;  // [M 0..max_matches][iters][5]
    double *d_nit_denom = nullptr;        // [(M,g)] log(1-(1-ep)^5) or NaN-coded flags
    int *d_nit_round = nullptr;           // [(M,g)] cvRound(num/denom), -1 => denom<DBL_MIN (return 0)
    double nit_num = 0;                   // log(1-p)
    RpeRansacState *d_rstate = nullptr;
    double2 *d_n1 = nullptr, *d_n2 = nullptr;   // K-normalised matched points [pair][max_matches]
    int *d_found = nullptr;                   // [pair] 0 none, 1 one model, n > 1: n stacked models (exactly 5 matches)
    double *d_hyp = nullptr;              // [pair][88][64] per-hypothesis record between the two solver kernels
    double *d_models = nullptr;           // [pair][CHUNK][10][9]
    int *d_nmodels = nullptr;             // [pair][MAXCHUNK]
    int *d_counts = nullptr;              // [pair][MAXCHUNK][10] inlier counts of the current chunk
    uint8_t *d_mask = nullptr;            // [pair][max_matches]
    uint8_t *d_pose_mask = nullptr;       // [pair][max_matches] rpe_fetch_structure only (created on first use)
    double *d_points = nullptr;           // [pair][max_matches][3] rpe_fetch_structure only (created on first use)
    // the first-use features: one record each (above, beside the feature's job)
    RpeRefineBufs ref; RpeLinkBufs link; RpeLinkPoseBufs lp; RpeBundleBufs ba; RpeGuidedBufs gm; RpeHomographyBufs hg;
    RpeTrackBufs tk; RpeSceneBufs scene; RpeTrackPointBufs tp; RpeWindowBufs wb; RpeGraphBufs pg; RpeSimilarBufs sim;
    // results
    double *d_R = nullptr, *d_t = nullptr, *d_E = nullptr;
    int *d_inliers = nullptr, *d_status = nullptr;
    double K_last[9] = {0}; bool K_valid = false;        // camera matrix resident in d_K (re-uploaded only when it changes)
    uint8_t *d_resall = nullptr; unsigned *d_ovfall = nullptr;   // whole-batch result block / flag words of a chunked host batch (created on first use)
    uint8_t *d_resblk = nullptr, *h_resblk = nullptr;   // d_R, d_t, d_inliers, d_status, d_m_n live in d_resblk; pinned host mirror
    double *d_K = nullptr;
    // Frame store (rpe_frames_*): per-frame features resident across calls, [slot][kcap] like the workspace arrays they
    // are scattered from, so the pair kernels index them with the same arithmetic.  One allocation per array;
    // rpe_frames_reserve builds the new set, copies the kept slots and frees the old one.
    struct FrameStore {
        int cap = 0;
        uint8_t *d_desc = nullptr;        // [slot][kcap][desc_bytes]
        float2 *d_kp_pt = nullptr;        // [slot][kcap]
        int2 *d_norm = nullptr;           // [slot][kcap] NORM_L2 handles only (either match mode): the MFMA matchers' norm words, computed at put time
        int *d_count = nullptr;           // [slot] keypoints (0 for a slot never filled)
        unsigned *d_ovf = nullptr;        // [slot] RPE_OVF_* flags of the extraction that filled the slot
        std::vector<uint8_t> filled;      // [slot] host side: the slot holds a frame (argument checks never read the device)
        rpe_camera *d_cam = nullptr;      // [slot] camera of the slot's frame (rpe_frames_set_cameras)
        std::vector<rpe_camera> h_cam;    // [slot] host mirror: source of the uploads, kept across rpe_frames_reserve
        std::vector<uint8_t> has_cam;     // [slot] host side: the slot has been given a camera
    } fs;
    int *h_pairtab = nullptr;             // pinned, RPE_TAB_RING pieces of 2*max_batch ints: slot list of a put / (slot1, slot2) table of a pair list
    int *d_pairtab = nullptr;             // device copy, uploaded on the handle's stream
    hipEvent_t ev_tab[RPE_TAB_RING] = {}; // piece r of h_pairtab has been uploaded (the call that takes it next may overwrite it)
    int tab_next = 0;
    rpe_camera *d_batch_cams = nullptr;   // [2*max_batch] cameras of a camera batch / stage call: cam1[0, B) then cam2[0, B) (created on first use)
    std::vector<rpe_camera> h_batch_cams; // their host staging
    // profiling
    unsigned *d_calib_sink = nullptr;     // one word the rpe_calibrate_* kernels name as their output and never write (created on first use)
    bool profiling = false;
    hipEvent_t ev[RPE_STAGE_COUNT + 1] = {};
    bool ev_valid = false;
    int ev_first = 0;                     // first stage the last profiled call ran (a pair list starts at RPE_STAGE_MATCH)
    std::vector<void *> user_allocs;            // rpe_device_malloc: the caller's buffers
};

// Every device buffer of the handle (the frame store keeps its own set, caller buffers are in user_allocs) comes from
// here: rpe_destroy frees what this recorded, and nothing else frees it.
template <typename T>
static int dmalloc(rpe_handle *h, T **p, size_t n)
{
    const hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) { *p = nullptr; h->err = std::string("hipMalloc failed: ") + hipGetErrorString(e); return RPE_ERR_HIP; }
    h->dev_allocs.push_back(*p);
    return RPE_OK;
}
#define DM(h, p, n) do { int r_ = dmalloc(h, &(p), (size_t)(n)); if (r_) return r_; } while (0)
// a single buffer created on first use
#define DM_ONCE(h, p, n) do { if (!(p)) DM(h, p, n); } while (0)

// The buffers a feature creates on first use are ONE set of its record and ONE piece list -- the record's fields with the
// sizes THIS call needs -- given to rpe_bufset_fit behind the host-side checks and hipSetDevice, before the first upload:
//   layout   piece i sits at the running sum of the 256-byte-aligned sizes of the pieces before it; the total is that sum,
//            and at least 256 (buf_layout.h).  A piece of 0 bytes gets nullptr.
//   growth   total > set.bytes: wait on the handle's stream if there is a block (growth is rare, and a call that returned
//            early behind a launch may have left work in flight), take the block out of dev_allocs and free it, empty the
//            set and null every piece, allocate exactly `total`: freed first, so a growth never holds both blocks.  A
//            failure returns RPE_ERR_HIP with the set empty and the pointers null: the next call tries again.  No shrinking.
//   carving  every call assigns every piece from its own sizes: a smaller call is carved smaller inside the same block; sizes
//            of the configuration alone give a constant total, so those pointers never move after the first call.
// Nothing in a set outlives its call (inputs are uploaded or written by the call's own kernels, outputs fetched before it
// returns; d_pose_mask and d_points do persist and stay DM_ONCE buffers), and none is part of a captured graph.  That is
// also why two features may share a set: scene.set serves the track points and the window bundles, each beside its own.
// A set fitted to the call's own sizes names, with each piece, the host array the call uploads into it (src, or null):
// the one list is fitted and then walked by rpe_bufset_upload, so a copy is exactly as long as its piece.
struct RpeBufPiece { void **p; size_t bytes; const void *src; };
template <typename T>
static inline RpeBufPiece buf_piece(T *&p, size_t n, const void *src = nullptr) { return {(void **)&p, n * sizeof(T), src}; }
int rpe_bufset_fit(rpe_handle *h, RpeBufSet &s, std::initializer_list<RpeBufPiece> pieces);   // rpe_api.hip
// the upload rule (rpe_host.h) over a fitted list: every piece that has a source and bytes, on the handle's stream, no wait
int rpe_bufset_upload(rpe_handle *h, std::initializer_list<RpeBufPiece> pieces);              // rpe_api.hip

// A failed HIP call ends the entry point: the text goes to the handle, or (rpe_create, no handle yet) to the create-time string
extern std::string g_create_err;
#define HIPCHK(h, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            char b_[512];                                                                       \
            snprintf(b_, sizeof(b_), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (h) (h)->err = b_; else g_create_err = b_;                                       \
            return RPE_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

// cv2's cvRound of a double: to nearest, ties to even
static inline int cv_round(double v) { return (int)lrint(v); }

// The refusal of an argument head: every failed call leaves a text of its own for rpe_last_error (h == NULL: nowhere to)
static inline int rpe_invalid(rpe_handle *h, const char *who, const char *what = RPE_NULL_ARGUMENT_TEXT)
{
    if (h) h->err = std::string(who) + ": " + what;
    return RPE_ERR_INVALID;
}

// The runs.  `cam` defaults to the shared K; a camera source must address its records as the run addresses its images.
static inline RpeRun rpe_run_rule(const rpe_handle *h, int pairs, int img2_base, RpeCamSrc cam)
{
    return {pairs, {h->d_desc, h->d_kp_count, h->d_kp_pt, (const int2 *)h->d_m_norm, nullptr, img2_base}, cam};
}
// B pairs on the workspace slots (p, B + p): a batch, and a stage call over B uploaded pairs
static inline RpeRun rpe_run_batch(const rpe_handle *h, int B, RpeCamSrc cam = {nullptr, nullptr, 0}) { return rpe_run_rule(h, B, B, cam); }
// pairs + 1 consecutive frames: pair p on the workspace slots (p, p + 1)
static inline RpeRun rpe_run_stream(const rpe_handle *h, int pairs, RpeCamSrc cam = {nullptr, nullptr, 0}) { return rpe_run_rule(h, pairs, 1, cam); }
// P entries of the device pair table over the frame store
static inline RpeRun rpe_run_list(const rpe_handle *h, int P, RpeCamSrc cam = {nullptr, nullptr, 0})
{
    return {P, {h->fs.d_desc, h->fs.d_count, h->fs.d_kp_pt, h->fs.d_norm, (const int2 *)h->d_pairtab, 0}, cam};
}

// The links one call may carry, and the entries of link.links and of every per-link buffer
static inline int rpe_link_capacity(const rpe_handle *h) { return 4 * h->cfg.max_batch; }
// The link kernels' source: the table in link.links over the last run's buffers
static inline RpeLinkSrc rpe_link_src(const rpe_handle *h)
{
    return {h->link.links, h->d_m_q, h->d_m_t, h->d_m_n, h->d_status, h->d_mask, h->d_pose_mask, h->d_points, h->d_R, h->d_t,
            h->d_n1, h->d_n2, h->cfg.max_matches, h->lay.kcap};
}

// ---- kernel launchers (defined in the .hip files) --------------------------
void rpe_launch_pyramid(rpe_handle *h, int n_img, int l0, int l1);   // levels [max(l0, 1), l1) from the level below each, in order
// FAST over the tiles [t0, t0 + nt) of d_tiles_fast and the selection chain (raster + retain_fast, harris, retain_harris)
// over the levels [l0, l1), on `stream`: a level group of orb_groups.h or everything.  compact (rpe_launch_keypoints) reads
// every level.
void rpe_launch_fast(rpe_handle *h, int n_img, int t0, int nt, hipStream_t stream);
void rpe_launch_raster_retain(rpe_handle *h, int n_img, int l0, int l1, hipStream_t stream);
void rpe_launch_harris(rpe_handle *h, int n_img, int l0, int l1, hipStream_t stream);
void rpe_launch_retain_harris(rpe_handle *h, int n_img, int l0, int l1, hipStream_t stream);
void rpe_launch_keypoints(rpe_handle *h, int n_img);
void rpe_launch_orient_describe(rpe_handle *h, int n_img);
void rpe_launch_debug_blur(rpe_handle *h, int img);
// dynamic LDS of the retain kernels for a list of `cap` elements (kind 0: 4-byte FAST entries, 1: 8-byte Harris entries)
// and its [cap + 4] u16 stopper positions
constexpr size_t rpe_retain_lds(int kind, int cap) { return (kind ? sizeof(unsigned long long) : sizeof(unsigned)) * (size_t)cap + sizeof(unsigned short) * ((size_t)cap + 4); }
void rpe_launch_debug_retain(rpe_handle *h, int kind, int stl, void *d_elems, const int *d_len, const int *d_n_points, int *d_out_len, int n_lists, int cap);
// How the matrix-core Hamming matchers (crossCheck: extra_uint4 = 0, guided: RPE_GUIDED_LDS_UINT4) run B pairs of capacity
// kcap; the rule is rpe_hamming_plan's alone (match_kernels.hip)
struct RpeHammingPlan {
    int region0;                   // the tile kernel's first LDS region, in 16-byte units
    int sortP;                     // sort size: the power of two >= max(kcap, 64)
    int split;                     // workgroups per pair (gridDim.y of the tile kernel)
    bool hbm;                      // election words in d_hm_*: tile kernel + select kernel; false: the fused tile kernel alone
    size_t lds_tile, lds_select;   // dynamic LDS of the tile kernel (as launched) and of the select kernel
};
RpeHammingPlan rpe_hamming_plan(int kcap, int B, int extra_uint4);
void rpe_launch_match(rpe_handle *h, const RpeRun &r);
void rpe_launch_match_l2(rpe_handle *h, const RpeRun &r);
void rpe_launch_l2_norms(rpe_handle *h, int n_img);
void rpe_launch_guided(rpe_handle *h, const RpeRun &r, const double *d_R, const double *d_t, const int *d_status, double gate_px, int max_distance);
void rpe_launch_guided_l2(rpe_handle *h, const RpeRun &r, const double *d_R, const double *d_t, const int *d_status, double gate_px, double max_distance);
int rpe_sift_create(rpe_handle *h);
void rpe_sift_destroy(rpe_handle *h);
int rpe_sift_run(rpe_handle *h, const uint8_t *d_a, const uint8_t *d_b, int na, int nb);
int rpe_sift_fetch(rpe_handle *h, int n_images, float *fin_host, int *counts);
int rpe_sift_fetch_gauss(rpe_handle *h, int index, float *out);
long long rpe_sift_gauss_floats(rpe_handle *h);
void rpe_launch_ransac(rpe_handle *h, const RpeRun &r, bool want_mask);
void rpe_launch_pose(rpe_handle *h, const RpeRun &r, bool set_status);
void rpe_launch_structure(rpe_handle *h, const RpeRun &r);
void rpe_launch_refine(rpe_handle *h, const RpeRun &r, int max_iters, bool from_batch);
void rpe_launch_scale_links(rpe_handle *h, int L, int min_shared);
void rpe_launch_link_poses(rpe_handle *h, const RpeRun &r, int L, int iters, double threshold_px, int min_shared, int refine_iters);
bool rpe_link_poses_in_lds(const rpe_handle *h);
void rpe_launch_bundle_gather(rpe_handle *h, const RpeRun &r, int L, double threshold_px);
void rpe_launch_bundle(rpe_handle *h, int n, int min_shared, int max_iters, bool links);
bool rpe_bundles_in_lds(const rpe_handle *h);
void rpe_launch_tracks(rpe_handle *h, const RpeTrackJob &job);
void rpe_launch_track_points(rpe_handle *h, const RpeTrackPointJob &job);
void rpe_launch_windows(rpe_handle *h, const RpeWindowJob &job);
void rpe_launch_graphs(rpe_handle *h, const RpeGraphJob &job);
void rpe_launch_similar(rpe_handle *h, const RpeSimilarJob &job);
void rpe_launch_normalise(rpe_handle *h, const RpeRun &r);
void rpe_launch_homography(rpe_handle *h, const RpeRun &r, int iters, double threshold_px, bool from_batch);
void rpe_launch_undistort(rpe_handle *h, const float2 *d_pts, int n, const rpe_camera *d_cam, double2 *d_out);

// per-stage hipEvents on the handle's stream (rpe_set_profiling / rpe_get_stage_ms)
#define MARK(h, stage) do { if ((h)->profiling) hipEventRecord((h)->ev[stage], (h)->stream); } while (0)
