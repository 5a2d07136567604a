// track_point_kernels.hip -- track points (include/rpe_amd.h, "track points"): one scene point per track from all its
// views under absolute poses, every observation judged.  All f64, + - * / sqrt only, in the header's operation order.
//
// Two launches on the handle's stream:
//   tp_prepare   one thread per observation: the normalised (undistorted) point, the world bearing, the camera centre, the
//                focal scale and the frame's group into one 80-byte record.  The lens iteration is the expensive part of
//                an observation and is fully parallel here; cameras and poses are per frame and read through obs_frame
//   tp_solve     one thread per track, walking its CSR segment in ascending order: that IS the header's summation order, so
//                there is no reduction tree, no barrier and no atomic.  The per-observation state of a track of any length
//                (its verdict) lives in the obs_flag output itself, which the thread reads back in the reselection round
// A view (bm_view) and the rule of the refinement (lm_loop, here for one thread) are bundle_math.h's, as in the link kernels
#include "geom_device.h"

struct alignas(16) TpObs { double x, y, d[3], c[3], f; int group, frame; };
static_assert(sizeof(TpObs) == RPE_TRACK_POINT_OBS_BYTES, "five 16-byte loads per observation");

struct TpArgs {
    RpeTrackPointJob job;
    TpObs *obs;                    // [n_obs]
    double *points, *rms, *min_cos, *obs_err;
    int *info;
    uint8_t *obs_flag;
};

__global__ __launch_bounds__(256) void tp_prepare_kernel(const TpArgs a)
{
    const int o = tk_thread_index(a.job.scene.n_obs);
    if (o < 0) return;
    const RpeTrackPointJob &j = a.job;
    const int fr = j.scene.obs_frame[o];
    const rpe_camera *cam = j.scene.cams + (size_t)fr * j.scene.cam_stride;
    const double2 n = rpe_camera_normalise(cam, rpe_camera_has_lens(cam), j.scene.obs_xy[o]);
    const double *R = j.scene.R + (size_t)fr * 9, *T = j.scene.T + (size_t)fr * 3;
    TpObs ob;
    ob.x = n.x; ob.y = n.y;
    double v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = (R[k] * n.x + R[3 + k] * n.y) + R[6 + k];
        ob.c[k] = -((R[k] * T[0] + R[3 + k] * T[1]) + R[6 + k] * T[2]);
    }
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) ob.d[k] = v[k] / len;
    ob.f = (cam->fx + cam->fy) / 2;
    ob.group = j.group ? j.group[fr] : 0;
    ob.frame = fr;
    a.obs[o] = ob;
}

// One view of X (bm_view): depth y2 (the return value says y2 > 0), the projection (u, w) and the pixel residual (e0, e1)
struct TpView { double y2, u, w, e0, e1; };
__device__ __forceinline__ bool tp_view(const TpObs &ob, const double *__restrict__ R, const double *__restrict__ T,
                                        const double (&X)[3], TpView &v)
{
    double yu[3];
    bm_view<false>(R, T, ob.f, X, ob.x, ob.y, v.e0, v.e1, nullptr, nullptr, yu);
    v.y2 = yu[0]; v.u = yu[1]; v.w = yu[2];
    return v.y2 > 0.;
}

// The selection of a round: the used set (group G) in the first, the inliers of its classification in the second
__device__ __forceinline__ bool tp_selected(const TpArgs &a, int o, const TpObs &ob, int G, bool inliers)
{
    return inliers ? a.obs_flag[o] == 1 : ob.group == G;
}

// Cost and normal equations of X over the selection; false when a selected view has no positive depth (H, g, cost are
// then not to be used)
__device__ __forceinline__ bool tp_linearise(const TpArgs &a, int s, int e, int G, bool inliers, const double (&X)[3],
                                             double &cost, double (&H)[6], double (&g)[3])
{
    bool front = true;
    cost = 0.;
#pragma unroll
    for (int k = 0; k < 6; ++k) H[k] = 0.;
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = 0.;
    for (int o = s; o < e; ++o) {
        const TpObs ob = a.obs[o];
        if (!tp_selected(a, o, ob, G, inliers)) continue;
        const double *R = a.job.scene.R + (size_t)ob.frame * 9;
        TpView v;
        front = tp_view(ob, R, a.job.scene.T + (size_t)ob.frame * 3, X, v) && front;
        cost = cost + (v.e0 * v.e0 + v.e1 * v.e1);
        const double q = ob.f / v.y2, qa = q * v.u, qb = q * v.w;
        double J0[3], J1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { J0[k] = q * R[k] - qa * R[6 + k]; J1[k] = q * R[3 + k] - qb * R[6 + k]; }
        int n = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = i; k < 3; ++k, ++n) H[n] = H[n] + (J0[i] * J0[k] + J1[i] * J1[k]);
            g[i] = g[i] + (J0[i] * v.e0 + J1[i] * v.e1);
        }
    }
    return front;
}

__global__ __launch_bounds__(256) void tp_solve_kernel(const TpArgs a)
{
    const int t = tk_thread_index(a.job.scene.n_tracks);
    if (t < 0) return;
    const RpeTrackPointJob &j = a.job;
    const int s = j.scene.track_start[t], e = j.scene.track_start[t + 1];
    // 1: the group and the used set; the flags double as this thread's per-observation state, so they start at zero
    int G = -1, nU = 0;
    for (int o = s; o < e; ++o) {
        const int g = a.obs[o].group;
        if (G < 0 && g >= 0) G = g;
        nU += G >= 0 && g == G;
        a.obs_flag[o] = 0; a.obs_err[o] = 0.;
    }
    int code = -1, nin = 0, iters = 0, acc = 0;             // acc: lm_loop counts the accepted steps, nothing here reads them
    double X[3] = {0., 0., 0.}, rms = 0., mc = 0.;
    if (nU < j.min_views) code = RPE_TRACKPT_TOO_FEW;
    for (int round = 0; code < 0; ++round) {
        const bool inl = round == 1;
        // 2: the midpoint of the selected rays
        double A[6] = {0., 0., 0., 0., 0., 0.}, b[3] = {0., 0., 0.};
        for (int o = s; o < e; ++o) {
            const TpObs ob = a.obs[o];
            if (!tp_selected(a, o, ob, G, inl)) continue;
            int n = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double m[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = (i == k ? 1. : 0.) - ob.d[i] * ob.d[k];
#pragma unroll
                for (int k = i; k < 3; ++k, ++n) A[n] = A[n] + m[k];
                b[i] = b[i] + ((m[0] * ob.c[0] + m[1] * ob.c[1]) + m[2] * ob.c[2]);
            }
        }
        const double nb[3] = {-b[0], -b[1], -b[2]};
        if (!refine_solve<3>(A, nb, 0., X)) { code = RPE_TRACKPT_DEGENERATE; break; }
        double cost, H[6], g[3];
        if (!tp_linearise(a, s, e, G, inl, X, cost, H, g)) { code = RPE_TRACKPT_BEHIND; break; }
        // 3: lm_loop for one thread.  A trial is linearised as it is costed, so an accepted one needs no second pass; a trial
        // with a selected view behind is vetoed
        double d[3], Xn[3], Hn[6], gn[3];
        auto trial = [&](double) {
            double c1;
            Xn[0] = X[0] + d[0]; Xn[1] = X[1] + d[1]; Xn[2] = X[2] + d[2];
            return tp_linearise(a, s, e, G, inl, Xn, c1, Hn, gn) ? c1 : (double)INFINITY;
        };
        auto accept = [&]() {
#pragma unroll
            for (int k = 0; k < 3; ++k) { X[k] = Xn[k]; g[k] = gn[k]; }
#pragma unroll
            for (int k = 0; k < 6; ++k) H[k] = Hn[k];
        };
        auto step = [&](double lambda) { return refine_solve<3>(H, g, lambda, d); };
        lm_loop(cost, j.max_iters, step, trial, [&]() { return lm_step_norm(d, 3); }, accept, iters, acc);
        // 4: every used view judged at X
        double ss = 0.;
        nin = 0;
        for (int o = s; o < e; ++o) {
            const TpObs ob = a.obs[o];
            if (ob.group != G) continue;
            TpView v;
            double err = -1.;
            bool in = false;
            if (tp_view(ob, j.scene.R + (size_t)ob.frame * 9, j.scene.T + (size_t)ob.frame * 3, X, v)) {
                const double e2 = v.e0 * v.e0 + v.e1 * v.e1;
                err = sqrt(e2);
                in = err <= j.threshold_px;
                if (in) { ss = ss + e2; ++nin; }
            }
            a.obs_flag[o] = in ? 1 : 2; a.obs_err[o] = err;
        }
        rms = nin > 0 ? sqrt(ss / (double)nin) : 0.;
        if (nin == nU || round == 1 || nin < j.min_views) {
            if (nin < j.min_views) code = RPE_TRACKPT_OUTLIERS;
            break;
        }
    }
    if (code < 0) {
        // 5: parallax over the inlier views
        bool first = true;
        double r1[3] = {0., 0., 0.}, n1 = 0.;
        mc = 1.;
        for (int o = s; o < e; ++o) {
            if (a.obs_flag[o] != 1) continue;
            const TpObs ob = a.obs[o];
            const double r[3] = {ob.c[0] - X[0], ob.c[1] - X[1], ob.c[2] - X[2]};
            const double nr = sqrt(hg_dot(r, r));
            if (first) { r1[0] = r[0]; r1[1] = r[1]; r1[2] = r[2]; n1 = nr; first = false; continue; }
            const double c = hg_dot(r1, r) / (n1 * nr);
            if (c < mc) mc = c;
        }
        code = mc > j.max_cos ? RPE_TRACKPT_LOW_PARALLAX : RPE_TRACKPT_OK;
    } else if (code == RPE_TRACKPT_DEGENERATE || code == RPE_TRACKPT_BEHIND) {
        // found in either round: what the first round's classification wrote is withdrawn
        const bool behind = code == RPE_TRACKPT_BEHIND;
        for (int o = s; o < e; ++o) {
            a.obs_flag[o] = behind && a.obs[o].group == G ? 2 : 0;
            a.obs_err[o] = 0.;
        }
        nin = 0; rms = 0.;
        if (!behind) { X[0] = 0.; X[1] = 0.; X[2] = 0.; }
    }
    a.points[(size_t)t * 3] = X[0]; a.points[(size_t)t * 3 + 1] = X[1]; a.points[(size_t)t * 3 + 2] = X[2];
    a.info[(size_t)t * 4] = code; a.info[(size_t)t * 4 + 1] = nU; a.info[(size_t)t * 4 + 2] = nin; a.info[(size_t)t * 4 + 3] = iters;
    a.rms[t] = rms; a.min_cos[t] = mc;
}

// The two launches of one job.  The buffers are the caller's business (rpe_triangulate_tracks, rpe_features.hip)
void rpe_launch_track_points(rpe_handle *h, const RpeTrackPointJob &job)
{
    TpArgs a{};
    a.job = job;
    a.obs = (TpObs *)h->tp.obs;
    a.points = h->tp.points; a.rms = h->tp.rms; a.min_cos = h->tp.mincos; a.obs_err = h->tp.oerr;
    a.info = h->tp.info; a.obs_flag = h->tp.oflag;
    const dim3 blk(256);
    if (job.scene.n_obs > 0) hipLaunchKernelGGL(tp_prepare_kernel, dim3((unsigned)(((long long)job.scene.n_obs + 255) / 256)), blk, 0, h->stream, a);
    hipLaunchKernelGGL(tp_solve_kernel, dim3((unsigned)(((long long)job.scene.n_tracks + 255) / 256)), blk, 0, h->stream, a);
}
