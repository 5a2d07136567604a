// window_kernels.hip -- window bundles (include/rpe_amd.h, "window bundles"): the poses of a window of 2 .. 8 frames and the
// points of the tracks they see, refined together on one reprojection cost.  All f64, + - * / sqrt only (sin for a rotation
// increment), in the header's operation order.
//
// Three launches on the handle's stream:
//   wb_prepare   one thread per observation: the normalised (undistorted) point and the focal scale, one 32-byte record
//   wb_gather    one workgroup per window: the candidates in track order by ordered_slot (no atomic decides an order), per
//                kept point its track and the observation of each window position (8 ints, -1 where there is none), per
//                position the number of observations (integer LDS atomics: a count, not an order)
//   wb_solve     one workgroup per window: the gauge, the codes, the Levenberg-Marquardt loop, the outputs.  The cameras
//                live in LDS, the points' state (X and the trial X, 48 B per point) in device memory.  A step at one
//                damping is
//                  pair passes  every pair (p <= q) of free positions is one pass of ONE wave over the points both see
//                               (lane stride 64, the point's blocks recomputed from the state): 36 sums of Y_p W_q' and, on
//                               p == q, the 21 of U_p, g_c, v and the count of singular V; the pairs are dealt to the four
//                               waves round robin, so there is no barrier between passes and nothing per point is stored
//                  reduce       the (6 W - 7)-square system and its right-hand side in LDS, a Cholesky by columns: every
//                               thread forms the pivot, thread i the entry of row i, each inner sum serially in ascending
//                               k, so it equals the scalar Cholesky of bm_chol (bundle_math.h) bit for bit; the right-hand
//                               side rides along as one more row (the forward substitution), thread 0 substitutes back;
//                               one barrier per column
//                  trial        per point (lane stride 256) dp = -V^-1 (g_p + W' step), the trial X and its cost
// A point's Jacobians are formed again in every pass: arithmetic is small next to storing 288 B per observation.
// A view with its rows, the point block with its inverse and the rule of the loop are bundle_math.h's, as in the link kernels.
#include "geom_device.h"

#define WB_V RPE_WINDOW_MAX_VIEWS
static_assert(WB_V == RPE_WINDOW_SLOT_OBS, "wb.pobs holds one observation per window position and point slot");
#define WB_NS (6 * WB_V - 7)                   // most camera parameters: 41
#define WB_PAIRS ((WB_V - 1) * WB_V / 2)       // most pairs (p <= q) of free positions: 28

struct alignas(16) WbObs { double x, y, f, pad; };
static_assert(sizeof(WbObs) == RPE_WINDOW_OBS_BYTES, "wb.obs holds one record per observation");

struct WbArgs {
    RpeWindowJob job;
    WbObs *obs;                    // [n_obs]
    int *ptrack, *pobs;            // [n_win * max_points], [n_win * max_points * 8]
    int *fcnt;                     // [n_win * 8]
    int *counts, *info;            // [n_win * 4] each
    double *state;                 // [n_win * max_points * 6]: X, then the trial X
    double *points;                // [n_win * max_points * 3]
    double *Rout, *Tout, *rms;
};

__global__ __launch_bounds__(256) void wb_prepare_kernel(const WbArgs a)
{
    const int o = tk_thread_index(a.job.scene.n_obs);
    if (o < 0) return;
    const RpeWindowJob &j = a.job;
    const rpe_camera *cam = j.scene.cams + (size_t)j.scene.obs_frame[o] * j.scene.cam_stride;
    const double2 n = rpe_camera_normalise(cam, rpe_camera_has_lens(cam), j.scene.obs_xy[o]);
    WbObs ob;
    ob.x = n.x; ob.y = n.y; ob.f = (cam->fx + cam->fy) / 2; ob.pad = 0.;
    a.obs[o] = ob;
}

__global__ __launch_bounds__(256) void wb_gather_kernel(const WbArgs a)
{
    __shared__ int s_fr[WB_V], s_cnt[WB_V], s_wc[4];
    const int w = blockIdx.x, tid = threadIdx.x;
    const RpeWindowJob &j = a.job;
    const int ws = j.win_start[w], W = j.win_start[w + 1] - ws;
    if (tid < WB_V) { s_fr[tid] = tid < W ? j.win_frame[ws + tid] : -1; s_cnt[tid] = 0; }
    __syncthreads();
    const size_t pm = (size_t)w * j.max_points;
    int n = 0;                                                               // candidates so far
    for (int t0 = 0; t0 < j.scene.n_tracks; t0 += 256) {
        const int t = t0 + tid;
        unsigned seen = 0;
        int s = 0, e = 0;
        if (t < j.scene.n_tracks && (!j.point_use || j.point_use[t])) {
            s = j.scene.track_start[t]; e = j.scene.track_start[t + 1];
            for (int o = s; o < e; ++o) {
                if (j.obs_use && j.obs_use[o] != 1) continue;
                const int fr = j.scene.obs_frame[o];
                for (int p = 0; p < W; ++p) if (s_fr[p] == fr) seen |= 1u << p;
            }
        }
        const bool cand = __popc(seen) >= 2;
        const int slot = ordered_slot(cand, s_wc, n);
        if (cand && slot < j.max_points) {
            a.ptrack[pm + slot] = t;
            int *po = a.pobs + (pm + slot) * WB_V;
#pragma unroll
            for (int p = 0; p < WB_V; ++p) po[p] = -1;
            unsigned done = 0;                                               // the lowest observation of a position wins
            for (int o = s; o < e; ++o) {
                if (j.obs_use && j.obs_use[o] != 1) continue;
                const int fr = j.scene.obs_frame[o];
                for (int p = 0; p < W; ++p)
                    if (s_fr[p] == fr && !((done >> p) & 1u)) { po[p] = o; done |= 1u << p; }
            }
            for (int p = 0; p < W; ++p) if ((seen >> p) & 1u) atomicAdd(&s_cnt[p], 1);
        }
    }
    __syncthreads();
    const int kept = min(n, j.max_points);
    for (int i = kept + tid; i < j.max_points; i += 256) a.ptrack[pm + i] = -1;
    if (tid < WB_V) a.fcnt[w * WB_V + tid] = s_cnt[tid];
    if (tid == 0) {
        int no = 0;
        for (int p = 0; p < W; ++p) no += s_cnt[p];
        a.counts[w * 4] = W; a.counts[w * 4 + 1] = kept; a.counts[w * 4 + 2] = no; a.counts[w * 4 + 3] = n - kept;
    }
}

// The two residuals of one view of X in pixels; with JAC the rows' derivatives by (w0 w1 w2 | d0 d1 d2) and by the point
// (bm_view, bm_point_rows).  Position 0 comes through here as (I, 0): a = X and Jt Q = Jt to the bit
template <bool JAC>
__device__ __forceinline__ void wb_view(const double *Q, const double *t, const WbObs &ob, const double *X, double (&e)[2],
                                        double (&Jx)[6], double (&Jy)[6], double (&JX)[2][3])
{
    bm_view<JAC>(Q, t, ob.f, X, ob.x, ob.y, e[0], e[1], Jx, Jy);
    if (JAC) bm_point_rows(Jx, Jy, Q, JX[0], JX[1]);
}

// the anchor's block: (w | tangent step); its sixth column is unused and zero
__device__ __forceinline__ void wb_anchor_cols(const double *b, double (&J)[6])
{
    const double c3 = (J[3] * b[0] + J[4] * b[1]) + J[5] * b[2], c4 = (J[3] * b[3] + J[4] * b[4]) + J[5] * b[5];
    J[3] = c3; J[4] = c4; J[5] = 0.;
}

// What a pass over the points reads: the window's size, the cameras (LDS), the tangent basis at the anchor's t (LDS), the
// observation records, a point's observation per position and the points' coordinates
struct WbState {
    int W, A;
    const double *Q, *t, *b;
    const WbObs *obs;
    const int *pobs;
    const double *X;
};

// The point block of point j under damping lambda: Vi = (Jp'Jp + lambda diag)^-1 by the adjugate and g_p = Jp'e, over the
// point's views in ascending position, x row before y row (bm_block_row).  False when V is singular.
__device__ __forceinline__ bool wb_block(const WbState &c, int j, double lambda, double (&Vi)[6], double (&gp)[3])
{
    double v[6] = {0., 0., 0., 0., 0., 0.};
    gp[0] = 0.; gp[1] = 0.; gp[2] = 0.;
    const int *po = c.pobs + (size_t)j * WB_V;
    const double *X = c.X + 3 * (size_t)j;
    for (int p = 0; p < c.W; ++p) {
        const int o = po[p];
        if (o < 0) continue;
        double e[2], Jx[6], Jy[6], JX[2][3];
        wb_view<true>(c.Q + 9 * p, c.t + 3 * p, c.obs[o], X, e, Jx, Jy, JX);
        bm_block_row(JX[0], e[0], v, gp);
        bm_block_row(JX[1], e[1], v, gp);
    }
    return bm_damped_inverse(v, lambda, Vi);
}

// The view of point j at position p >= 1 (observation o): its residuals, the rows by the block's parameters and W = Jc'Jp
__device__ __forceinline__ void wb_cam_view(const WbState &c, int j, int p, int o, double (&e)[2], double (&Jx)[6], double (&Jy)[6],
                                            double (&Wm)[6][3])
{
    double JX[2][3];
    wb_view<true>(c.Q + 9 * p, c.t + 3 * p, c.obs[o], c.X + 3 * (size_t)j, e, Jx, Jy, JX);
    if (p == c.A) { wb_anchor_cols(c.b, Jx); wb_anchor_cols(c.b, Jy); }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) Wm[k][i] = Jx[k] * JX[0][i] + Jy[k] * JX[1][i];
}

__device__ __forceinline__ int wb_tri6(int k, int m) { return k * 6 - k * (k - 1) / 2 + (m - k); }   // k <= m < 6

__global__ __launch_bounds__(256) void wb_solve_kernel(const WbArgs a)
{
    __shared__ double s_Q[WB_V * 9], s_t[WB_V * 3], s_Qn[WB_V * 9], s_tn[WB_V * 3], s_b[6], s_n2[WB_V];
    __shared__ double s_S[WB_NS * WB_NS], s_H[(WB_NS + 1) * WB_NS], s_U[WB_V * 21], s_gc[WB_NS], s_v[WB_NS], s_d[WB_NS], s_diag[WB_NS];
    __shared__ double s_red[4], s_bad[WB_PAIRS];
    __shared__ int s_off[WB_V], s_cam[WB_NS], s_k[WB_NS], s_pair[WB_PAIRS], s_fr[WB_V];
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const RpeWindowJob &jb = a.job;
    const int ws = jb.win_start[w], W = jb.win_start[w + 1] - ws;
    const int n = a.counts[w * 4 + 1], nobs = a.counts[w * 4 + 2];
    const size_t pm = (size_t)w * jb.max_points;
    const int *ptrack = a.ptrack + pm, *pobs = a.pobs + pm * WB_V;
    double *sX = a.state + pm * RPE_WINDOW_STATE_DOUBLES, *sXn = sX + 3 * (size_t)jb.max_points;
    double *pts = a.points + pm * 3;
    // ---- the gauge: every position relative to position 0
    if (tid < WB_V) s_fr[tid] = tid < W ? jb.win_frame[ws + tid] : 0;
    __syncthreads();
    const double *R0 = jb.scene.R + (size_t)s_fr[0] * 9, *T0 = jb.scene.T + (size_t)s_fr[0] * 3;
    if (tid < W) {
        const int p = tid;
        if (p == 0) {
#pragma unroll
            for (int e = 0; e < 9; ++e) { s_Q[e] = (e % 4 == 0) ? 1. : 0.; s_Qn[e] = s_Q[e]; }
#pragma unroll
            for (int e = 0; e < 3; ++e) { s_t[e] = 0.; s_tn[e] = 0.; }
            s_n2[0] = 0.;
        } else {
            const double *Rp = jb.scene.R + (size_t)s_fr[p] * 9, *Tp = jb.scene.T + (size_t)s_fr[p] * 3;
            double Q[9], s[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Q[r * 3 + c] = (Rp[r * 3] * R0[c * 3] + Rp[r * 3 + 1] * R0[c * 3 + 1]) + Rp[r * 3 + 2] * R0[c * 3 + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) s[r] = Tp[r] - ((Q[r * 3] * T0[0] + Q[r * 3 + 1] * T0[1]) + Q[r * 3 + 2] * T0[2]);
#pragma unroll
            for (int e = 0; e < 9; ++e) s_Q[p * 9 + e] = Q[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) s_t[p * 3 + e] = s[e];
            s_n2[p] = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
        }
    }
    __syncthreads();
    int A = 1;
    double best = s_n2[1];
    for (int p = 2; p < W; ++p) if (s_n2[p] > best) { A = p; best = s_n2[p]; }
    const double l = sqrt(best);
    int code = -1;
    if (!(l > 0.) || !hg_finite(l)) code = RPE_WINDOW_NO_BASELINE;
    if (code < 0) {
        const int need = max(jb.min_obs, 6);
        for (int p = 1; p < W; ++p) if (a.fcnt[w * WB_V + p] < need) code = RPE_WINDOW_TOO_FEW;
    }
    // the input state as the output: poses and points, zeros past the points
    auto return_input = [&]() {
        if (tid < W) {
            const double *Rp = jb.scene.R + (size_t)s_fr[tid] * 9, *Tp = jb.scene.T + (size_t)s_fr[tid] * 3;
#pragma unroll
            for (int e = 0; e < 9; ++e) a.Rout[(size_t)(ws + tid) * 9 + e] = Rp[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) a.Tout[(size_t)(ws + tid) * 3 + e] = Tp[e];
        }
        for (int j = tid; j < jb.max_points; j += 256) {
            const double *P = jb.points0 + 3 * (size_t)(j < n ? ptrack[j] : 0);
#pragma unroll
            for (int e = 0; e < 3; ++e) pts[3 * (size_t)j + e] = j < n ? P[e] : 0.;
        }
    };
    if (code >= 0) {                                                         // workgroup-uniform
        return_input();
        if (tid == 0) {
            a.info[w * 4] = code; a.info[w * 4 + 1] = 0; a.info[w * 4 + 2] = 0; a.info[w * 4 + 3] = A;
            a.rms[w * 2] = 0.; a.rms[w * 2 + 1] = 0.;
        }
        return;
    }
    // ---- the scaled problem: translations and points over l; the parameter tables
    const int N = 6 * W - 7, npairs = (W - 1) * W / 2;
    if (tid >= 1 && tid < W) {
#pragma unroll
        for (int e = 0; e < 3; ++e) s_t[tid * 3 + e] = s_t[tid * 3 + e] / l;
    }
    if (tid == 0) {
        int off = 0, pr = 0;
        for (int p = 1; p < W; ++p) {
            s_off[p] = off;
            const int np = p == A ? 5 : 6;
            for (int k = 0; k < np; ++k) { s_cam[off + k] = p; s_k[off + k] = k; }
            off += np;
            for (int q = p; q < W; ++q) s_pair[pr++] = p | (q << 4);
        }
        s_off[0] = 0;
    }
    for (int j = tid; j < n; j += 256) {
        const double *P = jb.points0 + 3 * (size_t)ptrack[j];
#pragma unroll
        for (int r = 0; r < 3; ++r) sX[3 * (size_t)j + r] = (((R0[r * 3] * P[0] + R0[r * 3 + 1] * P[1]) + R0[r * 3 + 2] * P[2]) + T0[r]) / l;
    }
    __syncthreads();
    auto basis = [&]() {                                                     // the tangent basis at the anchor's t
        if (tid == 0) refine_basis(s_t + 3 * A, s_b, s_b + 3);
        __syncthreads();
    };
    basis();
    WbState st{W, A, s_Q, s_t, s_b, a.obs, pobs, sX};
    // the cost of the points Xs under the cameras (Q, t): lane partials in strided order, butterfly, wave totals
    auto cost_of = [&](const double *Q, const double *t, const double *Xs) {
        double c[1] = {0.};
        for (int j = tid; j < n; j += 256) {
            const int *po = pobs + (size_t)j * WB_V;
            double pc = 0.;
            for (int p = 0; p < W; ++p) {
                const int o = po[p];
                if (o < 0) continue;
                double e[2], Jx[6], Jy[6], JX[2][3];
                wb_view<false>(Q + 9 * p, t + 3 * p, a.obs[o], Xs + 3 * (size_t)j, e, Jx, Jy, JX);
                pc = pc + (e[0] * e[0] + e[1] * e[1]);
            }
            c[0] += pc;
        }
        block_sum_f64<1>(c, s_red, tid);
        return c[0];
    };
    // the step at damping lambda into s_d; false when a V is singular or the reduced system is not positive definite
    auto solve = [&](double lambda) {
        for (int pr = wv; pr < npairs; pr += 4) {                            // wave-uniform: no barrier inside
            const int p = s_pair[pr] & 15, q = s_pair[pr] >> 4;
            const bool diag = p == q;
            double S[36], U[21], vv[6], gc[6], bad = 0.;
#pragma unroll
            for (int k = 0; k < 36; ++k) S[k] = 0.;
#pragma unroll
            for (int k = 0; k < 21; ++k) U[k] = 0.;
#pragma unroll
            for (int k = 0; k < 6; ++k) { vv[k] = 0.; gc[k] = 0.; }
            for (int j = lane; j < n; j += 64) {
                const int *po = pobs + (size_t)j * WB_V;
                const int op = po[p], oq = po[q];
                if (op < 0 || oq < 0) continue;
                double Vi[6], gp[3];
                if (!wb_block(st, j, lambda, Vi, gp)) { bad += 1.; continue; }
                double e[2], Jx[6], Jy[6], Wp[6][3], Wq[6][3];
                wb_cam_view(st, j, p, op, e, Jx, Jy, Wp);
                if (diag) {
                    int i = 0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
#pragma unroll
                        for (int m = k; m < 6; ++m, ++i) U[i] += Jx[k] * Jx[m] + Jy[k] * Jy[m];
                        gc[k] += Jx[k] * e[0] + Jy[k] * e[1];
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k)
#pragma unroll
                        for (int i2 = 0; i2 < 3; ++i2) Wq[k][i2] = Wp[k][i2];
                } else {
                    double eq[2], Jxq[6], Jyq[6];
                    wb_cam_view(st, j, q, oq, eq, Jxq, Jyq, Wq);
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double Y[3] = {bm_sym_row(Vi, 0, Wp[k]), bm_sym_row(Vi, 1, Wp[k]), bm_sym_row(Vi, 2, Wp[k])};
#pragma unroll
                    for (int m = 0; m < 6; ++m) S[k * 6 + m] += (Y[0] * Wq[m][0] + Y[1] * Wq[m][1]) + Y[2] * Wq[m][2];
                    if (diag) vv[k] += (Y[0] * gp[0] + Y[1] * gp[1]) + Y[2] * gp[2];
                }
            }
#pragma unroll
            for (int k = 0; k < 36; ++k) S[k] = wave_sum_f64(S[k]);
            bad = wave_sum_f64(bad);
            if (diag) {
#pragma unroll
                for (int k = 0; k < 21; ++k) U[k] = wave_sum_f64(U[k]);
#pragma unroll
                for (int k = 0; k < 6; ++k) { vv[k] = wave_sum_f64(vv[k]); gc[k] = wave_sum_f64(gc[k]); }
            }
            if (lane == 0) {
                const int np = p == A ? 5 : 6, nq = q == A ? 5 : 6, op0 = s_off[p], oq0 = s_off[q];
#pragma unroll
                for (int k = 0; k < 6; ++k)
#pragma unroll
                    for (int m = 0; m < 6; ++m)
                        if (k < np && m < nq && (!diag || k <= m)) s_S[(op0 + k) * WB_NS + oq0 + m] = S[k * 6 + m];
                if (diag) {
#pragma unroll
                    for (int k = 0; k < 21; ++k) s_U[p * 21 + k] = U[k];
#pragma unroll
                    for (int k = 0; k < 6; ++k) if (k < np) { s_gc[op0 + k] = gc[k]; s_v[op0 + k] = vv[k]; }
                }
                s_bad[pr] = bad;
            }
        }
        __syncthreads();
        bool singular = false;
        for (int pr = 0; pr < npairs; ++pr) singular = singular || s_bad[pr] != 0.;
        if (singular) { __syncthreads(); return false; }
        // H = (U + lambda diag U) - S, both triangles; row N: -(g_c - v)
        for (int i = tid; i < N * N; i += 256) {
            const int r = i / N, c = i - r * N;
            if (r > c) continue;
            double u = 0.;                                                   // no residual sees two cameras
            if (s_cam[r] == s_cam[c]) u = s_U[s_cam[r] * 21 + wb_tri6(s_k[r], s_k[c])];
            if (r == c) u = u + lambda * u;
            const double hv = u - s_S[r * WB_NS + c];
            s_H[r * WB_NS + c] = hv; s_H[c * WB_NS + r] = hv;
        }
        if (tid < N) s_H[N * WB_NS + tid] = -(s_gc[tid] - s_v[tid]);
        __syncthreads();
        // Cholesky by columns; row N is the right-hand side, so its entries are the forward substitution
        bool ok = true;
        for (int c = 0; c < N; ++c) {
            double s = s_H[c * WB_NS + c];
            for (int k = 0; k < c; ++k) s -= s_H[c * WB_NS + k] * s_H[c * WB_NS + k];
            if (!(s > 0.) || !hg_finite(s)) { ok = false; break; }           // identical operands on every thread
            const double dj = sqrt(s);
            const int r = c + 1 + tid;
            double v = 0.;
            if (r <= N) {
                v = s_H[r * WB_NS + c];
                for (int k = 0; k < c; ++k) v -= s_H[r * WB_NS + k] * s_H[c * WB_NS + k];
                v = v / dj;
            }
            // column c of rows below c is read by its own writer only in this step, and the pivot goes to s_diag, not onto the
            // diagonal every thread has just read: one barrier per column, behind the writes
            if (r <= N) s_H[r * WB_NS + c] = v;
            if (tid == 0) s_diag[c] = dj;
            __syncthreads();
        }
        if (ok && tid == 0) {
            for (int i = N - 1; i >= 0; --i) {
                double v = s_H[N * WB_NS + i];
                for (int k = i + 1; k < N; ++k) v -= s_H[k * WB_NS + i] * s_d[k];
                s_d[i] = v / s_diag[i];
            }
        }
        __syncthreads();
        return ok;
    };
    // the trial state of step s_d at damping lambda: cameras into (s_Qn, s_tn), points into sXn; returns its cost
    auto trial = [&](double lambda) {
        if (tid >= 1 && tid < W) {
            const int p = tid, off = s_off[p];
            double d[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] = (k < 5 || p != A) ? s_d[off + k] : 0.;
            refine_rotate(d, s_Q + 9 * p, s_Qn + 9 * p);
            if (p == A) {
                double tn[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) tn[e] = (s_t[3 * p + e] + d[3] * s_b[e]) + d[4] * s_b[3 + e];
                const double nt = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
#pragma unroll
                for (int e = 0; e < 3; ++e) s_tn[3 * p + e] = tn[e] / nt;
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e) s_tn[3 * p + e] = s_t[3 * p + e] + d[3 + e];
            }
        }
        for (int j = tid; j < n; j += 256) {
            double Vi[6], gp[3];
            wb_block(st, j, lambda, Vi, gp);
            double u[3] = {gp[0], gp[1], gp[2]};
            const int *po = pobs + (size_t)j * WB_V;
            for (int p = 1; p < W; ++p) {
                const int o = po[p];
                if (o < 0) continue;
                double e[2], Jx[6], Jy[6], Wm[6][3];
                wb_cam_view(st, j, p, o, e, Jx, Jy, Wm);
                const int off = s_off[p], np = p == A ? 5 : 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (k < np) {
                        const double dk = s_d[off + k];
#pragma unroll
                        for (int i = 0; i < 3; ++i) u[i] += Wm[k][i] * dk;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) sXn[3 * (size_t)j + i] = sX[3 * (size_t)j + i] - bm_sym_row(Vi, i, u);
        }
        __syncthreads();                                                     // the trial cameras; a thread reads its own trial points
        return cost_of(s_Qn, s_tn, sXn);
    };
    // ---- lm_loop over this state
    const double cost0 = cost_of(s_Q, s_t, sX);
    double cost = cost0;
    int iters = 0, acc = 0;
    auto accept = [&]() {
        __syncthreads();                                                     // every reader of the old state and of s_d is done
        if (tid < W * 9) s_Q[tid] = s_Qn[tid];
        if (tid < W * 3) s_t[tid] = s_tn[tid];
        for (int j = tid; j < n; j += 256) {
#pragma unroll
            for (int e = 0; e < 3; ++e) sX[3 * (size_t)j + e] = sXn[3 * (size_t)j + e];
        }
        __syncthreads();                                                     // the passes of solve() walk the points in another order
        basis();
    };
    if (hg_finite(cost0)) lm_loop(cost, jb.max_iters, solve, trial, [&]() { return lm_step_norm(s_d, N); }, accept, iters, acc);
    // ---- the bundled state is returned only if a step was accepted, it is finite and every point lies in front of its views
    double bad[1] = {0.};
    if (acc > 0) {
        for (int e = tid; e < W * 12; e += 256) {
            const double v = e < W * 9 ? s_Q[e] : s_t[e - W * 9];
            if (!hg_finite(v)) bad[0] += 1.;
        }
        for (int j = tid; j < n; j += 256) {
            const double *X = sX + 3 * (size_t)j;
            const int *po = pobs + (size_t)j * WB_V;
            bool ok = hg_finite(X[0]) && hg_finite(X[1]) && hg_finite(X[2]);
            for (int p = 0; p < W; ++p) {
                if (po[p] < 0) continue;
                const double *Q = s_Q + 9 * p;
                const double z = ((Q[6] * X[0] + Q[7] * X[1]) + Q[8] * X[2]) + s_t[3 * p + 2];
                ok = ok && z > 0.;
            }
            if (!ok) bad[0] += 1.;
        }
        block_sum_f64<1>(bad, s_red, tid);
    }
    const bool take = acc > 0 && bad[0] == 0.;
    if (take) {
        if (tid < W) {
            const int p = tid;
            double *Ro = a.Rout + (size_t)(ws + p) * 9, *To = a.Tout + (size_t)(ws + p) * 3;
            if (p == 0) {
#pragma unroll
                for (int e = 0; e < 9; ++e) Ro[e] = R0[e];
#pragma unroll
                for (int e = 0; e < 3; ++e) To[e] = T0[e];
            } else {
                const double *Q = s_Q + 9 * p;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) Ro[r * 3 + c] = (Q[r * 3] * R0[c] + Q[r * 3 + 1] * R0[3 + c]) + Q[r * 3 + 2] * R0[6 + c];
                    To[r] = l * s_t[3 * p + r] + ((Q[r * 3] * T0[0] + Q[r * 3 + 1] * T0[1]) + Q[r * 3 + 2] * T0[2]);
                }
            }
        }
        for (int j = tid; j < jb.max_points; j += 256) {
            double o[3] = {0., 0., 0.};
            if (j < n) {
                const double *X = sX + 3 * (size_t)j;
                const double m[3] = {l * X[0] - T0[0], l * X[1] - T0[1], l * X[2] - T0[2]};
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (R0[c] * m[0] + R0[3 + c] * m[1]) + R0[6 + c] * m[2];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) pts[3 * (size_t)j + c] = o[c];
        }
    } else {
        return_input();
    }
    if (tid == 0) {
        a.info[w * 4] = take ? RPE_WINDOW_OK : RPE_WINDOW_REJECTED; a.info[w * 4 + 1] = iters; a.info[w * 4 + 2] = acc; a.info[w * 4 + 3] = A;
        const double before = sqrt(cost0 / (double)nobs);
        a.rms[w * 2] = before;
        a.rms[w * 2 + 1] = take ? sqrt(cost / (double)nobs) : before;
    }
}

// The three launches of one job.  The buffers are the caller's business (rpe_bundle_windows, rpe_features.hip)
void rpe_launch_windows(rpe_handle *h, const RpeWindowJob &job)
{
    WbArgs a{};
    a.job = job;
    a.obs = (WbObs *)h->wb.obs;
    a.ptrack = h->wb.ptrack; a.pobs = h->wb.pobs; a.fcnt = h->wb.fcnt; a.counts = h->wb.counts; a.info = h->wb.info;
    a.state = h->wb.state; a.points = h->wb.points; a.Rout = h->wb.Rout; a.Tout = h->wb.Tout; a.rms = h->wb.rms;
    const dim3 blk(256);
    if (job.scene.n_obs > 0) hipLaunchKernelGGL(wb_prepare_kernel, dim3((unsigned)(((long long)job.scene.n_obs + 255) / 256)), blk, 0, h->stream, a);
    hipLaunchKernelGGL(wb_gather_kernel, dim3(job.n_win), blk, 0, h->stream, a);
    hipLaunchKernelGGL(wb_solve_kernel, dim3(job.n_win), blk, 0, h->stream, a);
}
