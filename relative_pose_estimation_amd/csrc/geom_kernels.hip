// geom_kernels.hip -- essential-matrix RANSAC and pose recovery on gfx950.
//
// Replaces cv2.findEssentialMat(pts1, pts2, K, RANSAC, 0.999, 1.0)
// (reference src/core/pose_estimator.py:522-527) and cv2.recoverPose(E, pts1, pts2, K)
// (:533).  Sequential OpenCV semantics (calib3d/ptsetreg.cpp RANSACPointSetRegistrator::run:
// fixed RNG stream, "strictly more inliers wins", adaptive niters) are reproduced on a
// parallel machine by evaluating a chunk of iterations at a time (32, 96, 384, 512) and replaying
// the update rule over the per-model inlier counts:
//   ransac_prepare : normalise points with K (f64), reset per-pair state
//   ransac_poly    : one lane = one minimal sample: null space, 10x20 elimination in lane-interleaved
//                    LDS, determinant polynomial of degree 10 (f64)
//   ransac_roots   : 8 lanes per sample (RG): lane = bracketing interval of the derivative chain, safeguarded
//                    Newton, ballot/shuffle compaction; back-substitution lane = root -> up to 10 models
//   ransac_score   : workgroup per (pair, 8 iterations) (SCORE_GROUP), wave per model: Sampson error (f64 -> f32
//                    compare) over the matches in LDS, shuffle-reduced inlier counts
//   ransac_update  : wave per pair: the sequential "strictly more inliers wins / niters shrinks / stop at
//                    niters" rule as prefix-max and prefix-min scans (bit-identical termination)
//   ransac_mask    : inlier mask of the winning model (stage API only)
//   recover_pose   : 3x3 one-sided Jacobi SVD, 4 candidate poses, per-point 4x4 Jacobi
//                    DLT triangulation + cheirality vote, wave-reduced counts
// All f64 arithmetic uses the oracle's operation order (compiled with -ffp-contract=off).
#include "rpe_internal.h"
#include "pose_triangulate.h"
#include "geom_device.h"
#include <float.h>
#include <algorithm>

// ------------------------------------------------ polynomial bookkeeping
// lin: x y z 1 ; quad: x2 y2 z2 xy xz yz x y z 1 ;
// cubic (Nister's elimination order): x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
__device__ static const signed char LL2Q[4][4] = {{0, 3, 4, 6}, {3, 1, 5, 7}, {4, 5, 2, 8}, {6, 7, 8, 9}};
__device__ static const signed char QL2C[10][4] = {{0, 2, 4, 5},   {3, 1, 6, 7},   {10, 13, 16, 17}, {2, 3, 8, 9},    {4, 8, 10, 11},
                                                    {8, 6, 13, 14}, {5, 9, 11, 12}, {9, 7, 14, 15},   {11, 14, 17, 18}, {12, 15, 18, 19}};

__device__ static void ll_acc(double *c, const double *a, const double *b)
{
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) c[LL2Q[i][j]] += a[i] * b[j];
}
__device__ static void ql_acc(double *c, const double *a, const double *b, double s)
{
    for (int i = 0; i < 10; ++i) for (int j = 0; j < 4; ++j) c[QL2C[i][j]] += s * (a[i] * b[j]);
}

// generic path (leading coefficient trimmed to degree < 10: rare): one lane walks the whole chain serially with dynamic
// indexing.  Its arrays live in workspace the CALLER provides (LDS in ransac_roots_kernel): as private arrays they would
// be a scratch segment of their own.  The kernel has one all the same: its metadata shows 114 spilled VGPRs of the
// degree-10 levels and 460 B of scratch (open).  Inlined: as a call this function added its
// own frame to that segment.
// Level k's polynomial is c differentiated n - k times, rebuilt from c on every level by the same multiplications in the
// same order as the oracle's derivative table (identical values), so the workspace is two rows instead of the 11 x 11
// table.  Both rows are kept zero above their degree: they are the oracle's zero-padded coefficients, evaluated by
// estrin<10> / estrin<9>.
#define GEN_WS_DOUBLES (4 * 11)          // p[11], dp[11], rts[2][11]
__device__ __forceinline__ int poly_real_roots_generic(const double *c, int n, double *roots, double *ws)
{
    double *p = ws, *dp = ws + 11, *rts = ws + 22;          // rts[which * 11 + i]
    int nr_prev = 0, cur = 0;
    for (int k = 1; k <= n; ++k) {
        for (int i = 0; i <= n; ++i) p[i] = c[i];
        for (int kk = n; kk > k; --kk)
            for (int i = 0; i < kk; ++i) p[i] = p[i + 1] * (double)(i + 1);
        if (k == 1) { rts[0] = -p[0] / p[1]; nr_prev = 1; cur = 0; continue; }
        for (int i = 0; i < k; ++i) dp[i] = p[i + 1] * (double)(i + 1);
        for (int i = k; i <= 10; ++i) { dp[i] = 0.; if (i > k) p[i] = 0.; }
        const double *crit = rts + cur * 11;
        double *out = rts + (cur ^ 1) * 11;
        int nout = 0;
        const double R = root_bound<0>(p, k);
        for (int iv = 0; iv <= nr_prev; ++iv) {
            double root;
            if (bracket_root<10>(p, dp, (iv == 0) ? -R : crit[iv - 1], (iv == nr_prev) ? R : crit[iv], R, true, root)) out[nout++] = root;
        }
        nr_prev = nout; cur ^= 1;
    }
    for (int i = 0; i < nr_prev; ++i) roots[i] = rts[cur * 11 + i];
    return nr_prev;
}

// ---- degree-10 fast path: the polynomial of each chain level lives in registers (static indexing); arithmetic
// identical to the generic path.  Level K's polynomial p = c10 differentiated 10 - K times and dp = p', by the
// multiplications of the oracle's derivative table in its order; returns the root bound of p.
template <int K>
__device__ __forceinline__ double level_poly(const double (&c10)[11], double (&p)[11], double (&dp)[11])
{
#pragma unroll
    for (int i = 0; i <= 10; ++i) p[i] = c10[i];
#pragma unroll
    for (int kk = 10; kk > K; --kk)
#pragma unroll
        for (int i = 0; i < kk; ++i) p[i] = p[i + 1] * (double)(i + 1);
#pragma unroll
    for (int i = 0; i < K; ++i) dp[i] = p[i + 1] * (double)(i + 1);
    return root_bound<K>(p);
}

// Nister five-point solver (five-point.cpp EMEstimatorCallback::runKernel restated;
// same operation order as oracle/geom_oracle.c)
// mx: this lane's 10x20 elimination matrix in LDS, element (i,j) at mx[(i*20+j)*POLY_LANES]
// (lane-interleaved: conflict-free ds_read/write_b64, no scratch round trips)
#define SCORE_GROUP 8       // iterations scored by one workgroup of ransac_score_kernel
#define POLY_LANES 32        // minimal samples per wave of ransac_poly_kernel (lanes 32..63 idle): see the kernel
#define MX(i, j) mx[((i) * 20 + (j)) * POLY_LANES]
// Part A of the solver (LDS-heavy): null space, constraint matrix, Gauss-Jordan, det B(z).
// Writes the hypothesis record rec[k*64] (k = 0..86): c10[11], Bx[12], By[12], B1[15], Eb[36], degree n;
// returns 0 when the elimination is singular.
#define HYP_DOUBLES 88
__device__ static int five_point_poly(const double *x1, const double *x2, double *mx, double *rec)
{
    double A[9][5];
    for (int k = 0; k < 5; ++k) {
        double a = x1[2 * k], b = x1[2 * k + 1], c = x2[2 * k], d = x2[2 * k + 1];
        A[0][k] = c * a; A[1][k] = c * b; A[2][k] = c;
        A[3][k] = d * a; A[4][k] = d * b; A[5][k] = d;
        A[6][k] = a;     A[7][k] = b;     A[8][k] = 1.;
    }
    double hv[5][9], beta[5];
    for (int k = 0; k < 5; ++k) {
        double nrm = 0.;
        for (int i = k; i < 9; ++i) nrm += A[i][k] * A[i][k];
        nrm = sqrt(nrm);
        double alpha = A[k][k] > 0. ? -nrm : nrm;
        for (int i = 0; i < 9; ++i) hv[k][i] = 0.;
        hv[k][k] = A[k][k] - alpha;
        for (int i = k + 1; i < 9; ++i) hv[k][i] = A[i][k];
        double vn = 0.;
        for (int i = k; i < 9; ++i) vn += hv[k][i] * hv[k][i];
        beta[k] = vn > 0. ? 2. / vn : 0.;
        for (int j = k; j < 5; ++j) {
            double s = 0.;
            for (int i = k; i < 9; ++i) s += hv[k][i] * A[i][j];
            s *= beta[k];
            for (int i = k; i < 9; ++i) A[i][j] -= s * hv[k][i];
        }
    }
    double Eb[4][9];
    for (int m = 0; m < 4; ++m) {
        double v[9];
        for (int i = 0; i < 9; ++i) v[i] = 0.;
        v[5 + m] = 1.;
        for (int k = 4; k >= 0; --k) {
            double s = 0.;
            for (int i = k; i < 9; ++i) s += hv[k][i] * v[i];
            s *= beta[k];
            for (int i = k; i < 9; ++i) v[i] -= s * hv[k][i];
        }
        for (int i = 0; i < 9; ++i) Eb[m][i] = v[i];
    }
    double El[9][4];
    for (int e = 0; e < 9; ++e) for (int m = 0; m < 4; ++m) El[e][m] = Eb[m][e];
    double EEt[3][3][10];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) for (int q = 0; q < 10; ++q) EEt[i][j][q] = 0.;
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) {
        for (int k = 0; k < 3; ++k) ll_acc(EEt[i][j], El[i * 3 + k], El[j * 3 + k]);
        if (j != i) for (int q = 0; q < 10; ++q) EEt[j][i][q] = EEt[i][j][q];
    }
    double htr[10];
    for (int q = 0; q < 10; ++q) htr[q] = 0.5 * ((EEt[0][0][q] + EEt[1][1][q]) + EEt[2][2][q]);
    for (int i = 0; i < 3; ++i) for (int q = 0; q < 10; ++q) EEt[i][i][q] -= htr[q];

    // constraint rows are accumulated in registers/scratch one at a time, then stored to LDS
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double row[20];
        for (int q = 0; q < 20; ++q) row[q] = 0.;
        for (int k = 0; k < 3; ++k) ql_acc(row, EEt[i][k], El[k * 3 + j], 1.);
        for (int q = 0; q < 20; ++q) MX(i * 3 + j, q) = row[q];
    }
    {
        double m0[10], m1[10], m2[10], neg[4];
        for (int q = 0; q < 10; ++q) { m0[q] = 0.; m1[q] = 0.; m2[q] = 0.; }
        ll_acc(m0, El[4], El[8]); for (int q = 0; q < 4; ++q) neg[q] = -El[5][q]; ll_acc(m0, neg, El[7]);
        ll_acc(m1, El[3], El[8]); ll_acc(m1, neg, El[6]);
        ll_acc(m2, El[3], El[7]); for (int q = 0; q < 4; ++q) neg[q] = -El[4][q]; ll_acc(m2, neg, El[6]);
        double row[20];
        for (int q = 0; q < 20; ++q) row[q] = 0.;
        ql_acc(row, m0, El[0], 1.);
        ql_acc(row, m1, El[1], -1.);
        ql_acc(row, m2, El[2], 1.);
        for (int q = 0; q < 20; ++q) MX(9, q) = row[q];
    }
    for (int c = 0; c < 10; ++c) {
        double col[10];
#pragma unroll
        for (int r = 0; r < 10; ++r) col[r] = MX(r, c);          // 10 independent LDS reads in flight
        int piv = c; double best = fabs(col[c]);
        for (int r = c + 1; r < 10; ++r) { double a = fabs(col[r]); if (a > best) { best = a; piv = r; } }
        if (best == 0.) return 0;
        double prow[20], crow[20];
#pragma unroll
        for (int j = 0; j < 20; ++j) { prow[j] = MX(piv, j); crow[j] = MX(c, j); }
        if (piv != c) {
#pragma unroll
            for (int j = 0; j < 20; ++j) MX(piv, j) = crow[j];
            double t = col[c]; col[c] = col[piv]; col[piv] = t;
        }
        const double inv = 1. / prow[c];
#pragma unroll
        for (int j = 0; j < 20; ++j) { if (j >= c) prow[j] = prow[j] * inv; }
#pragma unroll
        for (int j = 0; j < 20; ++j) MX(c, j) = prow[j];
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = col[r];
            if (f == 0.) continue;
            double row[20];
#pragma unroll
            for (int j = 0; j < 20; ++j) row[j] = MX(r, j);
#pragma unroll
            for (int j = 0; j < 20; ++j) { if (j >= c) row[j] -= f * prow[j]; }
#pragma unroll
            for (int j = 0; j < 20; ++j) MX(r, j) = row[j];
        }
    }
    double Bx[3][4], By[3][4], B1[3][5];
    for (int i = 0; i < 3; ++i) {
        double e[10], f[10];
        for (int q = 0; q < 10; ++q) { e[q] = MX(4 + 2 * i, 10 + q); f[q] = MX(5 + 2 * i, 10 + q); }
        Bx[i][3] = -f[0]; Bx[i][2] = e[0] - f[1]; Bx[i][1] = e[1] - f[2]; Bx[i][0] = e[2];
        By[i][3] = -f[3]; By[i][2] = e[3] - f[4]; By[i][1] = e[4] - f[5]; By[i][0] = e[5];
        B1[i][4] = -f[6]; B1[i][3] = e[6] - f[7]; B1[i][2] = e[7] - f[8]; B1[i][1] = e[8] - f[9]; B1[i][0] = e[9];
    }
    double c10[11];
    for (int i = 0; i < 11; ++i) c10[i] = 0.;
    for (int i = 0; i < 3; ++i) {
        int r0 = (i + 1) % 3, r1 = (i + 2) % 3;
        double minor[7];
        for (int k = 0; k < 7; ++k) minor[k] = 0.;
        for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b)
            minor[a + b] += Bx[r0][a] * By[r1][b] - Bx[r1][a] * By[r0][b];
        for (int a = 0; a < 7; ++a) for (int b = 0; b < 5; ++b) c10[a + b] += minor[a] * B1[i][b];
    }
    int n = 10;
    for (; n > 1; --n) if (fabs(c10[n]) > DBL_EPSILON) break;
    for (int i = 0; i < 11; ++i) rec[i * 64] = c10[i];
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 4; ++k) { rec[(11 + i * 4 + k) * 64] = Bx[i][k]; rec[(23 + i * 4 + k) * 64] = By[i][k]; }
        for (int k = 0; k < 5; ++k) rec[(35 + i * 5 + k) * 64] = B1[i][k];
    }
    for (int m = 0; m < 4; ++m) for (int e = 0; e < 9; ++e) rec[(50 + m * 9 + e) * 64] = Eb[m][e];
    rec[86 * 64] = (double)n;
    return 1;
}

// ---------------------------------------------------------------- prepare
// CAM (rpe_internal.h, RpeCamSrc): false = the shared K; true = the pair's two cameras, each point normalised and
// undistorted with the camera of its own frame.  One thread per match (RpePairNormalise: the cameras are
// workgroup-uniform scalar loads and the lens test is a uniform branch, the five iterations run in registers).
// Returns the pair's match count.
template <bool CAM>
__device__ __forceinline__ int normalise_match(const float2 *__restrict__ pts1, const float2 *__restrict__ pts2,
                                               const int *__restrict__ m_n, const double *__restrict__ K, const RpeCamSrc &cam,
                                               double2 *__restrict__ n1, double2 *__restrict__ n2, int max_matches)
{
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int M = min(m_n[pair], max_matches);
    const RpePairNormalise<CAM> normalise(K, cam, pair);
    if (i < M) {
        const long long o = (long long)pair * max_matches + i;
        normalise(pts1[o], pts2[o], n1[o], n2[o]);
    }
    return M;
}

// d_n1 / d_n2 of the uploaded points of a stage call that runs no RANSAC (recoverPose, the refinement)
template <bool CAM>
__global__ __launch_bounds__(256) void normalise_kernel(const float2 *__restrict__ pts1, const float2 *__restrict__ pts2,
                                                         const int *__restrict__ m_n, const double *__restrict__ K,
                                                         const RpeCamSrc cam,
                                                         double2 *__restrict__ n1, double2 *__restrict__ n2, int max_matches)
{
    normalise_match<CAM>(pts1, pts2, m_n, K, cam, n1, n2, max_matches);
}

template <bool CAM>
__global__ __launch_bounds__(256) void ransac_prepare_kernel(const float2 *__restrict__ pts1, const float2 *__restrict__ pts2,
                                                              const int *__restrict__ m_n, const double *__restrict__ K,
                                                              const RpeCamSrc cam,
                                                              double2 *__restrict__ n1, double2 *__restrict__ n2,
                                                              RpeRansacState *__restrict__ st, int *__restrict__ found,
                                                              int max_matches, int max_iters)
{
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int M = normalise_match<CAM>(pts1, pts2, m_n, K, cam, n1, n2, max_matches);
    if (i == 0) {
        RpeRansacState s;
        s.best_count = 0; s.best_iter = -1; s.best_model = -1;
        s.niters = max_iters; s.next_iter = 0; s.done = (M < 5); s.found = 0; s.M = M; s.iters_run = 0; s.pad_ = 0;
        for (int e = 0; e < 9; ++e) s.E[e] = 0.;
        st[pair] = s;
        found[pair] = 0;
    }
}

// ------------------------------------------------------------------ solve
// A: one wave per (pair, 32 iterations), 32 active lanes.  The 10x20 elimination lives in LDS (1600 B per sample); the
// kernel retires 0.015 G vector instructions in 0.44 ms -- 3 % of the issue roof: it is pure single-wave latency, and a
// full 64-sample wave (100 KB) fits a CU only once.  Half-filled waves (50 KB) fit three times: three latency chains per
// CU instead of one (the idle lanes cost nothing a latency-bound kernel would have used).
__global__ __launch_bounds__(POLY_LANES) void ransac_poly_kernel(const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                                  const RpeRansacState *__restrict__ st,
                                                                  const unsigned short *__restrict__ subsets,
                                                                  double *__restrict__ hyp, int *__restrict__ nmodels,
                                                                  int max_matches, int max_iters)
{
    __shared__ double s_mx[200 * POLY_LANES];
    // blockIdx.y = wave-chunk of 64 iterations * (64 / POLY_LANES) + part: lanes of this block = samples part*POLY_LANES .. of the chunk
    const int pair = blockIdx.x, wv = blockIdx.y / (64 / POLY_LANES), lane = (blockIdx.y % (64 / POLY_LANES)) * POLY_LANES + threadIdx.x;
    const RpeRansacState s = st[pair];
    if (s.done) return;
    const int it = s.next_iter + wv * 64 + lane;
    const long long slot = (long long)pair * RPE_RANSAC_MAXCHUNK + wv * 64 + lane;
    int ok = 0;
    const bool all5 = (s.M == 5);
    if (it < s.niters && (!all5 || it == 0)) {
        double x1[10], x2[10];
        const unsigned short *sub = subsets + ((long long)s.M * max_iters + it) * 5;
        for (int k = 0; k < 5; ++k) {
            int v = all5 ? k : (int)sub[k];
            double2 a = n1[(long long)pair * max_matches + v], b = n2[(long long)pair * max_matches + v];
            x1[2 * k] = a.x; x1[2 * k + 1] = a.y; x2[2 * k] = b.x; x2[2 * k + 1] = b.y;
        }
        ok = five_point_poly(x1, x2, s_mx + threadIdx.x, hyp + ((long long)pair * (RPE_RANSAC_MAXCHUNK / 64) + wv) * HYP_DOUBLES * 64 + lane);
    }
    nmodels[slot] = ok ? -1 : 0;          // -1: record valid, roots pending
}

// B: roots + back-substitution, RG = 8 lanes per minimal sample.  The real roots of the degree-k
// derivative split the line into <= k+1 intervals with at most one root of the degree-(k+1)
// derivative each, and those intervals are independent: lane j of a group brackets and refines
// interval j, the roots are compacted in interval order (ballot + n-th set bit + shuffle), so every
// lane performs exactly the arithmetic the sequential oracle performs for that interval and the
// root list comes out in the same order.  The kernel is bound by vector-instruction issue (r02 PMC: 0.2 G
// instructions in 0.43 ms for the first 64-iteration chunk, 76 % of the measured issue roof), and a wave costs what
// its slowest interval costs whatever the number of busy lanes: with 16 lanes per sample 70 % of the lanes idled (the
// derivative chain of these polynomials rarely has more than 4 real roots on a level); 8 lanes per sample halve the
// waves.  A level with more than 8 intervals (>= 8 real roots below it: levels 9 and 10 only) takes two rounds.
#define RG 8
#define RPE_RANSAC_FIRST_CHUNK 32   // iterations of the first launch group (schedule: rpe_launch_ransac)
__device__ __forceinline__ int nth_set_bit(unsigned m, int k)
{
    for (int t = 0; t < k; ++t) m &= m - 1;
    return m ? __ffs((int)m) - 1 : 0;
}

// crit: in = root #j of the level below (j < nr_prev), out = root #j of this level (j < return value)
template <int K>
__device__ __forceinline__ int roots_level_grp(const double (&c)[11], double &crit, int nr_prev, int j, int gbase)
{
    double p[11], dp[11];
    const double R = level_poly<K>(c, p, dp);
    const double below = __shfl_up(crit, 1);
    double root = 0.;
    const bool has = bracket_root<K>(p, dp, (j == 0) ? -R : below, (j == nr_prev) ? R : crit, R, j <= nr_prev, root);
    const unsigned m = (unsigned)(__ballot(has) >> gbase) & ((1u << RG) - 1u);
    crit = __shfl(root, gbase + nth_set_bit(m, j));
    return __popc(m);
}

// Levels 9 and 10 can have 9 / 10 intervals (8 / 9 real roots below): lane j then also takes interval 8 + j in a second
// round (lanes 0 and 1 only) and keeps root #(8 + j) in crit1.  Same arithmetic per interval, same root order.
template <int K>
__device__ __forceinline__ int roots_level_grp2(const double (&c)[11], double &crit0, double &crit1, int nr_prev, int j, int gbase)
{
    double p[11], dp[11];
    const double R = level_poly<K>(c, p, dp);
    // crit[iv - 1] and crit[iv] of this lane's interval in each round (nr_prev >= RG here)
    const double below0 = __shfl_up(crit0, 1);                    // crit[j - 1]
    const double c7 = __shfl(crit0, gbase + RG - 1), c8 = __shfl(crit1, gbase);
    double root[2] = {0., 0.};
    bool has[2] = {false, false};
#pragma unroll 1
    for (int rnd = 0; rnd < 2; ++rnd) {
        const int iv = rnd * RG + j;
        const double a = rnd == 0 ? (j == 0 ? -R : below0) : (j == 0 ? c7 : c8);
        const double b = (iv == nr_prev) ? R : (rnd == 0 ? crit0 : crit1);
        double r = 0.;
        const bool h = bracket_root<K>(p, dp, a, b, R, iv <= nr_prev, r);
        if (rnd == 0) { root[0] = r; has[0] = h; } else { root[1] = r; has[1] = h; }
    }
    const unsigned mA = (unsigned)(__ballot(has[0]) >> gbase) & ((1u << RG) - 1u);
    const unsigned mB = (unsigned)(__ballot(has[1]) >> gbase) & ((1u << RG) - 1u);
    const int nA = __popc(mA), nB = __popc(mB);
    // root #r of this level: the r-th found in round 0, then those of round 1
    const double a0 = __shfl(root[0], gbase + nth_set_bit(mA, j)), b0 = __shfl(root[1], gbase + nth_set_bit(mB, max(j - nA, 0)));
    const double a1 = __shfl(root[0], gbase + nth_set_bit(mA, min(j + RG, 31))), b1 = __shfl(root[1], gbase + nth_set_bit(mB, max(j + RG - nA, 0)));
    crit0 = j < nA ? a0 : b0;
    crit1 = j + RG < nA ? a1 : b1;
    return nA + nB;
}

#define ROOTS_WS (GEN_WS_DOUBLES + 11 + 10)      // generic-path workspace + coefficients + root list, per group
__global__ __launch_bounds__(256, 4) void ransac_roots_kernel(const RpeRansacState *__restrict__ st, const double *__restrict__ hyp,
                                                               double *__restrict__ models, int *__restrict__ nmodels, int n_pairs,
                                                               int per_pair /* samples of a pair in this launch: the chunk */)
{
    __shared__ double s_gen[256 / RG][ROOTS_WS];
    const int tid = threadIdx.x, j = tid & (RG - 1), gbase = tid & 63 & ~(RG - 1);
    const long long sidx = (long long)blockIdx.x * (256 / RG) + (tid / RG);     // sample = (pair, wv, lane)
    const int pair = (int)(sidx / per_pair), rem = (int)(sidx - (long long)pair * per_pair);
    const int wv = rem >> 6, lane = rem & 63;
    if (pair >= n_pairs) return;
    const RpeRansacState s = st[pair];
    if (s.done || s.next_iter + wv * 64 >= s.niters) return;          // uniform per workgroup
    const long long slot = (long long)pair * RPE_RANSAC_MAXCHUNK + wv * 64 + lane;
    if (nmodels[slot] != -1) return;                                   // uniform per group
    const double *rec = hyp + ((long long)pair * (RPE_RANSAC_MAXCHUNK / 64) + wv) * HYP_DOUBLES * 64 + lane;
    double c10[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) c10[i] = rec[i * 64];
    const int n = (int)rec[86 * 64];
    double z = 0., z1 = 0.;            // roots #j and #(RG + j) of the current level
    int nroots = 0;
    const bool generic = (n != 10);
    if (!generic) {
        {
            double p[11], dp[11];
            level_poly<1>(c10, p, dp);
            z = -p[0] / p[1];          // level 1 in closed form, as the oracle has it
        }
        nroots = 1;
        // a level has nroots + 1 intervals; levels 2..8 cannot exceed the 8 lanes (nroots <= K - 1 <= 7 below level K <= 8),
        // levels 9 and 10 take a second round when they do
        nroots = roots_level_grp<2>(c10, z, nroots, j, gbase);
        nroots = roots_level_grp<3>(c10, z, nroots, j, gbase);
        nroots = roots_level_grp<4>(c10, z, nroots, j, gbase);
        nroots = roots_level_grp<5>(c10, z, nroots, j, gbase);
        nroots = roots_level_grp<6>(c10, z, nroots, j, gbase);
        nroots = roots_level_grp<7>(c10, z, nroots, j, gbase);
        nroots = roots_level_grp<8>(c10, z, nroots, j, gbase);
        if (nroots + 1 > RG) nroots = roots_level_grp2<9>(c10, z, z1, nroots, j, gbase);       // group-uniform
        else nroots = roots_level_grp<9>(c10, z, nroots, j, gbase);
        if (nroots + 1 > RG) nroots = roots_level_grp2<10>(c10, z, z1, nroots, j, gbase);
        else nroots = roots_level_grp<10>(c10, z, nroots, j, gbase);
    }
    double *ws = s_gen[tid / RG];
    if (generic) {
        // the group leader runs the whole chain serially in its LDS workspace (groups are wave-local: the leader's LDS
        // writes are visible to its neighbours after the wave barrier)
        int nr = 0;
        if (j == 0) {
#pragma unroll
            for (int t = 0; t < 11; ++t) ws[GEN_WS_DOUBLES + t] = c10[t];
            nr = poly_real_roots_generic(ws + GEN_WS_DOUBLES, n, ws + GEN_WS_DOUBLES + 11, ws);
        }
        __builtin_amdgcn_wave_barrier();
        nroots = __shfl(nr, gbase);
    }
    // back-substitution: lane j <- root #j (five_point_roots' loop body), models compacted in root order; more than RG
    // roots (9 or 10: either path can return them) take a second round
    int nmod = 0;
    for (int r0 = 0; r0 < nroots; r0 += RG) {                          // group-uniform trip count (1, rarely 2)
        const int ri = r0 + j;
        __asm__ volatile("" ::: "memory");     // keep the ~75 record loads inside the round: hoisted out of the loop they spill
        if (generic) { if (ri < nroots) z = ws[GEN_WS_DOUBLES + 11 + ri]; }
        else if (r0) z = z1;
        bool okm = false;
        double Ev[9];
        if (ri < nroots) {
            double bz[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double x3 = rec[(11 + i * 4 + 3) * 64], x2 = rec[(11 + i * 4 + 2) * 64], x1 = rec[(11 + i * 4 + 1) * 64], x0 = rec[(11 + i * 4) * 64];
                const double y3 = rec[(23 + i * 4 + 3) * 64], y2 = rec[(23 + i * 4 + 2) * 64], y1 = rec[(23 + i * 4 + 1) * 64], y0 = rec[(23 + i * 4) * 64];
                const double w4 = rec[(35 + i * 5 + 4) * 64], w3 = rec[(35 + i * 5 + 3) * 64], w2 = rec[(35 + i * 5 + 2) * 64],
                             w1 = rec[(35 + i * 5 + 1) * 64], w0 = rec[(35 + i * 5) * 64];
                bz[i][0] = ((x3 * z + x2) * z + x1) * z + x0;
                bz[i][1] = ((y3 * z + y2) * z + y1) * z + y0;
                bz[i][2] = (((w4 * z + w3) * z + w2) * z + w1) * z + w0;
            }
            double bestn = -1., xv0 = 0., xv1 = 0., xv2 = 0.;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int q0 = i, q1 = (i + 1) % 3;
                const double cx = bz[q0][1] * bz[q1][2] - bz[q0][2] * bz[q1][1];
                const double cy = bz[q0][2] * bz[q1][0] - bz[q0][0] * bz[q1][2];
                const double cz = bz[q0][0] * bz[q1][1] - bz[q0][1] * bz[q1][0];
                const double nn = cx * cx + cy * cy + cz * cz;
                if (nn > bestn) { bestn = nn; xv0 = cx; xv1 = cy; xv2 = cz; }
            }
            if (bestn > 0.) {
                const double inv = 1. / sqrt(bestn);
                const double w = xv2 * inv;
                if (!(fabs(w) < 1e-10)) {
                    const double x = xv0 / xv2, y = xv1 / xv2;
                    double nrm = 0.;
#pragma unroll
                    for (int e = 0; e < 9; ++e) {
                        Ev[e] = ((rec[(50 + e) * 64] * x + rec[(59 + e) * 64] * y) + rec[(68 + e) * 64] * z) + rec[(77 + e) * 64];
                        nrm += Ev[e] * Ev[e];
                    }
                    nrm = sqrt(nrm);
                    if (nrm > 0.) {
                        okm = true;
#pragma unroll
                        for (int e = 0; e < 9; ++e) Ev[e] = Ev[e] / nrm;
                    }
                }
            }
        }
        const unsigned m = (unsigned)(__ballot(okm) >> gbase) & ((1u << RG) - 1u);
        if (okm) {
            double *dst = models + (slot * RPE_MAX_MODELS + nmod + __popc(m & ((1u << j) - 1u))) * 9;
#pragma unroll
            for (int e = 0; e < 9; ++e) dst[e] = Ev[e];
        }
        nmod += __popc(m);
    }
    if (j == 0) nmodels[slot] = nmod;
}

// ------------------------------------------------------- Sampson inlier test
// EMEstimatorCallback::computeError + findInliers: (float)err <= (float)(thr*thr), err = num / den in the oracle's
// operation order (count_inliers)
__device__ __forceinline__ void sampson_terms(const double *E, double x1, double y1, double x2, double y2, double &num, double &den)
{
    double Ex0 = (E[0] * x1 + E[1] * y1) + E[2];
    double Ex1 = (E[3] * x1 + E[4] * y1) + E[5];
    double Ex2 = (E[6] * x1 + E[7] * y1) + E[8];
    double Et0 = (E[0] * x2 + E[3] * y2) + E[6];
    double Et1 = (E[1] * x2 + E[4] * y2) + E[7];
    double x2tEx1 = (x2 * Ex0 + y2 * Ex1) + Ex2;
    double a = Ex0 * Ex0, b = Ex1 * Ex1, c = Et0 * Et0, d = Et1 * Et1;
    num = x2tEx1 * x2tEx1; den = ((a + b) + c) + d;
}

__device__ __forceinline__ int sampson_inlier(const double *E, double x1, double y1, double x2, double y2, float thr2)
{
    double num, den;
    sampson_terms(E, x1, y1, x2, y2, num, den);
    return (float)(num / den) <= thr2;
}

// The same predicate without the f64 division (a ~30-instruction IEEE sequence in the innermost RANSAC loop).
// (float)(num / den) <= thr2  <=>  fl64(num / den) <= B, B = the largest double that still rounds (to nearest even) to a
// float <= thr2.  num <= 0.999.. * fl(B * den) proves the left side, num >= 1.000.. * fl(B * den) disproves it (margins
// 2^-40, far above the 2^-53 rounding of the product and of the quotient); only the sliver in between (and den <= 0 /
// non-finite values) takes the exact division.  Bit-identical to sampson_inlier by construction.
struct SampsonBound { double B; };
__device__ __forceinline__ SampsonBound sampson_bound(float thr2)
{
    const unsigned u = __float_as_uint(thr2);
    const float nf = __uint_as_float(u + 1u);                             // next float above thr2 (thr2 > 0, finite)
    const double m = 0.5 * ((double)thr2 + (double)nf);                   // exact midpoint: ties go to the even float
    SampsonBound b;
    b.B = (u & 1u) ? __longlong_as_double(__double_as_longlong(m) - 1) : m;
    return b;
}
__device__ __forceinline__ int sampson_inlier_fast(const double *E, double x1, double y1, double x2, double y2, float thr2, SampsonBound sb)
{
    double num, den;
    sampson_terms(E, x1, y1, x2, y2, num, den);
    const double p = sb.B * den;
    if (den > 0. && p < 1e300) {
        if (num <= p * (1. - 0x1p-40)) return 1;
        if (num >= p * (1. + 0x1p-40)) return 0;
    }
    return (float)(num / den) <= thr2;
}

// RANSACUpdateNumIters with log() terms tabulated on the host per (M, goodCount)
__device__ __forceinline__ int update_niters(const double *nit_denom, const int *nit_round, double num, int M, int good, int niters)
{
    long long idx = (long long)M * (M + 1) / 2 + good;
    int r = nit_round[idx];
    if (r == -1) return 0;
    double denom = nit_denom[idx];
    return (denom >= 0 || -num >= niters * (-denom)) ? niters : r;
}

// ------------------------------------------------------------------ score
// One workgroup per (pair, group of SCORE_GROUP iterations): a wave scores its models one after the other, so the group
// size sets the kernel's latency (the later RANSAC rounds run few pairs and are pure latency): SCORE_GROUP = 8
// iterations per workgroup = 8x the workgroups of a 64-iteration grouping, each an eighth as long.  The normalised
// matches sit in LDS; each of the 4 waves scores a different model (lanes stride over the matches, Sampson error
// f64 -> f32 compare, wave-shuffle popcount), so there is no cross-wave reduction.  Counts go to HBM.
template <bool CAM>
__global__ __launch_bounds__(256) void ransac_score_kernel(const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                            const RpeRansacState *__restrict__ st, const double *__restrict__ models,
                                                            const int *__restrict__ nmodels, const double *__restrict__ K,
                                                            const RpeCamSrc cam, double threshold, int *__restrict__ counts, int max_matches, int use_lds)
{
    extern __shared__ double2 s_pts[];              // [2][max_matches] when the points fit LDS (use_lds)
    __shared__ int s_nm[SCORE_GROUP], s_first[SCORE_GROUP + 1];
    const int pair = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const RpeRansacState s = st[pair];
    if (s.done || s.M <= 5 || s.next_iter + grp * SCORE_GROUP >= s.niters) return;
    const int M = s.M;
    // max_matches > 2048 ("no truncation" configurations): 32 B per match no longer fit the 64 KB of dynamic LDS;
    // the points are then read from HBM / L2 directly (every wave walks the same 64 KB-scale array)
    const double2 *sp1 = n1 + (long long)pair * max_matches, *sp2 = n2 + (long long)pair * max_matches;
    if (use_lds) {
        double2 *l1 = s_pts, *l2 = s_pts + max_matches;
        for (int i = tid; i < M; i += 256) { l1[i] = sp1[i]; l2[i] = sp2[i]; }
        sp1 = l1; sp2 = l2;
    }
    const long long slot0 = (long long)pair * RPE_RANSAC_MAXCHUNK + grp * SCORE_GROUP;
    if (tid < SCORE_GROUP) s_nm[tid] = max(nmodels[slot0 + tid], 0);
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int k = 0; k < SCORE_GROUP; ++k) { s_first[k] = acc; acc += s_nm[k]; } s_first[SCORE_GROUP] = acc; }
    __syncthreads();
    const double thr = threshold / rpe_pair_focal<CAM>(K, cam, pair);
    const float thr2 = (float)(thr * thr);
    const SampsonBound sbound = sampson_bound(thr2);
    const int total = s_first[SCORE_GROUP];
    // a wave scores models j = wv, wv + 4, ... one after the other; the 72 bytes of the NEXT model are fetched (lanes 0..8,
    // one double each) before the current one is scored, so the HBM / L2 round trip of the model hides behind ~400
    // instructions of Sampson arithmetic instead of heading every iteration (the kernel ran at 28 % of its issue roof)
    int k = 0, kn = 0;
    double e_next = 0.;
    int j = wv;
    if (j < total) {
        while (s_first[kn + 1] <= j) ++kn;
        if (lane < 9) e_next = models[((slot0 + kn) * RPE_MAX_MODELS + (j - s_first[kn])) * 9 + lane];
    }
    for (; j < total; j += 4) {                      // j-th model of this group, flattened (iteration-major)
        k = kn;
        const int m = j - s_first[k];
        const double e_cur = e_next;
        const int jn = j + 4;
        if (jn < total) {
            while (s_first[kn + 1] <= jn) ++kn;
            if (lane < 9) e_next = models[((slot0 + kn) * RPE_MAX_MODELS + (jn - s_first[kn])) * 9 + lane];
        }
        double E[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) E[e] = __shfl(e_cur, e);
        int cnt = 0;
        for (int i = lane; i < M; i += 64) {
            double2 a = sp1[i], b = sp2[i];
            cnt += sampson_inlier_fast(E, a.x, a.y, b.x, b.y, thr2, sbound);
        }
        cnt = wave_sum(cnt);                             // DPP row shifts + v_readlane: 8 instructions instead of 6 ds_bpermute rounds
        if (lane == 0) counts[(slot0 + k) * RPE_MAX_MODELS + m] = cnt;
    }
}

// Replay of OpenCV's sequential update rule (ptsetreg.cpp) over the counts of one chunk: "strictly
// more inliers wins", niters shrinks through RANSACUpdateNumIters, the loop stops at niters.
// RANSACUpdateNumIters(.., niters) == min(niters, R(good)) with R tabulated on the host (0 when the
// log underflows, unbounded when denom >= 0), so the serial recurrence is a pair of scans: one wave per
// pair, lane = iteration, 64 iterations per step: exclusive prefix max of the per-iteration best count
// (who is a record breaker), per-lane replay of its <= 10 models against that prefix, exclusive prefix
// min of the resulting niters, first lane whose iteration index reaches its niters = the break.
// Bit-identical to the serial loop (it was 0.25-1.1 ms of single-lane latency per step).
__global__ __launch_bounds__(256) void ransac_update_kernel(RpeRansacState *__restrict__ st, const double *__restrict__ models,
                                                            const int *__restrict__ nmodels, const int *__restrict__ counts,
                                                            const double *__restrict__ nit_denom, const int *__restrict__ nit_round,
                                                            double nit_num, double *__restrict__ E_out, int *__restrict__ found,
                                                            int chunk, int n_pairs)
{
    const int lane = threadIdx.x & 63, pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;
    RpeRansacState s = st[pair];
    if (s.done) return;                                   // wave-uniform
    const int M = s.M;
    const long long slot0 = (long long)pair * RPE_RANSAC_MAXCHUNK;
    int best = s.best_count, niters = s.niters, bk = -1, bm = -1;
    int nstack = 0;
    if (M == 5) {
        // ptsetreg.cpp: count == modelPoints -> runKernel on all points; cv2 returns EVERY model stacked (3n x 3).
        // One model = a usable E; more than one is reported (found = n) and becomes RPE_PAIR_AMBIGUOUS_ESSENTIAL
        // (the reference's recoverPose call then fails its 3x3 assertion, pose_estimator.py:533); E keeps the first.
        nstack = nmodels[slot0];
        if (nstack > 0) { best = 5; bk = 0; bm = 0; s.best_iter = 0; s.best_model = 0; }
        niters = 1;
        s.next_iter = 1;
        s.iters_run = 1;
    } else {
        const int kmax = min(chunk, s.niters - s.next_iter);
        bool stopped = false;
        for (int k0 = 0; k0 < kmax && !stopped; k0 += 64) {
            const int k = k0 + lane, it = s.next_iter + k;
            const bool act = k < kmax;
            const int nm = act ? nmodels[slot0 + k] : 0;
            int c[RPE_MAX_MODELS];
            int cmax = 0;
#pragma unroll
            for (int m = 0; m < RPE_MAX_MODELS; ++m) {
                c[m] = (m < nm) ? counts[(slot0 + k) * RPE_MAX_MODELS + m] : 0;
                if (c[m] > 4) cmax = max(cmax, c[m]);          // a model needs > max(best, 4) inliers to count
            }
            // exclusive prefix max over the lanes (iterations), seeded with the incoming best
            const int inc = wave_inclusive_max(cmax);
            int pre = __shfl_up(inc, 1);
            if (lane == 0) pre = 0;
            pre = max(pre, best);
            // this lane's models against its prefix: local record breakers shrink niters
            int run = pre, lmin = 0x7FFFFFFF, wm = -1;
#pragma unroll
            for (int m = 0; m < RPE_MAX_MODELS; ++m) {
                if (m < nm && c[m] > max(run, 4)) {
                    run = c[m]; wm = m;
                    lmin = min(lmin, update_niters(nit_denom, nit_round, nit_num, M, c[m], 0x7FFFFFFF));
                }
            }
            // exclusive prefix min of niters
            const int pmin = wave_inclusive_min(lmin);
            int nit_before = __shfl_up(pmin, 1);
            if (lane == 0) nit_before = 0x7FFFFFFF;
            nit_before = min(nit_before, niters);
            const unsigned long long brk = __ballot(!act || it >= nit_before);
            const int stop = brk ? (__ffsll((long long)brk) - 1) : 64;       // lanes [0, stop) are processed
            if (stop > 0) {
                // state after the last processed lane
                const int last = stop - 1;
                const int nbest = __shfl(run, last);
                const int nnit = min(niters, __shfl(pmin, last));
                if (nbest > best) {
                    // the winner is the first processed lane whose run reached nbest (first occurrence of the max)
                    const unsigned long long wmask = __ballot(lane < stop && run == nbest && wm >= 0);
                    const int wl = __ffsll((long long)wmask) - 1;
                    bk = k0 + wl; bm = __shfl(wm, wl);
                    s.best_iter = s.next_iter + bk; s.best_model = bm;
                    best = nbest;
                }
                niters = nnit;
                s.iters_run = s.next_iter + k0 + stop;
            }
            if (stop < 64) stopped = true;
        }
        s.next_iter += chunk;
    }
    if (bk >= 0 && lane < 9) {
        const double *Eg = models + ((slot0 + bk) * RPE_MAX_MODELS + bm) * 9;
        const double e = Eg[lane];
        E_out[pair * 9 + lane] = e;
        st[pair].E[lane] = e;
    }
    if (lane == 0) {
        RpeRansacState *d = st + pair;
        d->best_count = best; d->niters = niters; d->best_iter = s.best_iter; d->best_model = s.best_model;
        d->next_iter = s.next_iter; d->iters_run = s.iters_run;
        const int fnd = (M == 5) ? nstack : (best > 0 ? 1 : 0);
        d->found = fnd;
        d->done = s.next_iter >= niters;
        found[pair] = fnd;
    }
}

// ------------------------------------------------------------------- mask
// status (may be null): pairs of a batch whose status is not RPE_PAIR_OK get an all-zero mask
template <bool CAM>
__global__ __launch_bounds__(256) void ransac_mask_kernel(const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                           const RpeRansacState *__restrict__ st, const double *__restrict__ K,
                                                           const RpeCamSrc cam, double threshold, const int *__restrict__ status,
                                                           uint8_t *__restrict__ mask, int max_matches)
{
    const int pair = blockIdx.x, tid = threadIdx.x;
    const RpeRansacState s = st[pair];
    const double thr = threshold / rpe_pair_focal<CAM>(K, cam, pair);
    const float thr2 = (float)(thr * thr);
    const bool ok = !status || status[pair] == RPE_PAIR_OK;
    for (int i = tid; i < max_matches; i += 256) {
        uint8_t v = 0;
        if (ok && i < s.M && s.found) {
            if (s.M == 5) v = 1;
            else {
                double2 a = n1[(long long)pair * max_matches + i], b = n2[(long long)pair * max_matches + i];
                v = (uint8_t)sampson_inlier(s.E, a.x, a.y, b.x, b.y, thr2);
            }
        }
        mask[(long long)pair * max_matches + i] = v;
    }
}

static void launch_mask(rpe_handle *h, const RpeRun &r, const int *status)
{
    launch_cam(r, ransac_mask_kernel<true>, ransac_mask_kernel<false>, dim3(r.pairs), dim3(256), 0, h->stream,
               h->d_n1, h->d_n2, h->d_rstate, h->d_K, r.cam, h->cfg.ransac_threshold, status, h->d_mask, h->cfg.max_matches);
}

// stage forms that run no RANSAC (recoverPose, the refinement over uploaded points): d_n1 / d_n2 of the uploaded points
void rpe_launch_normalise(rpe_handle *h, const RpeRun &r)
{
    const int mm = h->cfg.max_matches;
    launch_cam(r, normalise_kernel<true>, normalise_kernel<false>, dim3((mm + 255) / 256, r.pairs), dim3(256), 0, h->stream,
               h->d_pts1, h->d_pts2, h->d_m_n, h->d_K, r.cam, h->d_n1, h->d_n2, mm);
}

void rpe_launch_ransac(rpe_handle *h, const RpeRun &r, bool want_mask)
{
    const int mm = h->cfg.max_matches, it = h->cfg.ransac_max_iters, B = r.pairs;
    double2 *n1 = h->d_n1, *n2 = h->d_n2;
    launch_cam(r, ransac_prepare_kernel<true>, ransac_prepare_kernel<false>, dim3((mm + 255) / 256, B), dim3(256), 0, h->stream,
               h->d_pts1, h->d_pts2, h->d_m_n, h->d_K, r.cam, n1, n2, h->d_rstate, h->d_found, mm, it);
    // chunk schedule 32, 96, 384, 512, 512, ... (cumulative 32, 128, 512, 1024).  A launch group costs
    //   max(latency floor, work): the floor is one wave's dependent chain through poly -> roots -> score -> update
    //   (~170-200 us whatever the number of pairs still running), the work is ~12.6 ns per (pair, iteration) that is
    //   still below its pair's current niters (r02 trace: 414 us for 1024 pairs x 32 iterations).
    // RANSACUpdateNumIters ends most pairs early (inlier ratio 0.72 -> 32 iterations, 0.64 -> 64), so the first group is
    // small (its whole chunk is evaluated for every pair); after it the launches are floor-bound and every extra group
    // costs a floor, so the chunks grow fast.  Measured on the 1024-pair bench batch (same box, interleaved):
    //   64,64,128,256,512: 1.58 ms   32,32,64,128,256,512: 1.43   32,32,64,384,512: 1.29   32,96,384,512: 1.20
    //   32,480,512: 1.23   64,448,512: 1.26   96,416,512: 1.40   (results identical: the replay in ransac_update_kernel
    //   is exact for any chunking).
    constexpr int lds_matches = 2048;
    static_assert(sizeof(double2) * 2 * lds_matches <= RPE_LDS_DEFAULT_BYTES, "the points of the cut fit the default dynamic LDS");
    const int use_lds = mm <= lds_matches;
    const size_t lds = use_lds ? sizeof(double2) * 2 * (size_t)mm : 0;
    static_assert(RPE_RANSAC_FIRST_CHUNK % POLY_LANES == 0 && RPE_RANSAC_FIRST_CHUNK % SCORE_GROUP == 0 && (RPE_RANSAC_FIRST_CHUNK * RG) % 256 == 0, "chunk granularity");
    static const int kSchedule[] = {RPE_RANSAC_FIRST_CHUNK, 96, 384, RPE_RANSAC_MAXCHUNK};      // the last entry repeats
    int done_iters = 0, chunk = kSchedule[0], nlaunch = 0;
    while (done_iters < it) {
        hipLaunchKernelGGL(ransac_poly_kernel, dim3(B, chunk / POLY_LANES), dim3(POLY_LANES), 0, h->stream,
                           n1, n2, h->d_rstate, h->d_subsets, h->d_hyp, h->d_nmodels, mm, it);
        hipLaunchKernelGGL(ransac_roots_kernel, dim3((unsigned)((long long)B * chunk * RG / 256)), dim3(256), 0, h->stream,
                           (const RpeRansacState *)h->d_rstate, (const double *)h->d_hyp, h->d_models, h->d_nmodels, B, chunk);
        launch_cam(r, ransac_score_kernel<true>, ransac_score_kernel<false>, dim3(B, chunk / SCORE_GROUP), dim3(256), lds, h->stream,
                   n1, n2, (const RpeRansacState *)h->d_rstate, (const double *)h->d_models, (const int *)h->d_nmodels,
                   (const double *)h->d_K, r.cam, h->cfg.ransac_threshold, h->d_counts, mm, use_lds);
        hipLaunchKernelGGL(ransac_update_kernel, dim3((B + 3) / 4), dim3(256), 0, h->stream,
                           h->d_rstate, (const double *)h->d_models, (const int *)h->d_nmodels, (const int *)h->d_counts,
                           (const double *)h->d_nit_denom, (const int *)h->d_nit_round, h->nit_num, h->d_E, h->d_found, chunk, B);
        done_iters += chunk;
        ++nlaunch;
        chunk = kSchedule[std::min(nlaunch, 3)];
    }
    if (want_mask) launch_mask(h, r, (const int *)nullptr);
}

// ------------------------------------------------------------ recoverPose
// jacobi_cols, triangulate_one and triangulate_pm: pose_triangulate.h (shared with the host test of the -t mirror)
__device__ __forceinline__ double det3(const double *m)
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// decomposeEssentialMat (five-point.cpp)
__device__ static void decompose_essential(const double *E, double *R1, double *R2, double *t)
{
    double A[9], V[9];
    for (int i = 0; i < 9; ++i) A[i] = E[i];
    jacobi_cols<3, 3>(A, V);
    double sv[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) sv[j] = sqrt((A[j] * A[j] + A[3 + j] * A[3 + j]) + A[6 + j] * A[6 + j]);
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2 - i; ++j)
        if (sv[ord[j]] < sv[ord[j + 1]]) { int tt = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = tt; }
    double U[9], Vt[9];
    for (int c = 0; c < 2; ++c) {
        int j = ord[c];
        double s = sv[j] > 0. ? 1. / sv[j] : 0.;
        for (int r = 0; r < 3; ++r) U[r * 3 + c] = A[r * 3 + j] * s;
    }
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) Vt[c * 3 + r] = V[r * 3 + ord[c]];
    if (det3(U) < 0) for (int i = 0; i < 9; ++i) U[i] = -U[i];
    if (det3(Vt) < 0) for (int i = 0; i < 9; ++i) Vt[i] = -Vt[i];
    double UW[9], UWt[9];
    for (int r = 0; r < 3; ++r) {
        UW[r * 3 + 0] = -U[r * 3 + 1]; UW[r * 3 + 1] = U[r * 3 + 0]; UW[r * 3 + 2] = U[r * 3 + 2];
        UWt[r * 3 + 0] = U[r * 3 + 1]; UWt[r * 3 + 1] = -U[r * 3 + 0]; UWt[r * 3 + 2] = U[r * 3 + 2];
    }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) {
        R1[r * 3 + c] = (UW[r * 3] * Vt[c] + UW[r * 3 + 1] * Vt[3 + c]) + UW[r * 3 + 2] * Vt[6 + c];
        R2[r * 3 + c] = (UWt[r * 3] * Vt[c] + UWt[r * 3 + 1] * Vt[3 + c]) + UWt[r * 3 + 2] * Vt[6 + c];
    }
    t[0] = U[2]; t[1] = U[5]; t[2] = U[8];
}

// The normalised coordinates of match o for recover_pose_kernel and pose_structure_kernel.  CAM = true: read from
// d_n1 / d_n2, the normalised and undistorted coordinates the RANSAC of the same call worked on (or normalise_kernel's,
// stage form); CAM = false: normalised again with K, the same expression and so the same bits as d_n1 / d_n2 (reading
// those here too did not pass the timing check of DESIGN section 4, round 8).
template <bool CAM>
__device__ __forceinline__ void pose_match(const RpePairNormalise<false> &with_K, const float2 *__restrict__ pts1,
                                           const float2 *__restrict__ pts2, const double2 *__restrict__ n1,
                                           const double2 *__restrict__ n2, long long o, double2 &a, double2 &b)
{
    if (CAM) { a = n1[o]; b = n2[o]; }
    else with_K(pts1[o], pts2[o], a, b);
}

template <bool TAB, bool CAM>
__global__ __launch_bounds__(256) void recover_pose_kernel(const double *__restrict__ Eall, const float2 *__restrict__ pts1,
                                                            const float2 *__restrict__ pts2, const double2 *__restrict__ n1,
                                                            const double2 *__restrict__ n2, const int *__restrict__ m_n,
                                                            const int *__restrict__ found, const int *__restrict__ kp_count,
                                                            int img2_base, const int2 *__restrict__ pair_tab, const double *__restrict__ K,
                                                            double *__restrict__ Rout, double *__restrict__ tout,
                                                            int *__restrict__ inliers, int *__restrict__ status, int max_matches)
{
    __shared__ int s_g[4];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int M = min(m_n[pair], max_matches);
    int stt = RPE_PAIR_OK;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    if (kp_count && (kp_count[img1] == 0 || kp_count[img2] == 0)) stt = RPE_PAIR_NO_DESCRIPTORS;
    else if (M < 5) stt = RPE_PAIR_INSUFFICIENT_MATCHES;
    else if (found && !found[pair]) stt = RPE_PAIR_NO_ESSENTIAL;
    else if (found && found[pair] > 1) stt = RPE_PAIR_AMBIGUOUS_ESSENTIAL;
    if (stt != RPE_PAIR_OK) {
        if (tid < 9) Rout[pair * 9 + tid] = (tid % 4 == 0) ? 1. : 0.;
        if (tid < 3) tout[pair * 3 + tid] = 0.;
        if (tid == 0) { inliers[pair] = 0; if (status) status[pair] = stt; }
        return;
    }
    if (tid < 4) s_g[tid] = 0;
    __syncthreads();
    double E[9], R1[9], R2[9], tt[3], tn[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = Eall[pair * 9 + e];
    decompose_essential(E, R1, R2, tt);
    tn[0] = -tt[0]; tn[1] = -tt[1]; tn[2] = -tt[2];
    const RpePairNormalise<false> with_K(K, RpeCamSrc{}, pair);
    int g1 = 0, g2 = 0, g3 = 0, g4 = 0;
    // one SVD per rotation: the verdict of (R, -t) is the mirror of (R, t)'s (pose_triangulate.h)
    for (int i = tid; i < M; i += 256) {
        double2 a, b;
        pose_match<CAM>(with_K, pts1, pts2, n1, n2, (long long)pair * max_matches + i, a, b);
        double P[3];
        int gp, gm;
        triangulate_pm(R1, tt, a.x, a.y, b.x, b.y, gp, gm, P);
        g1 += gp; g3 += gm;
        triangulate_pm(R2, tt, a.x, a.y, b.x, b.y, gp, gm, P);
        g2 += gp; g4 += gm;
    }
    g1 = wave_sum(g1); g2 = wave_sum(g2); g3 = wave_sum(g3); g4 = wave_sum(g4);
    if ((tid & 63) == 0) { atomicAdd(&s_g[0], g1); atomicAdd(&s_g[1], g2); atomicAdd(&s_g[2], g3); atomicAdd(&s_g[3], g4); }
    __syncthreads();
    if (tid == 0) {
        g1 = s_g[0]; g2 = s_g[1]; g3 = s_g[2]; g4 = s_g[3];
        const double *Rs, *ts; int g;
        if (g1 >= g2 && g1 >= g3 && g1 >= g4)      { Rs = R1; ts = tt; g = g1; }
        else if (g2 >= g1 && g2 >= g3 && g2 >= g4) { Rs = R2; ts = tt; g = g2; }
        else if (g3 >= g1 && g3 >= g2 && g3 >= g4) { Rs = R1; ts = tn; g = g3; }
        else                                        { Rs = R2; ts = tn; g = g4; }
        for (int e = 0; e < 9; ++e) Rout[pair * 9 + e] = Rs[e];
        for (int e = 0; e < 3; ++e) tout[pair * 3 + e] = ts[e];
        inliers[pair] = g;
        if (status) status[pair] = RPE_PAIR_OK;
    }
}

// Per-match results of the pose recover_pose_kernel returned (recoverPose's mask and triangulatedPoints, distanceThresh
// 50): one block per pair, one candidate per match.  Entries past the pair's match count and every entry of a pair whose
// status is not OK are zero.
template <bool CAM>
__global__ __launch_bounds__(256) void pose_structure_kernel(const float2 *__restrict__ pts1, const float2 *__restrict__ pts2,
                                                              const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                              const int *__restrict__ m_n, const int *__restrict__ status,
                                                              const double *__restrict__ K, const double *__restrict__ Rall,
                                                              const double *__restrict__ tall, uint8_t *__restrict__ pose_mask,
                                                              double *__restrict__ points, int max_matches)
{
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int M = status[pair] == RPE_PAIR_OK ? min(m_n[pair], max_matches) : 0;
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rall[pair * 9 + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = tall[pair * 3 + e];
    const RpePairNormalise<false> with_K(K, RpeCamSrc{}, pair);
    for (int i = tid; i < max_matches; i += 256) {
        const long long o = (long long)pair * max_matches + i;
        double P[3] = {0., 0., 0.};
        int g = 0;
        if (i < M) {
            double2 a, b;
            pose_match<CAM>(with_K, pts1, pts2, n1, n2, o, a, b);
            g = triangulate_one(R, t, a.x, a.y, b.x, b.y, P);
        }
        pose_mask[o] = (uint8_t)g;
        points[o * 3] = P[0]; points[o * 3 + 1] = P[1]; points[o * 3 + 2] = P[2];
    }
}

// Only rpe_fetch_structure launches these, after a batch: d_n1 / d_n2 / d_rstate still hold the batch's normalised points
// and RANSAC state, d_R / d_t / d_status its results.
void rpe_launch_structure(rpe_handle *h, const RpeRun &r)
{
    launch_mask(h, r, (const int *)h->d_status);
    launch_cam(r, pose_structure_kernel<true>, pose_structure_kernel<false>, dim3(r.pairs), dim3(256), 0, h->stream,
               h->d_pts1, h->d_pts2, h->d_n1, h->d_n2, h->d_m_n, h->d_status, h->d_K, h->d_R, h->d_t, h->d_pose_mask, h->d_points, h->cfg.max_matches);
}

// fused (a batch, a stream, a pair list): the status test reads ransac's d_found and the keypoint counts of the pair's two
// images, through the pair table when the run has one.  Stage form: neither, and the rule instances.
void rpe_launch_pose(rpe_handle *h, const RpeRun &r, bool fused)
{
    const RpeFeatSrc &f = r.feat;
    const bool tab = fused && f.tab;
    // the camera instances read d_n1 / d_n2: ransac_prepare_kernel<true> (fused) or rpe_launch_normalise (stage form) of
    // the same call has filled them
    launch_cam(r, tab ? recover_pose_kernel<true, true> : recover_pose_kernel<false, true>,
               tab ? recover_pose_kernel<true, false> : recover_pose_kernel<false, false>, dim3(r.pairs), dim3(256), 0, h->stream,
               h->d_E, h->d_pts1, h->d_pts2, h->d_n1, h->d_n2, h->d_m_n, fused ? (const int *)h->d_found : (const int *)nullptr,
               fused ? f.count : (const int *)nullptr, f.img2_base, tab ? f.tab : (const int2 *)nullptr, h->d_K,
               h->d_R, h->d_t, h->d_inliers, h->d_status, h->cfg.max_matches);
}

// ------------------------------------------------------------ pose refinement
// rpe_refine_poses / rpe_refine_pose_points (NOT in the reference): Levenberg-Marquardt on the essential manifold over
// findEssentialMat's inliers, started from recoverPose's (R, t).  One 256-thread workgroup per pair, f64 throughout.
//   parameters  R <- exp([w]x) R (Rodrigues), t <- normalise(t + a b1 + b b2), (b1, b2) = tangent basis of the sphere at t
//   residual    signed Sampson distance of E = [t]x R in pixels (scale (fx + fy) / 2, as the RANSAC threshold)
//   step        refine_lm<5>: (J'J + lambda diag(J'J)) d = -J'r by 5x5 Cholesky (every lane, identical operands), trial
//               cost in a second pass, accepted only on a strict decrease (lambda / 10), rejected otherwise (lambda * 10)
//   sums        lane partials in strided order -> xor butterfly inside the wave -> the four waves added in wave order
//               through LDS: no floating-point atomics, bit-deterministic
//   points      the inliers are compacted in match order once: into LDS (max_matches <= REFINE_LDS_MATCHES: 32 B per
//               match, 64 KB at the cut, two workgroups per CU) or, above the cut, as 16-bit indices into d_n1 / d_n2
//               (both forms walk the same list in the same order: same sums)
//   fallback    the refined pose is returned only if it is finite and keeps at least the cheirality inliers of the
//               input pose (triangulate_one over all matches, as recover_pose_kernel counts them)
#define REFINE_MIN_RESIDUALS 6       // 5 degrees of freedom
#define REFINE_LDS_MATCHES 2048      // staging cut (max_matches)
#define REFINE_NSUM 21               // 15 J'J + 5 J'r + 1 r'r

// Sampson residual of one match in pixels; optionally its 5 derivatives (w0 w1 w2 | b1 b2)
template <bool JAC>
__device__ __forceinline__ double refine_residual(const double *R, const double *t, const double *b1, const double *b2, double scale,
                                                  double x1, double y1, double x2, double y2, double *J)
{
    double a[3], l[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = (R[3 * i] * x1 + R[3 * i + 1] * y1) + R[3 * i + 2];      // R x1
    cross3(t, a, l);                                                                              // E x1
    const double X2[3] = {x2, y2, 1.};
    cross3(X2, t, c);                                                                             // E' x2 = R' (x2 x t)
    const double m0 = (R[0] * c[0] + R[3] * c[1]) + R[6] * c[2], m1 = (R[1] * c[0] + R[4] * c[1]) + R[7] * c[2];
    const double C = (x2 * l[0] + y2 * l[1]) + l[2];
    const double D = ((l[0] * l[0] + l[1] * l[1]) + m0 * m0) + m1 * m1;
    const double inv = scale / sqrt(D);
    if (JAC) {
        const double rc0[3] = {R[0], R[3], R[6]}, rc1[3] = {R[1], R[4], R[7]};
        const double ta = (t[0] * a[0] + t[1] * a[1]) + t[2] * a[2], q = C / D;
        double dC[3], dm0[3], dm1[3];
        cross3(a, c, dC); cross3(rc0, c, dm0); cross3(rc1, c, dm1);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double dl0 = (j == 0 ? ta : 0.) - a[0] * t[j], dl1 = (j == 1 ? ta : 0.) - a[1] * t[j];
            const double g = ((l[0] * dl0 + l[1] * dl1) + m0 * dm0[j]) + m1 * dm1[j];
            J[j] = inv * (dC[j] - q * g);
        }
        double aX[3], r0X[3], r1X[3];
        cross3(a, X2, aX); cross3(rc0, X2, r0X); cross3(rc1, X2, r1X);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double b[3] = {k ? b2[0] : b1[0], k ? b2[1] : b1[1], k ? b2[2] : b1[2]};
            const double dCk = (b[0] * aX[0] + b[1] * aX[1]) + b[2] * aX[2];
            const double dl0 = b[1] * a[2] - b[2] * a[1], dl1 = b[2] * a[0] - b[0] * a[2];
            const double e0 = (b[0] * r0X[0] + b[1] * r0X[1]) + b[2] * r0X[2], e1 = (b[0] * r1X[0] + b[1] * r1X[1]) + b[2] * r1X[2];
            const double g = ((l[0] * dl0 + l[1] * dl1) + m0 * e0) + m1 * e1;
            J[3 + k] = inv * (dCk - q * g);
        }
    }
    return C * inv;
}

// status / inl_in may be null (stage form): every pair is then refined and the input pose's cheirality inliers are counted here
template <bool LDS, bool CAM>
__global__ __launch_bounds__(256) void pose_refine_kernel(const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                           const uint8_t *__restrict__ mask, const int *__restrict__ m_n,
                                                           const int *__restrict__ status, const int *__restrict__ inl_in,
                                                           const double *__restrict__ K, const RpeCamSrc cam, const double *__restrict__ Rin,
                                                           const double *__restrict__ tin, double *__restrict__ Rout,
                                                           double *__restrict__ tout, int *__restrict__ inl_out,
                                                           int *__restrict__ info, double *__restrict__ rms,
                                                           int max_matches, int max_iters)
{
    extern __shared__ double2 s_dyn[];            // LDS: [2][max_matches] compacted inlier points; else u16 [max_matches] inlier indices
    __shared__ double s_red[4 * REFINE_NSUM];
    __shared__ int s_wc[4], s_g[2];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int M = min(m_n[pair], max_matches);
    const bool st_ok = !status || status[pair] == RPE_PAIR_OK;
    const double2 *gp1 = n1 + (long long)pair * max_matches, *gp2 = n2 + (long long)pair * max_matches;
    const uint8_t *mk = mask + (long long)pair * max_matches;
    double2 *l1 = s_dyn, *l2 = s_dyn + max_matches;
    unsigned short *s_idx = (unsigned short *)s_dyn;
    if (tid < 2) s_g[tid] = 0;
    // ---- ordered compaction of the inliers
    int n = 0;
    for (int i0 = 0; i0 < (st_ok ? M : 0); i0 += 256) {
        const int i = i0 + tid;
        const bool f = i < M && mk[i] != 0;
        const int pos = ordered_slot(f, s_wc, n);
        if (f) {
            if (LDS) { l1[pos] = gp1[i]; l2[pos] = gp2[i]; }
            else s_idx[pos] = (unsigned short)i;
        }
    }
    __syncthreads();                                   // the list is complete
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rin[pair * 9 + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = tin[pair * 3 + e];
    const double scale = rpe_pair_focal<CAM>(K, cam, pair);
    auto fetch = [&](int j, double2 &a, double2 &b) {
        if (LDS) { a = l1[j]; b = l2[j]; }
        else { const int i = s_idx[j]; a = gp1[i]; b = gp2[i]; }
    };
    double s[REFINE_NSUM], b1[3], b2[3];
    double cost = 0., cost0 = 0.;
    int iters = 0, acc = 0;
    bool finite = true;
    // also leaves the tangent basis at t in (b1, b2) for the trial steps
    auto linearise = [&]() {
        refine_basis(t, b1, b2);
#pragma unroll
        for (int k = 0; k < REFINE_NSUM; ++k) s[k] = 0.;
        for (int j = tid; j < n; j += 256) {
            double2 a, b; fetch(j, a, b);
            double J[5];
            const double r = refine_residual<true>(R, t, b1, b2, scale, a.x, a.y, b.x, b.y, J);
            int q = 0;
#pragma unroll
            for (int u = 0; u < 5; ++u)
#pragma unroll
                for (int v = u; v < 5; ++v, ++q) s[q] += J[u] * J[v];
#pragma unroll
            for (int u = 0; u < 5; ++u) s[15 + u] += J[u] * r;
            s[20] += r * r;
        }
        block_sum_f64<REFINE_NSUM>(s, s_red, tid);
    };
    const bool skip = !st_ok || n < REFINE_MIN_RESIDUALS;
    // R <- exp([w]x) R, t <- normalise(t + d3 b1 + d4 b2)
    auto trial = [&](const double (&d)[5], double (&Rn)[9], double (&tn)[3]) {
        refine_rotate(d, R, Rn);
#pragma unroll
        for (int e = 0; e < 3; ++e) tn[e] = (t[e] + d[3] * b1[e]) + d[4] * b2[e];
        const double nt = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
        tn[0] /= nt; tn[1] /= nt; tn[2] /= nt;
        double c = 0.;
        for (int j = tid; j < n; j += 256) {
            double2 a, b; fetch(j, a, b);
            const double r = refine_residual<false>(Rn, tn, b1, b2, scale, a.x, a.y, b.x, b.y, nullptr);
            c += r * r;
        }
        return c;
    };
    if (n > 0) {
        linearise();
        cost = cost0 = s[20];
        finite = isfinite(cost0);
    }
    if (!skip && finite) {
        refine_lm<5>(R, t, cost, max_iters, s_red, linearise, RefineNormalSolve<5>{s}, trial, RefineNoCommit{}, iters, acc);
#pragma unroll
        for (int e = 0; e < 9; ++e) finite = finite && isfinite(R[e]);
#pragma unroll
        for (int e = 0; e < 3; ++e) finite = finite && isfinite(t[e]);
    }
    // ---- cheirality inliers over ALL matches: of the refined pose, and of the input pose where the caller has no count
    const bool moved = !skip && finite && acc > 0;
    const bool need_org = st_ok && inl_in == nullptr;
    if (moved || need_org) {
        double R0[9], t0[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) R0[e] = Rin[pair * 9 + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) t0[e] = tin[pair * 3 + e];
        int gr = 0, go = 0;
        for (int i = tid; i < M; i += 256) {
            const double2 a = gp1[i], b = gp2[i];
            double P[3];
            if (moved) gr += triangulate_one(R, t, a.x, a.y, b.x, b.y, P);
            if (need_org) go += triangulate_one(R0, t0, a.x, a.y, b.x, b.y, P);
        }
        gr = wave_sum(gr); go = wave_sum(go);
        __syncthreads();
        if (lane == 0) { atomicAdd(&s_g[0], gr); atomicAdd(&s_g[1], go); }
    }
    __syncthreads();
    const int g_org = inl_in ? inl_in[pair] : s_g[1];
    const int g_ref = moved ? s_g[0] : g_org;
    int code = RPE_REFINE_OK;
    if (skip) code = RPE_REFINE_SKIPPED;
    else if (!finite || g_ref < g_org) code = RPE_REFINE_REJECTED;
    const bool take = code == RPE_REFINE_OK && moved;
    if (tid < 9) Rout[pair * 9 + tid] = take ? R[tid] : Rin[pair * 9 + tid];
    if (tid < 3) tout[pair * 3 + tid] = take ? t[tid] : tin[pair * 3 + tid];
    if (tid == 0) {
        inl_out[pair] = take ? g_ref : g_org;
        info[pair * 4] = code; info[pair * 4 + 1] = iters; info[pair * 4 + 2] = n; info[pair * 4 + 3] = acc;
        const double before = n > 0 ? sqrt(cost0 / n) : 0.;
        rms[pair * 2] = before;
        rms[pair * 2 + 1] = take ? sqrt(cost / n) : before;
    }
}

// rpe_undistort_points: n pixels of one camera -> normalised, undistorted coordinates; one thread per point, the camera a
// uniform scalar load, one 16-byte store per point
__global__ __launch_bounds__(256) void undistort_points_kernel(const float2 *__restrict__ pts, int n, const rpe_camera *__restrict__ cam,
                                                                double2 *__restrict__ out)
{
    const bool lens = rpe_camera_has_lens(cam);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = rpe_camera_normalise(cam, lens, pts[i]);
}

void rpe_launch_undistort(rpe_handle *h, const float2 *d_pts, int n, const rpe_camera *d_cam, double2 *d_out)
{
    const int blocks = std::min((n + 255) / 256, 2048);
    hipLaunchKernelGGL(undistort_points_kernel, dim3(blocks), dim3(256), 0, h->stream, d_pts, n, d_cam, d_out);
}

// after a batch / stream (from_batch): inliers = ransac_mask_kernel's mask of the winning model, start = d_R / d_t.
// stage form: d_mask, ref.R0 / ref.t0 and d_pts* were uploaded by the caller.
void rpe_launch_refine(rpe_handle *h, const RpeRun &r, int max_iters, bool from_batch)
{
    const int mm = h->cfg.max_matches, B = r.pairs;
    if (from_batch) launch_mask(h, r, (const int *)h->d_status);
    else rpe_launch_normalise(h, r);
    const double *Rin = from_batch ? h->d_R : h->ref.R0, *tin = from_batch ? h->d_t : h->ref.t0;
    const int *status = from_batch ? h->d_status : nullptr, *inl = from_batch ? h->d_inliers : nullptr;
    // the inliers staged in LDS, or, above the cut, as 16-bit indices
    const bool lds = mm <= REFINE_LDS_MATCHES;
    static_assert(sizeof(double2) * 2 * REFINE_LDS_MATCHES <= RPE_LDS_DEFAULT_BYTES && sizeof(unsigned short) * RPE_MAX_MATCHES_LIMIT <= RPE_LDS_DEFAULT_BYTES,
                  "either form fits the default dynamic LDS");
    launch_cam(r, lds ? pose_refine_kernel<true, true> : pose_refine_kernel<false, true>,
               lds ? pose_refine_kernel<true, false> : pose_refine_kernel<false, false>, dim3(B), dim3(256),
               lds ? sizeof(double2) * 2 * (size_t)mm : sizeof(unsigned short) * (size_t)mm, h->stream,
               h->d_n1, h->d_n2, h->d_mask, h->d_m_n, status, inl, h->d_K, r.cam, Rin, tin,
               h->ref.R, h->ref.t, h->ref.inl, h->ref.info, h->ref.rms, mm, max_iters);
}

// ------------------------------------------------------------ homography / rotation-only
// rpe_pair_homographies / rpe_find_homography (NOT in the reference; include/rpe_amd.h states the rule): a homography by
// RANSAC over the first four indices of findEssentialMat's subset stream, the rotation fitted to its inliers, and the
// inlier count of that rotation.  One 256-thread workgroup per pair, f64 throughout, no contraction.
//   rounds   HG_ROUND = 256 samples at a time: thread j solves sample j in registers (closed form, static indexing, no
//            scratch) and parks H and G = adj(H), 18 doubles, in LDS; the four waves then score the round's valid models
//            round-robin (wave w: models w, w + 4, ...), lanes striding the matches, wave_sum for the count.  A wave meets
//            its models in ascending iteration order and replaces its best on a strictly larger count only, so its best
//            is its lowest iteration of that count; the cross-wave election (elect_best) compares (count, iteration).
//   points   the pair's normalised points in LDS behind the models, as ransac_score_kernel holds them
//            (max_matches <= HG_LDS_MATCHES: 32 B per match); read from d_n1 / d_n2 directly above the cut
//   winner   solved again by every thread from its sample (the same code on the same operands: the same bits), then the
//            mask, the bearing sums C (block_sum_f64: lane partials in strided order, xor butterfly, waves in wave
//            order), recoverPose's 3x3 Jacobi on every lane (identical operands), and n_rot
// Dynamic LDS (base 16-byte aligned): [HG_ROUND][18] f64 models = 36 KB, then [2][max_matches] double2 points: 52 KB at
// the default 500 matches, 100 KB at the cut (hg_lds_bytes; the most: rpe_geom_lds_ceilings).
#define HG_ROUND 256
#define HG_MODEL_DOUBLES 18
#define HG_LDS_MATCHES 2048
constexpr size_t hg_lds_bytes(int max_matches)
{
    return sizeof(double) * HG_ROUND * HG_MODEL_DOUBLES + (max_matches <= HG_LDS_MATCHES ? sizeof(double2) * 2 * (size_t)max_matches : 0);
}
static_assert(hg_lds_bytes(HG_LDS_MATCHES) <= RPE_CU_LDS_BYTES, "the models and the points of the cut fit a CU's LDS");

// adj(A), A row-major: rows cross(c1, c2), cross(c2, c0), cross(c0, c1) of A's columns
__device__ __forceinline__ void hg_adj(const double (&A)[9], double (&J)[9])
{
    const double c0[3] = {A[0], A[3], A[6]}, c1[3] = {A[1], A[4], A[7]}, c2[3] = {A[2], A[5], A[8]};
    double r0[3], r1[3], r2[3];
    hg_cross(c1, c2, r0); hg_cross(c2, c0, r1); hg_cross(c0, c1, r2);
    J[0] = r0[0]; J[1] = r0[1]; J[2] = r0[2]; J[3] = r1[0]; J[4] = r1[1]; J[5] = r1[2]; J[6] = r2[0]; J[7] = r2[1]; J[8] = r2[2];
}

// lambda of four points and the matrix with columns lambda_k * p_k; false when a lambda_k is 0
__device__ __forceinline__ bool hg_basis(const double2 (&s)[4], double (&A)[9])
{
    const double p0[3] = {s[0].x, s[0].y, 1.}, p1[3] = {s[1].x, s[1].y, 1.}, p2[3] = {s[2].x, s[2].y, 1.}, p3[3] = {s[3].x, s[3].y, 1.};
    double c[3];
    hg_cross(p1, p2, c); const double l0 = hg_dot(c, p3);
    hg_cross(p2, p0, c); const double l1 = hg_dot(c, p3);
    hg_cross(p0, p1, c); const double l2 = hg_dot(c, p3);
#pragma unroll
    for (int r = 0; r < 3; ++r) { A[r * 3] = l0 * p0[r]; A[r * 3 + 1] = l1 * p1[r]; A[r * 3 + 2] = l2 * p2[r]; }
    return l0 != 0. && l1 != 0. && l2 != 0.;
}

// the four-point model of the header: H (unit norm, gauged at p0), G = adj(H) (gauged at q0); returns its validity
__device__ __forceinline__ bool hg_four_point(const double2 (&p)[4], const double2 (&q)[4], double (&H)[9], double (&G)[9])
{
    double A[9], Bm[9], J[9];
    const bool okp = hg_basis(p, A), okq = hg_basis(q, Bm);
    bool ok = okp && okq;
    hg_adj(A, J);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r * 3 + c] = (Bm[r * 3] * J[c] + Bm[r * 3 + 1] * J[3 + c]) + Bm[r * 3 + 2] * J[6 + c];
    double ss = H[0] * H[0];
#pragma unroll
    for (int e = 1; e < 9; ++e) ss = ss + H[e] * H[e];
    const double n = sqrt(ss);
#pragma unroll
    for (int e = 0; e < 9; ++e) { H[e] = H[e] / n; ok = ok && hg_finite(H[e]); }
    if ((H[6] * p[0].x + H[7] * p[0].y) + H[8] < 0.) {
#pragma unroll
        for (int e = 0; e < 9; ++e) H[e] = -H[e];
    }
    hg_adj(H, G);
    if ((G[6] * q[0].x + G[7] * q[0].y) + G[8] < 0.) {
#pragma unroll
        for (int e = 0; e < 9; ++e) G[e] = -G[e];
    }
    return ok;
}

// T(F, p -> q) of the header
__device__ __forceinline__ bool hg_transfer(const double (&F)[9], double x, double y, double qx, double qy, double thr2)
{
    const double u = (F[0] * x + F[1] * y) + F[2], v = (F[3] * x + F[4] * y) + F[5], w = (F[6] * x + F[7] * y) + F[8];
    const double dx = u - qx * w, dy = v - qy * w;
    return w > 0. && (dx * dx + dy * dy) <= thr2 * (w * w);
}

__device__ __forceinline__ void hg_sample(const unsigned short *__restrict__ sub, int it, const double2 *sp1, const double2 *sp2,
                                          double2 (&p)[4], double2 (&q)[4])
{
    const unsigned short *s5 = sub + (long long)it * 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int v = s5[k]; p[k] = sp1[v]; q[k] = sp2[v]; }
}

__device__ __forceinline__ void hg_swap3(double (&a)[3], double (&b)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double t = a[k]; a[k] = b[k]; b[k] = t; }
}

// R_rot of the header from C = sum b^ a^T; false when an entry is not finite
__device__ __forceinline__ bool hg_rotation_fit(const double (&C)[9], double (&R)[9])
{
    double A[9], V[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) A[e] = C[e];
    jacobi_cols<3, 3>(A, V);                         // A = C V = U S, column by column
    double u0[3] = {A[0], A[3], A[6]}, u1[3] = {A[1], A[4], A[7]}, u2[3] = {A[2], A[5], A[8]};
    double v0[3] = {V[0], V[3], V[6]}, v1[3] = {V[1], V[4], V[7]}, v2[3] = {V[2], V[5], V[8]};
    double s0 = sqrt((u0[0] * u0[0] + u0[1] * u0[1]) + u0[2] * u0[2]);
    double s1 = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    double s2 = sqrt((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]);
    // descending: compare-and-swap (0, 1), (1, 2), (0, 1)
    if (s0 < s1) { const double t = s0; s0 = s1; s1 = t; hg_swap3(u0, u1); hg_swap3(v0, v1); }
    if (s1 < s2) { const double t = s1; s1 = s2; s2 = t; hg_swap3(u1, u2); hg_swap3(v1, v2); }
    if (s0 < s1) { const double t = s0; s0 = s1; s1 = t; hg_swap3(u0, u1); hg_swap3(v0, v1); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { u0[k] = u0[k] / s0; u1[k] = u1[k] / s1; }
    hg_cross(u0, u1, u2);
    const double Vt[9] = {v0[0], v0[1], v0[2], v1[0], v1[1], v1[2], v2[0], v2[1], v2[2]};
    const double d = det3(Vt) < 0. ? -1. : 1.;
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R[r * 3 + c] = (u0[r] * v0[c] + u1[r] * v1[c]) + (d * u2[r]) * v2[c];
            fin = fin && hg_finite(R[r * 3 + c]);
        }
    return fin;
}

// status (batch form; null in the stage form): a pair whose status is not RPE_PAIR_OK is skipped.  rstate (batch form; null
// in the stage form): the run's RANSAC state, whose best_count is n_E.
template <bool CAM>
__global__ __launch_bounds__(256) void homography_kernel(const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                          const int *__restrict__ m_n, const int *__restrict__ status,
                                                          const RpeRansacState *__restrict__ rstate,
                                                          const unsigned short *__restrict__ subsets, const double *__restrict__ K,
                                                          const RpeCamSrc cam, double threshold_px, int iters, int max_iters,
                                                          int max_matches, int use_lds, double *__restrict__ Hout,
                                                          double *__restrict__ Rout, uint8_t *__restrict__ mask,
                                                          int *__restrict__ counts, int *__restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_hg[];
    double *s_model = (double *)s_hg;                                                        // [HG_ROUND][18]
    double2 *s_pts = (double2 *)(s_hg + sizeof(double) * HG_ROUND * HG_MODEL_DOUBLES);       // [2][max_matches] when use_lds
    __shared__ int s_ok[HG_ROUND], s_best[8], s_cnt[4], s_nvalid;
    __shared__ double s_red[4 * 9];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int M = min(m_n[pair], max_matches);
    const bool pair_ok = !status || status[pair] == RPE_PAIR_OK;
    const int nE = rstate ? (pair_ok ? rstate[pair].best_count : 0) : -1;
    const long long o = (long long)pair * max_matches;
    int code = (!pair_ok || M < 6) ? RPE_HOMOGRAPHY_SKIPPED : RPE_HOMOGRAPHY_OK;
    int win_cnt = -1, win_it = -1, nvalid_all = 0;
    const double2 *sp1 = n1 + o, *sp2 = n2 + o;
    double thr2 = 0.;
    if (code == RPE_HOMOGRAPHY_OK) {                         // workgroup-uniform
        if (use_lds) {
            double2 *l1 = s_pts, *l2 = s_pts + max_matches;
            for (int i = tid; i < M; i += 256) { l1[i] = sp1[i]; l2[i] = sp2[i]; }
            sp1 = l1; sp2 = l2;
        }
        if (tid == 0) s_nvalid = 0;
        const double thr = threshold_px / rpe_pair_focal<CAM>(K, cam, pair);
        thr2 = thr * thr;
        const unsigned short *sub = subsets + (long long)M * max_iters * 5;
        int best_cnt = -1, best_it = -1, nvalid = 0;
        for (int base = 0; base < iters; base += HG_ROUND) {
            const int nr = min(HG_ROUND, iters - base);
            __syncthreads();                                 // the points are staged; the previous round's models have been scored
            int ok = 0;
            if (tid < nr) {
                double2 p[4], q[4];
                double H[9], G[9];
                hg_sample(sub, base + tid, sp1, sp2, p, q);
                ok = hg_four_point(p, q, H, G);
                double *d = s_model + tid * HG_MODEL_DOUBLES;
#pragma unroll
                for (int e = 0; e < 9; ++e) { d[e] = H[e]; d[9 + e] = G[e]; }
            }
            s_ok[tid] = ok;
            nvalid += ok;
            __syncthreads();
            for (int j = wv; j < nr; j += 4) {
                if (!s_ok[j]) continue;                      // wave-uniform
                double H[9], G[9];
                const double *d = s_model + j * HG_MODEL_DOUBLES;
#pragma unroll
                for (int e = 0; e < 9; ++e) { H[e] = d[e]; G[e] = d[9 + e]; }
                int cnt = 0;
                for (int i = lane; i < M; i += 64) {
                    const double2 a = sp1[i], b = sp2[i];
                    cnt += (hg_transfer(H, a.x, a.y, b.x, b.y, thr2) && hg_transfer(G, b.x, b.y, a.x, a.y, thr2)) ? 1 : 0;
                }
                cnt = wave_sum(cnt);
                if (cnt > best_cnt) { best_cnt = cnt; best_it = base + j; }
            }
        }
        nvalid = wave_sum(nvalid);
        if (lane == 0) atomicAdd(&s_nvalid, nvalid);
        elect_best(best_cnt, best_it, s_best, win_cnt, win_it);
        nvalid_all = s_nvalid;
        if (win_it < 0) code = RPE_HOMOGRAPHY_NONE;
    }
    if (code != RPE_HOMOGRAPHY_OK) {
        for (int i = tid; i < max_matches; i += 256) mask[o + i] = 0;
        if (tid < 9) { Hout[pair * 9 + tid] = 0.; Rout[pair * 9 + tid] = 0.; }
        if (tid == 0) {
            counts[pair * 3] = 0; counts[pair * 3 + 1] = 0; counts[pair * 3 + 2] = nE;
            info[pair * 4] = code; info[pair * 4 + 1] = 0; info[pair * 4 + 2] = 0; info[pair * 4 + 3] = 0;
        }
        return;
    }
    // the winner again, on every thread
    double H[9], G[9];
    {
        double2 p[4], q[4];
        hg_sample(subsets + (long long)M * max_iters * 5, win_it, sp1, sp2, p, q);
        hg_four_point(p, q, H, G);
    }
    double C[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = 0.;
    for (int i = tid; i < max_matches; i += 256) {
        uint8_t v = 0;
        if (i < M) {
            const double2 a = sp1[i], b = sp2[i];
            if (hg_transfer(H, a.x, a.y, b.x, b.y, thr2) && hg_transfer(G, b.x, b.y, a.x, a.y, thr2)) {
                v = 1;
                const double na = sqrt((a.x * a.x + a.y * a.y) + 1), nb = sqrt((b.x * b.x + b.y * b.y) + 1);
                const double ah[3] = {a.x / na, a.y / na, 1 / na}, bh[3] = {b.x / nb, b.y / nb, 1 / nb};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[r * 3 + c] += bh[r] * ah[c];
            }
        }
        mask[o + i] = v;
    }
    block_sum_f64<9>(C, s_red, tid);
    double R[9];
    const bool fin = hg_rotation_fit(C, R);
    int nrot = 0;
    if (fin) {                                               // workgroup-uniform: every lane holds the same C
        const double Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
        for (int i = tid; i < M; i += 256) {
            const double2 a = sp1[i], b = sp2[i];
            nrot += (hg_transfer(R, a.x, a.y, b.x, b.y, thr2) && hg_transfer(Rt, b.x, b.y, a.x, a.y, thr2)) ? 1 : 0;
        }
    }
    nrot = block_count(nrot, s_cnt);
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) { Hout[pair * 9 + e] = H[e]; Rout[pair * 9 + e] = fin ? R[e] : 0.; }
        counts[pair * 3] = win_cnt; counts[pair * 3 + 1] = nrot; counts[pair * 3 + 2] = nE;
        info[pair * 4] = RPE_HOMOGRAPHY_OK; info[pair * 4 + 1] = win_it; info[pair * 4 + 2] = nvalid_all; info[pair * 4 + 3] = 0;
    }
}

// d_n1 / d_n2 (the run's, or rpe_launch_normalise's in the stage form) -> hg.*.  from_batch: the run's d_status and
// d_rstate gate the pairs and supply n_E.
void rpe_launch_homography(rpe_handle *h, const RpeRun &r, int iters, double threshold_px, bool from_batch)
{
    const int mm = h->cfg.max_matches;
    const int use_lds = mm <= HG_LDS_MATCHES;
    launch_cam(r, homography_kernel<true>, homography_kernel<false>, dim3(r.pairs), dim3(256), hg_lds_bytes(mm), h->stream,
               (const double2 *)h->d_n1, (const double2 *)h->d_n2, (const int *)h->d_m_n,
               from_batch ? (const int *)h->d_status : (const int *)nullptr,
               from_batch ? (const RpeRansacState *)h->d_rstate : (const RpeRansacState *)nullptr,
               (const unsigned short *)h->d_subsets, (const double *)h->d_K, r.cam, threshold_px, iters, h->cfg.ransac_max_iters,
               mm, use_lds, h->hg.H, h->hg.R, h->hg.mask, h->hg.counts, h->hg.info);
}

// The kernels of this file that launch above the default dynamic LDS.  ransac_score_kernel and pose_refine_kernel stay at
// it: both stage 32 B per match up to a cut of 2048 matches, exactly 64 KB (the static_asserts in their launchers).
std::vector<RpeLdsCeiling> rpe_geom_lds_ceilings()
{
    return {{(const void *)homography_kernel<true>, "homography_kernel<true>", hg_lds_bytes(HG_LDS_MATCHES)},
            {(const void *)homography_kernel<false>, "homography_kernel<false>", hg_lds_bytes(HG_LDS_MATCHES)}};
}
