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
#include <float.h>
#include <stdlib.h>
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

// Fixed Estrin scheme for degree <= 10 (dependency depth 7 instead of Horner's 20; the root finder is latency bound), the
// arithmetic of horner() in oracle/geom_oracle.c.  c is anything indexable: a register array (static indices: K is the
// level's degree) or an LDS row.  The oracle evaluates the full degree-10 scheme on coefficients zero-padded above the
// degree; here the terms whose coefficients are structurally zero (index > K) are omitted: they would only add exact
// zeros, so estrin<K> on a degree-K polynomial equals estrin<10> on its zero-padded row bit for bit.
template <int K, typename C>
__device__ __forceinline__ double estrin(const C &c, double x)
{
    const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    auto A = [&](int i) -> double {           // a_i = c[2i] + c[2i+1] x
        if (2 * i + 1 <= K) return c[2 * i] + c[2 * i + 1] * x;
        return (2 * i <= K) ? c[2 * i] : 0.;
    };
    double b0, b1 = 0., b2 = 0.;
    b0 = (2 <= K) ? A(0) + A(1) * x2 : A(0);
    if (4 <= K) b1 = (6 <= K) ? A(2) + A(3) * x2 : A(2);
    if (8 <= K) b2 = (10 <= K) ? A(4) + c[10] * x2 : A(4);
    double r = (4 <= K) ? b0 + b1 * x4 : b0;
    if (8 <= K) r = r + b2 * x8;
    return r;
}

// Safeguarded Newton on a bracket with a sign change (same code path as the oracle); p and dp evaluate the polynomial
// and its derivative.
template <typename P, typename DP>
__device__ __forceinline__ double refine_root(P p, DP dp, double a, double b, int sa)
{
    double xl = sa ? b : a, xh = sa ? a : b;
    double rts = 0.5 * (a + b);
    double dxold = fabs(b - a), dx = dxold;
    double f = p(rts), df = dp(rts);
    for (int it = 0; it < 100; ++it) {
        int bis = ((((rts - xh) * df - f) * ((rts - xl) * df - f)) > 0.0) || (fabs(2.0 * f) > fabs(dxold * df));
        double nr;
        dxold = dx;
        if (bis) { dx = 0.5 * (xh - xl); nr = xl + dx; }
        else { dx = f / df; nr = rts - dx; }
        if (nr == rts || fabs(nr - rts) <= 2.3e-13 * fabs(nr)) { rts = nr; break; }
        rts = nr;
        f = p(rts); df = dp(rts);
        if (f > 0.0) xh = rts; else xl = rts;
    }
    return rts;
}

// Root bound from binary exponents only (same integers on CPU and GPU): Fujiwara's |z| <= 2 max_i |a_{k-i}/a_k|^(1/i)
// with |a| < 2^(ilogb(a)+1): R = 2^(1 + max_i ceil((e_{k-i} - e_k + 1)/i)).  Cauchy's bound put the outer brackets
// orders of magnitude beyond the roots and the safeguarded Newton bisected its way back (oracle: root_bound()).
// K: the degree where it is a compile-time constant (the register path: the loop unrolls, p keeps static indices and
// the divisions by m are by constants), 0 where it is k at run time (the generic path).  The constant has to be a
// template argument: as a function argument it arrived, after inlining, too late for the unsigned form of the
// divisions: 121 more instructions over levels 2..10 and 0.5 % on the ransac stage.
template <int K, typename C>
__device__ __forceinline__ double root_bound(const C &p, int k_run = 0)
{
    const int k = K ? K : k_run;
    const int ek = ilogb(p[k]);
    int emax = -100000;
#pragma unroll
    for (int i = 0; i < k; ++i) {
        if (p[i] != 0.) {
            const int d = ilogb(p[i]) - ek + 1, m = k - i;
            const int q = d >= 0 ? (d + m - 1) / m : -((-d) / m);
            if (q > emax) emax = q;
        }
    }
    double R = emax == -100000 ? 1. : ldexp(1., emax + 1);
    if (!(R < 1e12)) R = 1e12;
    return R;
}

// One interval of a level (the oracle's loop body in poly_real_roots): clamp the bracket to the root bound, test the
// signs, refine.  p has degree K, dp = p'; both may be rows zero-padded to degree 10 (K = 10 then evaluates any level).
template <int K, typename C>
__device__ __forceinline__ bool bracket_root(const C &p, const C &dp, double a, double b, double R, bool active, double &root)
{
    if (a < -R) a = -R;
    if (b > R) b = R;
    if (!(active && a < b)) return false;
    const int sa = estrin<K>(p, a) > 0., sb = estrin<K>(p, b) > 0.;
    if (sa == sb) return false;
    root = refine_root([&](double x) { return estrin<K>(p, x); }, [&](double x) { return estrin<K - 1>(dp, x); }, a, b, sa);
    return true;
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

// Launches the camera instance of a kernel when the run carries a camera source, the shared-K instance otherwise (the
// single-K paths launch CAM = false only): the two instances share one signature
template <typename Kernel, typename... Args>
static void launch_cam(const RpeRun &r, Kernel with_cameras, Kernel with_K, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args)
{
    hipLaunchKernelGGL(r.cam.cams ? with_cameras : with_K, grid, block, lds, stream, args...);
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
    const int use_lds = mm <= 2048;
    const size_t lds = use_lds ? sizeof(double2) * 2 * (size_t)mm : 0;
    static_assert(RPE_RANSAC_FIRST_CHUNK % POLY_LANES == 0 && RPE_RANSAC_FIRST_CHUNK % SCORE_GROUP == 0 && (RPE_RANSAC_FIRST_CHUNK * RG) % 256 == 0, "chunk granularity");
    // experiment hook: RPE_RANSAC_SCHEDULE="32,96,384,512" replaces the chunk schedule (multiples of 32, <= 512; the last
    // entry repeats)
    static std::vector<int> env_sched = [] {
        std::vector<int> v;
        if (const char *e = getenv("RPE_RANSAC_SCHEDULE")) {
            for (const char *q = e; *q;) { const int c = atoi(q); if (c >= 32 && c <= RPE_RANSAC_MAXCHUNK && c % 32 == 0) v.push_back(c); while (*q && *q != ',') ++q; if (*q) ++q; }
        }
        return v;
    }();
    static const int kSchedule[] = {RPE_RANSAC_FIRST_CHUNK, 96, 384, RPE_RANSAC_MAXCHUNK};
    int done_iters = 0, chunk = env_sched.empty() ? kSchedule[0] : env_sched[0], nlaunch = 0;
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
        if (!env_sched.empty()) chunk = env_sched[std::min((size_t)nlaunch, env_sched.size() - 1)];
        else chunk = kSchedule[std::min(nlaunch, 3)];
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
#define REFINE_LAMBDA0 1e-3          // initial damping
#define REFINE_REL_TOL 1e-6          // stop when an accepted step lowers the cost by no more than this fraction
#define REFINE_STEP_TOL 1e-9         // ... or its 5-vector is no longer than this
#define REFINE_SMALL_ANGLE 1e-4      // Rodrigues: series for sin(th)/th and (1 - cos th)/th^2 below this angle
#define REFINE_MIN_RESIDUALS 6       // 5 degrees of freedom
#define REFINE_LDS_MATCHES 2048      // staging cut (max_matches)
#define REFINE_NSUM 21               // 15 J'J + 5 J'r + 1 r'r

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// all 256 threads return the same N totals: ((wave 0 + wave 1) + wave 2) + wave 3
template <int N>
__device__ __forceinline__ void block_sum_f64(double (&v)[N], double *s_red, int tid)
{
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum_f64(v[k]);
    __syncthreads();                                   // readers of the previous reduction are done
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_red[(tid >> 6) * N + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((s_red[k] + s_red[N + k]) + s_red[2 * N + k]) + s_red[3 * N + k];
}

// Ordered compaction, one step of 256 candidates in thread order: the slot of this thread's element when f is set (n + the
// number of flagged threads below it), and n advanced by the step's total.  All 256 threads call it (two barriers, both
// in front of the caller's store to the slot: a barrier follows the last step before anyone reads the list);
// ballot / popcount only, so the order never depends on timing.  s_wc: one LDS word per wave.
__device__ __forceinline__ int ordered_slot(bool f, int *s_wc /*[4]*/, int &n)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) s_wc[wv] = __popcll(bal);
    __syncthreads();
    int off = n, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int c = s_wc[w]; if (w < wv) off += c; tot += c; }
    n += tot;
    __syncthreads();
    return off + __popcll(bal & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

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

// tangent basis of the unit sphere at t: b1 = normalise(t x e_k), k = axis of smallest |t_k| (lowest on ties), b2 = t x b1
__device__ __forceinline__ void refine_basis(const double *t, double *b1, double *b2)
{
    int k = 0;                                       // static indices only
    double m = fabs(t[0]);
    if (fabs(t[1]) < m) { k = 1; m = fabs(t[1]); }
    if (fabs(t[2]) < m) k = 2;
    const double e[3] = {k == 0 ? 1. : 0., k == 1 ? 1. : 0., k == 2 ? 1. : 0.};
    cross3(t, e, b1);
    const double n = sqrt((b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2]);
    b1[0] /= n; b1[1] /= n; b1[2] /= n;
    cross3(t, b1, b2);
}

// Rn = exp([w]x) R
__device__ __forceinline__ void refine_rotate(const double *w, const double *R, double *Rn)
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
    double A, B;
    if (th < REFINE_SMALL_ANGLE) { A = 1. - th2 / 6.; B = 0.5 - th2 / 24.; }
    else { const double sh = sin(0.5 * th); A = sin(th) / th; B = 2. * (sh * sh) / th2; }
    // exp = I + A [w]x + B [w]x^2,  [w]x^2 = w w' - th2 I
    double X[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) X[i * 3 + j] = B * (w[i] * w[j]) + (i == j ? 1. - B * th2 : 0.);
    X[1] -= A * w[2]; X[2] += A * w[1];
    X[3] += A * w[2]; X[5] -= A * w[0];
    X[6] -= A * w[1]; X[7] += A * w[0];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = (X[i * 3] * R[j] + X[i * 3 + 1] * R[3 + j]) + X[i * 3 + 2] * R[6 + j];
}

// (H + lambda diag H) d = -g for N parameters, H given as its upper triangle (row-major, N (N + 1) / 2 entries); false when
// not positive definite
template <int N>
__device__ __forceinline__ bool refine_solve(const double *H, const double *g, double lambda, double *d)
{
    double L[N][N];
    int q = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j, ++q) { L[i][j] = H[q]; L[j][i] = H[q]; }
#pragma unroll
    for (int i = 0; i < N; ++i) L[i][i] = L[i][i] + lambda * L[i][i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.) || !isfinite(s)) ok = false;
        const double dj = sqrt(s);
        L[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / dj;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    return ok;
}

// The Levenberg-Marquardt loop over N parameters, shared by pose_refine_kernel, link_pose_kernel and bundle_kernel; all 256
// threads call it with identical operands.
//   linearise()        the normal equations at the caller's state, summed over the workgroup (block_sum_f64)
//   solve(lambda, d)   the damped step d from them; false when there is none (a matrix that is not positive definite).
//                      RefineNormalSolve is the plain form: s holds the upper triangle of J'J, then J'r, then r'r
//   trial(d, Rn, tn)   the pose (Rn, tn) that step d leads to from (R, t), and this thread's part of its cost
//   commit()           an accepted step: whatever state the caller keeps outside (R, t) moves with it
// A failed solve or a step that does not strictly lower the cost multiplies lambda by 10; an accepted step divides it by
// 10, moves (R, t, cost) and stops the loop when it lowered the cost by no more than REFINE_REL_TOL of it or is no longer
// than REFINE_STEP_TOL.  The state is linearised again only when another iteration follows an accepted step.  iters counts
// the iterations begun, acc the steps accepted.
template <int N>
struct RefineNormalSolve {
    const double *s;
    __device__ __forceinline__ bool operator()(double lambda, double (&d)[N]) const { return refine_solve<N>(s, s + N * (N + 1) / 2, lambda, d); }
};
struct RefineNoCommit { __device__ __forceinline__ void operator()() const {} };

template <int N, class Linearise, class Solve, class Trial, class Commit>
__device__ __forceinline__ void refine_lm(double (&R)[9], double (&t)[3], double &cost, int max_iters, double *s_red,
                                          Linearise linearise, Solve solve, Trial trial, Commit commit, int &iters, int &acc)
{
    double lambda = REFINE_LAMBDA0;
    bool need_lin = false;
    for (int it = 0; it < max_iters; ++it) {
        if (need_lin) { linearise(); need_lin = false; }
        ++iters;
        double d[N];
        if (!solve(lambda, d)) { lambda = lambda * 10.; continue; }
        double Rn[9], tn[3];
        double c1[1] = {trial(d, Rn, tn)};
        block_sum_f64<1>(c1, s_red, threadIdx.x);
        if (isfinite(c1[0]) && c1[0] < cost) {
            const double dec = cost - c1[0], prev = cost;
            double dn = d[0] * d[0];
#pragma unroll
            for (int k = 1; k < N; ++k) dn = dn + d[k] * d[k];
            dn = sqrt(dn);
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = Rn[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) t[e] = tn[e];
            commit();
            cost = c1[0]; lambda = lambda / 10.; ++acc; need_lin = true;
            if (dec <= REFINE_REL_TOL * prev || dn <= REFINE_STEP_TOL) break;
        } else {
            lambda = lambda * 10.;
        }
    }
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
// stage form: d_mask, d_ref_R0 / d_ref_t0 and d_pts* were uploaded by the caller.
void rpe_launch_refine(rpe_handle *h, const RpeRun &r, int max_iters, bool from_batch)
{
    const int mm = h->cfg.max_matches, B = r.pairs;
    if (from_batch) launch_mask(h, r, (const int *)h->d_status);
    else rpe_launch_normalise(h, r);
    const double *Rin = from_batch ? h->d_R : h->d_ref_R0, *tin = from_batch ? h->d_t : h->d_ref_t0;
    const int *status = from_batch ? h->d_status : nullptr, *inl = from_batch ? h->d_inliers : nullptr;
    // the inliers staged in LDS, or, above the cut, as 16-bit indices
    const bool lds = mm <= REFINE_LDS_MATCHES;
    launch_cam(r, lds ? pose_refine_kernel<true, true> : pose_refine_kernel<false, true>,
               lds ? pose_refine_kernel<true, false> : pose_refine_kernel<false, false>, dim3(B), dim3(256),
               lds ? sizeof(double2) * 2 * (size_t)mm : sizeof(unsigned short) * (size_t)mm, h->stream,
               h->d_n1, h->d_n2, h->d_mask, h->d_m_n, status, inl, h->d_K, r.cam, Rin, tin,
               h->d_ref_R, h->d_ref_t, h->d_ref_inl, h->d_ref_info, h->d_ref_rms, mm, max_iters);
}

// ------------------------------------------------------------ scale links
// rpe_scale_links (NOT in the reference; include/rpe_amd.h states the rules): the baseline of pair b in units of the
// baseline of pair a, from the keypoints of the frame the two pairs share that both triangulated.  One 256-thread
// workgroup per link, f64 throughout, everything between the per-match buffers and the three results stays in LDS.
//   table   (link_join) one word per keypoint of the shared frame: high half = lowest usable match index of pair a, low
//           half = of pair b, 0xFFFF = none (max_matches <= 8064).  Pass 1: a's usable matches atomicMin (index << 16 |
//           0xFFFF): every low half is still 0xFFFF, so the minimum orders the high halves.  Pass 2: b's usable matches
//           whose key has an a entry atomicMin (that high half << 16 | index): equal high halves, the minimum orders the
//           low ones.
//   ratios  pass 3: b's matches that won their key compute d_a / d_b and append it to an LDS array (integer atomicAdd on
//           the fill count: the order inside the array varies run to run, the set does not)
//   ranks   bitonic sort of the array, padded with +inf to a power of two; the three results are elements of the sorted
//           array, so they are bit-deterministic whatever order pass 3 left (ties are equal values)
// Dynamic LDS (all of the kernel's LDS, base 16-byte aligned): [sort_cap f64 ratios][kcap u32 table][fill count],
// sort_cap = next power of two >= max_matches.  Defaults (500 matches, 4064 keypoints): 4 + 15.9 KB; uncapped SIFT
// (8064 matches, 16384 keypoints): 64 + 64 KB, above the 64 KB a kernel gets without the function attribute.
// The link, the two pairs' status, match counts, R and t come from blockIdx-indexed reads: uniform, scalar loads.
#define LINK_NONE 0xFFFFu

// the triangulated point P of a pair with pose (R, t) in the shared frame's coordinates: P itself when the shared frame is
// the pair's image 1, R P + t when it is its image 2
__device__ __forceinline__ void link_point(const double *__restrict__ P, const double (&R)[9], const double (&t)[3], bool image2,
                                           double &x, double &y, double &z)
{
    x = P[0]; y = P[1]; z = P[2];
    if (image2) {
        const double X = x, Y = y, Z = z;
        x = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
        y = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
        z = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    }
}

__device__ __forceinline__ double link_distance(const double *__restrict__ P, const double (&R)[9], const double (&t)[3], bool image2)
{
    double x, y, z;
    link_point(P, R, t, image2, x, y, z);
    return sqrt((x * x + y * y) + z * z);
}

// The table of the header in s_tab[kcap], for pairs a and b of a link: key_a / key_b their matches' keypoint indices in the
// shared frame, na / nb their match counts, oa / ob their offsets into the two masks.  A match of a is usable when both
// masks hold it; FILTER_B asks the same of b's matches, else every match of b takes part.  All 256 threads call it (three
// barriers, the last behind pass 2: the table is final on return).
template <bool FILTER_B>
__device__ __forceinline__ void link_join(unsigned *s_tab, int kcap, const int *__restrict__ key_a, int na, long long oa,
                                          const int *__restrict__ key_b, int nb, long long ob,
                                          const uint8_t *__restrict__ ransac_mask, const uint8_t *__restrict__ pose_mask)
{
    const int tid = threadIdx.x;
    for (int k = tid; k < kcap; k += 256) s_tab[k] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = tid; i < na; i += 256) {
        if (!(ransac_mask[oa + i] && pose_mask[oa + i])) continue;
        const int key = key_a[i];
        if ((unsigned)key < (unsigned)kcap) atomicMin(&s_tab[key], ((unsigned)i << 16) | LINK_NONE);
    }
    __syncthreads();
    for (int i = tid; i < nb; i += 256) {
        if (FILTER_B && !(ransac_mask[ob + i] && pose_mask[ob + i])) continue;
        const int key = key_b[i];
        if ((unsigned)key >= (unsigned)kcap) continue;
        const unsigned e = s_tab[key];                      // the high half is final since the barrier
        if ((e >> 16) != LINK_NONE) atomicMin(&s_tab[key], (e & 0xFFFF0000u) | (unsigned)i);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void scale_links_kernel(const RpeLink *__restrict__ links, const int *__restrict__ m_q,
                                                           const int *__restrict__ m_t, const int *__restrict__ m_n,
                                                           const int *__restrict__ status, const uint8_t *__restrict__ ransac_mask,
                                                           const uint8_t *__restrict__ pose_mask, const double *__restrict__ points,
                                                           const double *__restrict__ Rall, const double *__restrict__ tall,
                                                           int max_matches, int kcap, int sort_cap, int min_shared,
                                                           double *__restrict__ stats, int *__restrict__ n_shared, int *__restrict__ code)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_link[];
    double *s_ratio = (double *)s_link;
    unsigned *s_tab = (unsigned *)(s_link + sizeof(double) * (size_t)sort_cap);
    int *s_fill = (int *)(s_tab + kcap);
    const int link = blockIdx.x, tid = threadIdx.x;
    const RpeLink lk = links[link];
    if (status[lk.a] != RPE_PAIR_OK || status[lk.b] != RPE_PAIR_OK) {
        if (tid < 3) stats[link * 3 + tid] = 0.;
        if (tid == 0) { n_shared[link] = 0; code[link] = RPE_LINK_PAIR_FAILED; }
        return;
    }
    const bool a2 = (lk.side & 1) != 0, b2 = (lk.side & 2) != 0;
    const int na = min(m_n[lk.a], max_matches), nb = min(m_n[lk.b], max_matches);
    const long long oa = (long long)lk.a * max_matches, ob = (long long)lk.b * max_matches;
    const int *key_a = (a2 ? m_t : m_q) + oa, *key_b = (b2 ? m_t : m_q) + ob;
    if (tid == 0) *s_fill = 0;
    link_join<true>(s_tab, kcap, key_a, na, oa, key_b, nb, ob, ransac_mask, pose_mask);
    double Ra[9], ta[3], Rb[9], tb[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) { Ra[e] = Rall[lk.a * 9 + e]; Rb[e] = Rall[lk.b * 9 + e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) { ta[e] = tall[lk.a * 3 + e]; tb[e] = tall[lk.b * 3 + e]; }
    for (int i = tid; i < nb; i += 256) {
        if (!(ransac_mask[ob + i] && pose_mask[ob + i])) continue;
        const int key = key_b[i];
        if ((unsigned)key >= (unsigned)kcap) continue;
        const unsigned e = s_tab[key];
        if ((e >> 16) == LINK_NONE || (e & 0xFFFFu) != (unsigned)i) continue;
        const double da = link_distance(points + (oa + (e >> 16)) * 3, Ra, ta, a2);
        const double db = link_distance(points + (ob + i) * 3, Rb, tb, b2);
        s_ratio[atomicAdd(s_fill, 1)] = da / db;             // at most one winner per match of b: fill <= nb <= sort_cap
    }
    __syncthreads();
    const int n = *s_fill;
    int N = 1;
    while (N < n) N <<= 1;
    for (int i = n + tid; i < N; i += 256) s_ratio[i] = __builtin_inf();
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const double u = s_ratio[i], v = s_ratio[p];
                    if ((u > v) == ((i & k) == 0)) { s_ratio[i] = v; s_ratio[p] = u; }
                }
            }
            __syncthreads();
        }
    const bool ok = n >= min_shared;
    if (tid < 3) stats[link * 3 + tid] = ok ? s_ratio[((n - 1) * (tid + 1)) / 4] : 0.;
    if (tid == 0) { n_shared[link] = n; code[link] = ok ? RPE_LINK_OK : RPE_LINK_TOO_FEW; }
}

// A launch with more than 64 KB of dynamic LDS needs the kernels' limit raised first, once per device: the launchers of
// scale links, homographies and link poses call this when their handle asks for that much.  The limit belongs to the
// kernel, not to the handle, so lds_max is the most any legal handle asks of these kernels; the handle records the
// kernels it has raised.  Never inside a graph capture: rpe_scale_links, rpe_pair_homographies / rpe_find_homography and
// rpe_link_poses alone come here.
static int raise_lds_limit(rpe_handle *h, std::initializer_list<const void *> kernels, size_t lds_max)
{
    for (const void *k : kernels) {
        if (std::find(h->lds_raised.begin(), h->lds_raised.end(), k) != h->lds_raised.end()) continue;
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) return RPE_ERR_HIP;
        h->lds_raised.push_back(k);
    }
    return RPE_OK;
}

// sort_cap and the dynamic LDS of scale_links_kernel for max_matches matches and kcap keypoints (the layout at the head of
// the section)
static int scale_links_sort_cap(int mm)
{
    int sort_cap = 8;
    while (sort_cap < mm) sort_cap <<= 1;
    return sort_cap;
}
static size_t scale_links_lds(int mm, int kcap) { return sizeof(double) * (size_t)scale_links_sort_cap(mm) + sizeof(unsigned) * (size_t)kcap + 16; }

// the last run's d_status / d_m_n / d_R / d_t, its match indices and the structure buffers -> d_link_stats / _n / _code of
// the L links in d_links
int rpe_launch_scale_links(rpe_handle *h, int L, int min_shared)
{
    const int mm = h->cfg.max_matches, kcap = h->lay.kcap;
    const int sort_cap = scale_links_sort_cap(mm);
    const size_t lds = scale_links_lds(mm, kcap);
    // the most: 8064 matches of uncapped SIFT's keypoints
    if (lds > 65536 && raise_lds_limit(h, {(const void *)scale_links_kernel}, scale_links_lds(8064, RPE_SIFT_UNCAPPED_CAPACITY + 64)) != RPE_OK)
        return RPE_ERR_HIP;
    hipLaunchKernelGGL(scale_links_kernel, dim3(L), dim3(256), lds, h->stream, (const RpeLink *)h->d_links,
                       (const int *)h->d_m_q, (const int *)h->d_m_t, (const int *)h->d_m_n, (const int *)h->d_status,
                       (const uint8_t *)h->d_mask, (const uint8_t *)h->d_pose_mask, (const double *)h->d_points,
                       (const double *)h->d_R, (const double *)h->d_t, mm, kcap, sort_cap, min_shared,
                       h->d_link_stats, h->d_link_n, h->d_link_code);
    return RPE_OK;
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
// the default 500 matches, 100 KB at the cut -- above the 64 KB a kernel gets without the function attribute.
#define HG_ROUND 256
#define HG_MODEL_DOUBLES 18
#define HG_LDS_MATCHES 2048

__device__ __forceinline__ double hg_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void hg_cross(const double (&a)[3], const double (&b)[3], double (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

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

__device__ __forceinline__ bool hg_finite(double v) { return fabs(v) <= DBL_MAX; }

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

// d_n1 / d_n2 (the run's, or rpe_launch_normalise's in the stage form) -> d_hg_*.  from_batch: the run's d_status and
// d_rstate gate the pairs and supply n_E.
int rpe_launch_homography(rpe_handle *h, const RpeRun &r, int iters, double threshold_px, bool from_batch)
{
    const int mm = h->cfg.max_matches;
    const int use_lds = mm <= HG_LDS_MATCHES;
    const size_t lds = sizeof(double) * HG_ROUND * HG_MODEL_DOUBLES + (use_lds ? sizeof(double2) * 2 * (size_t)mm : 0);
    // the most: the points of the cut
    const size_t lds_max = sizeof(double) * HG_ROUND * HG_MODEL_DOUBLES + sizeof(double2) * 2 * HG_LDS_MATCHES;
    if (lds > 65536 && raise_lds_limit(h, {(const void *)homography_kernel<true>, (const void *)homography_kernel<false>}, lds_max) != RPE_OK)
        return RPE_ERR_HIP;
    launch_cam(r, homography_kernel<true>, homography_kernel<false>, dim3(r.pairs), dim3(256), lds, h->stream,
               (const double2 *)h->d_n1, (const double2 *)h->d_n2, (const int *)h->d_m_n,
               from_batch ? (const int *)h->d_status : (const int *)nullptr,
               from_batch ? (const RpeRansacState *)h->d_rstate : (const RpeRansacState *)nullptr,
               (const unsigned short *)h->d_subsets, (const double *)h->d_K, r.cam, threshold_px, iters, h->cfg.ransac_max_iters,
               mm, use_lds, h->d_hg_H, h->d_hg_R, h->d_hg_mask, h->d_hg_counts, h->d_hg_info);
    return RPE_OK;
}

// ------------------------------------------------------------ link poses
// rpe_link_poses (NOT in the reference; include/rpe_amd.h states the rule): the pose of pair b's other frame C against the
// points pair a triangulated, by P3P RANSAC over the keypoints of the shared frame S, on pair a's scale.  One 256-thread
// workgroup per link, f64 throughout, no contraction.
//   join     link_join's packed table (high half: lowest usable match of a, low half: lowest match of b; here every match
//            of b takes part).  The winners of b are then compacted in match order by ordered_slot (ballot / popcount):
//            correspondence c = the c-th winner, so no atomic decides an order.
//   list     per correspondence X (3 f64, link_point: in S's frame), q (2 f64) and b's match index (u16).  X and q live in
//            LDS up to LP_LDS_MATCHES matches (40 B each: 20 KB at the default 500) and in d_lp_corr above it; both forms
//            are walked through the same pointers in the same order.  The indices are always in LDS.
//   rounds   as the homography's: LP_ROUND = 256 samples at a time, thread j solves sample j in registers (quartic, the
//            derivative chain with static indices, up to four poses) and parks its candidates at slot 4 j + root; the
//            slots of the valid ones are listed densely in (iteration, root) order (block_excl_scan of the per-thread
//            counts).  The four waves score the dense list round-robin, lanes striding the correspondences, wave_sum
//            for the count; a wave meets its candidates in ascending (iteration, root) order and replaces its best on a
//            strictly larger count only; the cross-wave election (elect_best) compares (count, 4 * iteration + root).
//   winner   solved again by every thread (the same code on the same operands: the same bits), its inlier flags, then the
//            polish: refine_lm<6> on the reprojection residuals (block_sum_f64 sums, refine_rotate), and the fallback
//            test over all correspondences.
// Dynamic LDS (all of the kernel's LDS, base 16-byte aligned):
//   [A] max(kcap u32 table, LP_ROUND * 4 poses of 12 f64 = 96 KB): the table is dead once the list is built, the poses
//       once the election is over (the winner's inlier flags then live there)
//   [s_red 4 * 28 f64][X, q: 40 B * max_matches when in LDS][dense list 1024 u16][match indices max_matches u16][32 ints]
// 120 KB at the defaults (one workgroup per CU), 141 KB at the cut, 115 KB for uncapped SIFT (8064 matches in d_lp_corr).
#define LP_ROUND 256
#define LP_POSE_DOUBLES 12
#define LP_LDS_MATCHES 1024
#define LP_NSUM 28                   // 21 J'J + 6 J'r + 1 r'r

struct LpQuartic { double j[9], b2, q1, n0, n1, n2, d0, d1, c[5]; };

// bearings, side lengths, cosines and the quartic in v of the header
__device__ __forceinline__ void lp_quartic(const double (&P)[9], const double (&q)[6], LpQuartic &g)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = q[2 * k], y = q[2 * k + 1], m = sqrt((x * x + y * y) + 1.);
        g.j[3 * k] = x / m; g.j[3 * k + 1] = y / m; g.j[3 * k + 2] = 1. / m;
    }
    const double d23[3] = {P[3] - P[6], P[4] - P[7], P[5] - P[8]}, d13[3] = {P[0] - P[6], P[1] - P[7], P[2] - P[8]};
    const double d12[3] = {P[0] - P[3], P[1] - P[4], P[2] - P[5]};
    const double j1[3] = {g.j[0], g.j[1], g.j[2]}, j2[3] = {g.j[3], g.j[4], g.j[5]}, j3[3] = {g.j[6], g.j[7], g.j[8]};
    const double a2 = hg_dot(d23, d23), b2 = hg_dot(d13, d13), c2 = hg_dot(d12, d12);
    const double ca = hg_dot(j2, j3), cb = hg_dot(j1, j3), cg = hg_dot(j1, j2);
    const double q1 = -(2. * cb), m = a2 - c2;
    const double n0 = b2 + m, n1 = m * q1, n2 = m - b2;
    const double d0 = (2. * b2) * cg, d1 = -((2. * b2) * ca);
    const double nn[5] = {n0 * n0, 2. * (n0 * n1), 2. * (n0 * n2) + n1 * n1, 2. * (n1 * n2), n2 * n2};
    const double nd[4] = {n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1};
    const double dd[3] = {d0 * d0, 2. * (d0 * d1), d1 * d1};
    const double w0 = b2 - c2, w1 = -(c2 * q1), w2 = -c2;
    const double wd[5] = {w0 * dd[0], w0 * dd[1] + w1 * dd[0], (w0 * dd[2] + w1 * dd[1]) + w2 * dd[0], w1 * dd[2] + w2 * dd[1], w2 * dd[2]};
#pragma unroll
    for (int i = 0; i < 4; ++i) g.c[i] = (b2 * nn[i] - d0 * nd[i]) + wd[i];
    g.c[4] = b2 * nn[4] + wd[4];
    g.b2 = b2; g.q1 = q1; g.n0 = n0; g.n1 = n1; g.n2 = n2; g.d0 = d0; g.d1 = d1;
}

// One level of the derivative chain in registers: the roots of p (degree K, p' = dp) between the nr_prev roots of dp in
// crit, ascending into out.  Every index is static: the interval loop unrolls, a root lands in its slot by compares.
template <int K>
__device__ __forceinline__ int lp_level(const double (&p)[5], const double (&dp)[5], const double (&crit)[4], int nr_prev, double (&out)[4])
{
    const double R = root_bound<K>(p);
    int nout = 0;
#pragma unroll
    for (int iv = 0; iv < K; ++iv) {                     // dp has at most K - 1 roots: at most K intervals
        const double a = iv == 0 ? -R : crit[iv - 1], b = iv == nr_prev ? R : crit[iv];
        double root;
        if (bracket_root<K>(p, dp, a, b, R, iv <= nr_prev, root)) {
#pragma unroll
            for (int s = 0; s < 4; ++s) if (s == nout) out[s] = root;
            ++nout;
        }
    }
    return nout;
}

// real roots, ascending, of c[0] + ... + c[N] x^N (c[N] != 0): poly_real_roots_generic's chain for a degree known at
// compile time
template <int N>
__device__ __forceinline__ int lp_chain(const double (&c)[5], double (&roots)[4])
{
    double lv[5][5];
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int i = 0; i < 5; ++i) lv[k][i] = (k == N && i <= N) ? c[i] : 0.;
#pragma unroll
    for (int k = N; k >= 2; --k)
#pragma unroll
        for (int i = 0; i < k; ++i) lv[k - 1][i] = lv[k][i + 1] * (double)(i + 1);
    double crit[4] = {-lv[1][0] / lv[1][1], 0., 0., 0.};
    int nr = 1;
    if (N >= 2) {
        double out[4] = {0., 0., 0., 0.};
        nr = lp_level<2>(lv[2], lv[1], crit, nr, out);
#pragma unroll
        for (int s = 0; s < 4; ++s) crit[s] = out[s];
    }
    if (N >= 3) {
        double out[4] = {0., 0., 0., 0.};
        nr = lp_level<3>(lv[3], lv[2], crit, nr, out);
#pragma unroll
        for (int s = 0; s < 4; ++s) crit[s] = out[s];
    }
    if (N >= 4) {
        double out[4] = {0., 0., 0., 0.};
        nr = lp_level<4>(lv[4], lv[3], crit, nr, out);
#pragma unroll
        for (int s = 0; s < 4; ++s) crit[s] = out[s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) roots[s] = crit[s];
    return nr;
}

// the quartic's real roots: its degree is the highest non-zero coefficient
__device__ __forceinline__ int lp_roots(const double (&c)[5], double (&roots)[4])
{
    if (c[4] != 0.) return lp_chain<4>(c, roots);
    if (c[3] != 0.) return lp_chain<3>(c, roots);
    if (c[2] != 0.) return lp_chain<2>(c, roots);
    if (c[1] != 0.) return lp_chain<1>(c, roots);
    return 0;
}

// e1 = (A2 - A1) / |.|, e3 = (e1 x (A3 - A1)) / |.|, e2 = e3 x e1 of three points A1 A2 A3 (rows of A); e = rows e1 e2 e3
__device__ __forceinline__ void lp_frame(const double (&A)[9], double (&e)[9])
{
    const double d[3] = {A[3] - A[0], A[4] - A[1], A[5] - A[2]}, w[3] = {A[6] - A[0], A[7] - A[1], A[8] - A[2]};
    const double nd = sqrt(hg_dot(d, d));
    const double e1[3] = {d[0] / nd, d[1] / nd, d[2] / nd};
    double c[3], e2[3];
    hg_cross(e1, w, c);
    const double nc = sqrt(hg_dot(c, c));
    const double e3[3] = {c[0] / nc, c[1] / nc, c[2] / nc};
    hg_cross(e3, e1, e2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { e[k] = e1[k]; e[3 + k] = e2[k]; e[6 + k] = e3[k]; }
}

// the candidate of root v: Rt = R (9, row-major) then t (3); false when v is no candidate
__device__ __forceinline__ bool lp_pose(const double (&P)[9], const LpQuartic &g, double v, double (&Rt)[LP_POSE_DOUBLES])
{
    const double Dv = g.d0 + g.d1 * v, Nv = (g.n0 + g.n1 * v) + g.n2 * (v * v), Qv = (1. + g.q1 * v) + v * v;
    const double u = Nv / Dv;
    bool ok = v > 0. && Dv != 0. && u > 0. && Qv > 0.;
    const double s1 = sqrt(g.b2 / Qv), s2 = u * s1, s3 = v * s1;
    double Y[9], e[9], f[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { Y[k] = s1 * g.j[k]; Y[3 + k] = s2 * g.j[3 + k]; Y[6 + k] = s3 * g.j[6 + k]; }
    lp_frame(P, e); lp_frame(Y, f);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Rt[r * 3 + c] = (f[r] * e[c] + f[3 + r] * e[3 + c]) + f[6 + r] * e[6 + c];
        Rt[9 + r] = Y[r] - ((Rt[r * 3] * P[0] + Rt[r * 3 + 1] * P[1]) + Rt[r * 3 + 2] * P[2]);
    }
#pragma unroll
    for (int k = 0; k < LP_POSE_DOUBLES; ++k) ok = ok && hg_finite(Rt[k]);
    return ok;
}

// y = R X + t and the inlier test of the header
__device__ __forceinline__ bool lp_inlier(const double (&Rt)[LP_POSE_DOUBLES], const double *X, const double *q, double thr2)
{
    const double y0 = ((Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2]) + Rt[9];
    const double y1 = ((Rt[3] * X[0] + Rt[4] * X[1]) + Rt[5] * X[2]) + Rt[10];
    const double y2 = ((Rt[6] * X[0] + Rt[7] * X[1]) + Rt[8] * X[2]) + Rt[11];
    const double dx = y0 - q[0] * y2, dy = y1 - q[1] * y2;
    return y2 > 0. && (dx * dx + dy * dy) <= thr2 * (y2 * y2);
}

// the three correspondences of iteration `it`
__device__ __forceinline__ void lp_sample(const unsigned short *__restrict__ sub, int it, const double *cX, const double *cq,
                                          double (&P)[9], double (&q)[6])
{
    const unsigned short *s5 = sub + (long long)it * 5;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = s5[k];
        P[3 * k] = cX[3 * v]; P[3 * k + 1] = cX[3 * v + 1]; P[3 * k + 2] = cX[3 * v + 2];
        q[2 * k] = cq[2 * v]; q[2 * k + 1] = cq[2 * v + 1];
    }
}

// the two reprojection residuals of one correspondence in pixels; optionally their derivatives by (w0 w1 w2 | d0 d1 d2)
template <bool JAC>
__device__ __forceinline__ void lp_residual(const double *R, const double *t, double scale, const double *X, const double *q,
                                            double &rx, double &ry, double *Jx, double *Jy)
{
    const double a0 = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], a1 = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2];
    const double a2 = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
    const double y0 = a0 + t[0], y1 = a1 + t[1], y2 = a2 + t[2];
    const double ux = y0 / y2, uy = y1 / y2;
    rx = scale * (ux - q[0]); ry = scale * (uy - q[1]);
    if (JAC) {                                            // d y / d w_k = e_k x (R X), d y / d d = I
        const double s = scale / y2;
        Jx[0] = -s * (ux * a1); Jx[1] = s * (a2 + ux * a0); Jx[2] = -s * a1; Jx[3] = s; Jx[4] = 0.; Jx[5] = -s * ux;
        Jy[0] = -s * (a2 + uy * a1); Jy[1] = s * (uy * a0); Jy[2] = s * a0; Jy[3] = 0.; Jy[4] = s; Jy[5] = -s * uy;
    }
}

template <bool CAM>
__global__ __launch_bounds__(256) void link_pose_kernel(const RpeLink *__restrict__ links, const int *__restrict__ m_q,
                                                         const int *__restrict__ m_t, const int *__restrict__ m_n,
                                                         const int *__restrict__ status, const uint8_t *__restrict__ ransac_mask,
                                                         const uint8_t *__restrict__ pose_mask, const double *__restrict__ points,
                                                         const double *__restrict__ Rall, const double *__restrict__ tall,
                                                         const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                         const unsigned short *__restrict__ subsets, const double *__restrict__ K,
                                                         const RpeCamSrc cam, double threshold_px, int iters, int max_iters,
                                                         int max_matches, int kcap, int min_shared, int refine_iters,
                                                         double *__restrict__ corr, double *__restrict__ Rout,
                                                         double *__restrict__ tout, uint8_t *__restrict__ mask,
                                                         int *__restrict__ counts, int *__restrict__ info, double *__restrict__ rms)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lp[];
    const bool use_lds = corr == nullptr;
    const size_t bytesT = sizeof(unsigned) * (size_t)kcap, bytesM = sizeof(double) * LP_ROUND * 4 * LP_POSE_DOUBLES;
    const size_t bytesA = bytesT > bytesM ? bytesT : bytesM;
    unsigned *s_tab = (unsigned *)s_lp;                                      // [kcap], until the list is built
    double *s_model = (double *)s_lp;                                        // [LP_ROUND * 4][12], during the rounds
    uint8_t *s_in = (uint8_t *)s_lp;                                         // [n] the winner's inlier flags, after the election
    double *s_red = (double *)(s_lp + ((bytesA + 15) & ~(size_t)15));        // [4 * LP_NSUM]
    double *s_corr = s_red + 4 * LP_NSUM;                                    // [5 * max_matches] when use_lds
    unsigned short *s_list = (unsigned short *)(s_corr + (use_lds ? 5 * (size_t)max_matches : 0));   // [LP_ROUND * 4]
    unsigned short *s_idx = s_list + LP_ROUND * 4;                           // [max_matches rounded up to 8]
    int *s_int = (int *)(s_idx + ((max_matches + 7) & ~7));                  // [4] wave counts, [8] bests, [4] counts
    int *s_wc = s_int, *s_best = s_int + 4, *s_cnt = s_int + 12;
    const int link = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const RpeLink lk = links[link];
    const long long om = (long long)link * max_matches;
    int code = status[lk.a] == RPE_PAIR_OK ? RPE_LINKPOSE_OK : RPE_LINKPOSE_PAIR_FAILED;
    int n = 0;
    double *cX = use_lds ? s_corr : corr + (long long)link * 5 * max_matches, *cq = cX + 3 * (size_t)max_matches;
    const bool a2 = (lk.side & 1) != 0, b2 = (lk.side & 2) != 0;
    if (code == RPE_LINKPOSE_OK) {                                           // workgroup-uniform
        // ---- join and ordered list
        const int na = min(m_n[lk.a], max_matches), nb = min(m_n[lk.b], max_matches);
        const long long oa = (long long)lk.a * max_matches, ob = (long long)lk.b * max_matches;
        const int *key_a = (a2 ? m_t : m_q) + oa, *key_b = (b2 ? m_t : m_q) + ob;
        const double2 *obs = (b2 ? n1 : n2) + ob;                            // b's point on C, its frame that is not shared
        link_join<false>(s_tab, kcap, key_a, na, oa, key_b, nb, ob, ransac_mask, pose_mask);
        double Ra[9], ta[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) Ra[e] = Rall[lk.a * 9 + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) ta[e] = tall[lk.a * 3 + e];
        for (int i0 = 0; i0 < nb; i0 += 256) {
            const int i = i0 + tid;
            unsigned e = 0xFFFFFFFFu;
            if (i < nb) { const int key = key_b[i]; if ((unsigned)key < (unsigned)kcap) e = s_tab[key]; }
            const bool f = i < nb && (e >> 16) != LINK_NONE && (e & 0xFFFFu) == (unsigned)i;
            const int pos = ordered_slot(f, s_wc, n);
            if (f) {
                double x, y, z;
                link_point(points + (oa + (e >> 16)) * 3, Ra, ta, a2, x, y, z);
                const double2 o = obs[i];
                // the table and an LDS list share no bytes: s_corr lies behind region A
                cX[3 * pos] = x; cX[3 * pos + 1] = y; cX[3 * pos + 2] = z;
                cq[2 * pos] = o.x; cq[2 * pos + 1] = o.y;
                s_idx[pos] = (unsigned short)i;
            }
        }
        __syncthreads();                                                     // the list is complete, the table is dead
        if (n < max(min_shared, 6)) code = RPE_LINKPOSE_TOO_FEW;
    }
    int win_cnt = -1, win_key = -1;
    double thr2 = 0., scale = 0.;
    const unsigned short *sub = subsets + (long long)n * max_iters * 5;
    if (code == RPE_LINKPOSE_OK) {
        scale = rpe_pair_focal<CAM>(K, cam, lk.b);
        const double thr = threshold_px / scale;
        thr2 = thr * thr;
        int best_cnt = -1, best_key = -1;
        for (int base = 0; base < iters; base += LP_ROUND) {
            const int nr = min(LP_ROUND, iters - base);
            __syncthreads();                                                 // the previous round's candidates have been scored
            unsigned vm = 0;
            if (tid < nr) {
                double P[9], q[6], roots[4];
                LpQuartic g;
                lp_sample(sub, base + tid, cX, cq, P, q);
                lp_quartic(P, q, g);
                const int nroots = lp_roots(g.c, roots);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double Rt[LP_POSE_DOUBLES];
                    if (r < nroots && lp_pose(P, g, roots[r], Rt)) {
                        double *d = s_model + (tid * 4 + r) * LP_POSE_DOUBLES;
#pragma unroll
                        for (int e = 0; e < LP_POSE_DOUBLES; ++e) d[e] = Rt[e];
                        vm |= 1u << r;
                    }
                }
            }
            int total;
            int off = block_excl_scan(__popc(vm), s_wc, total);
#pragma unroll
            for (int r = 0; r < 4; ++r) if (vm & (1u << r)) s_list[off++] = (unsigned short)(tid * 4 + r);
            __syncthreads();
            for (int j = wv; j < total; j += 4) {                            // wave-uniform
                const int id = s_list[j];
                double Rt[LP_POSE_DOUBLES];
                const double *d = s_model + id * LP_POSE_DOUBLES;
#pragma unroll
                for (int e = 0; e < LP_POSE_DOUBLES; ++e) Rt[e] = d[e];
                int cnt = 0;
                for (int c = lane; c < n; c += 64) cnt += lp_inlier(Rt, cX + 3 * c, cq + 2 * c, thr2) ? 1 : 0;
                cnt = wave_sum(cnt);
                if (cnt > best_cnt) { best_cnt = cnt; best_key = (base + (id >> 2)) * 4 + (id & 3); }
            }
        }
        elect_best(best_cnt, best_key, s_best, win_cnt, win_key);
        if (win_key < 0) code = RPE_LINKPOSE_NONE;
    }
    if (code != RPE_LINKPOSE_OK) {
        for (int i = tid; i < max_matches; i += 256) mask[om + i] = 0;
        if (tid < 9) Rout[link * 9 + tid] = 0.;
        if (tid < 3) tout[link * 3 + tid] = 0.;
        if (tid < 2) rms[link * 2 + tid] = 0.;
        if (tid == 0) {
            counts[link * 2] = n; counts[link * 2 + 1] = 0;
            info[link * 4] = code; info[link * 4 + 1] = 0; info[link * 4 + 2] = 0; info[link * 4 + 3] = 0;
        }
        return;
    }
    // ---- the winner again, on every thread
    const int win_it = win_key >> 2, win_root = win_key & 3;
    double Rt[LP_POSE_DOUBLES];
    {
        double P[9], q[6], roots[4];
        LpQuartic g;
        lp_sample(sub, win_it, cX, cq, P, q);
        lp_quartic(P, q, g);
        lp_roots(g.c, roots);
        double v = roots[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) if (r == win_root) v = roots[r];
        lp_pose(P, g, v, Rt);
    }
    // its inlier flags (the candidates are dead: every wave passed the barrier of the election)
    for (int c = tid; c < n; c += 256) s_in[c] = lp_inlier(Rt, cX + 3 * c, cq + 2 * c, thr2) ? 1 : 0;
    __syncthreads();
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rt[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = Rt[9 + e];
    // ---- polish over the winner's inliers
    double s[LP_NSUM];
    auto linearise = [&]() {
#pragma unroll
        for (int k = 0; k < LP_NSUM; ++k) s[k] = 0.;
        for (int c = tid; c < n; c += 256) {
            if (!s_in[c]) continue;
            double rx, ry, Jx[6], Jy[6];
            lp_residual<true>(R, t, scale, cX + 3 * c, cq + 2 * c, rx, ry, Jx, Jy);
            int q = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u)
#pragma unroll
                for (int v = u; v < 6; ++v, ++q) s[q] += Jx[u] * Jx[v] + Jy[u] * Jy[v];
#pragma unroll
            for (int u = 0; u < 6; ++u) s[21 + u] += Jx[u] * rx + Jy[u] * ry;
            s[27] += rx * rx + ry * ry;
        }
        block_sum_f64<LP_NSUM>(s, s_red, tid);
    };
    // R <- exp([w]x) R, t <- t + (d3 d4 d5)
    auto trial = [&](const double (&d)[6], double (&Rn)[9], double (&tn)[3]) {
        refine_rotate(d, R, Rn);
#pragma unroll
        for (int e = 0; e < 3; ++e) tn[e] = t[e] + d[3 + e];
        double cs = 0.;
        for (int c = tid; c < n; c += 256) {
            if (!s_in[c]) continue;
            double rx, ry;
            lp_residual<false>(Rn, tn, scale, cX + 3 * c, cq + 2 * c, rx, ry, nullptr, nullptr);
            cs += rx * rx + ry * ry;
        }
        return cs;
    };
    linearise();
    const double cost0 = s[27];
    double cost = cost0;
    int lm_iters = 0, acc = 0;
    if (isfinite(cost0)) refine_lm<6>(R, t, cost, refine_iters, s_red, linearise, RefineNormalSolve<6>{s}, trial, RefineNoCommit{}, lm_iters, acc);
    // ---- fallback: the polished pose must be finite and keep the winner's count over all correspondences
    const int m = win_cnt;                                                  // the winner's inliers: the residual set
    int polish = 0;
    if (acc > 0) {
        double Rp[LP_POSE_DOUBLES];
        bool fin = true;
#pragma unroll
        for (int e = 0; e < 9; ++e) { Rp[e] = R[e]; fin = fin && hg_finite(R[e]); }
#pragma unroll
        for (int e = 0; e < 3; ++e) { Rp[9 + e] = t[e]; fin = fin && hg_finite(t[e]); }
        int cnt = 0;
        for (int c = tid; c < n; c += 256) cnt += lp_inlier(Rp, cX + 3 * c, cq + 2 * c, thr2) ? 1 : 0;
        cnt = block_count(cnt, s_cnt);
        if (fin && cnt >= win_cnt) {
            polish = lm_iters;
            win_cnt = cnt;
#pragma unroll
            for (int e = 0; e < LP_POSE_DOUBLES; ++e) Rt[e] = Rp[e];
        } else
            polish = -1;
    }
    // ---- outputs: the mask by pair b's match index, the pose in pair b's convention
    for (int i = tid; i < max_matches; i += 256) mask[om + i] = 0;
    __syncthreads();                                                         // zeros first: another thread sets the inliers
    for (int c = tid; c < n; c += 256)
        if (lp_inlier(Rt, cX + 3 * c, cq + 2 * c, thr2)) mask[om + s_idx[c]] = 1;
    if (tid == 0) {
        double Ro[9], to[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Ro[r * 3 + c] = b2 ? Rt[c * 3 + r] : Rt[r * 3 + c];
            to[r] = b2 ? -((Rt[r] * Rt[9] + Rt[3 + r] * Rt[10]) + Rt[6 + r] * Rt[11]) : Rt[9 + r];
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) Rout[link * 9 + e] = Ro[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) tout[link * 3 + e] = to[e];
        counts[link * 2] = n; counts[link * 2 + 1] = win_cnt;
        info[link * 4] = RPE_LINKPOSE_OK; info[link * 4 + 1] = win_it; info[link * 4 + 2] = win_root; info[link * 4 + 3] = polish;
        const double before = m > 0 ? sqrt(cost0 / m) : 0.;
        rms[link * 2] = before;
        rms[link * 2 + 1] = polish > 0 ? sqrt(cost / m) : before;
    }
}

// dynamic LDS of link_pose_kernel for max_matches matches and kcap keypoints (the layout at the head of the kernel)
static size_t link_pose_lds(int mm, int kcap)
{
    const size_t bytesA = std::max(sizeof(unsigned) * (size_t)kcap, sizeof(double) * LP_ROUND * 4 * LP_POSE_DOUBLES);
    return ((bytesA + 15) & ~(size_t)15) + sizeof(double) * 4 * LP_NSUM + (mm <= LP_LDS_MATCHES ? sizeof(double) * 5 * (size_t)mm : 0) +
           sizeof(unsigned short) * (LP_ROUND * 4 + (size_t)((mm + 7) & ~7)) + sizeof(int) * 32;
}

// the correspondence lists of this handle fit the kernel's LDS (else rpe_link_poses creates d_lp_corr)
bool rpe_link_poses_in_lds(const rpe_handle *h) { return h->cfg.max_matches <= LP_LDS_MATCHES; }

// the links in d_links over the last run r (its d_status / d_m_n / d_R / d_t, match indices, d_n1 / d_n2 and the structure
// buffers) -> d_lp_*.  Above LP_LDS_MATCHES the lists go to d_lp_corr, which the caller has allocated.
int rpe_launch_link_poses(rpe_handle *h, const RpeRun &r, int L, int iters, double threshold_px, int min_shared, int refine_iters)
{
    const int mm = h->cfg.max_matches, kcap = h->lay.kcap;
    const size_t lds = link_pose_lds(mm, kcap);
    // the most: the cut, or the largest max_matches; no table is larger than the candidates it shares region A with
    const size_t lds_max = std::max(link_pose_lds(LP_LDS_MATCHES, 0), link_pose_lds(8064, 0));
    if (lds > lds_max) return RPE_ERR_HIP;
    if (lds > 65536 && raise_lds_limit(h, {(const void *)link_pose_kernel<true>, (const void *)link_pose_kernel<false>}, lds_max) != RPE_OK)
        return RPE_ERR_HIP;
    launch_cam(r, link_pose_kernel<true>, link_pose_kernel<false>, dim3(L), dim3(256), lds, h->stream, (const RpeLink *)h->d_links,
               (const int *)h->d_m_q, (const int *)h->d_m_t, (const int *)h->d_m_n, (const int *)h->d_status,
               (const uint8_t *)h->d_mask, (const uint8_t *)h->d_pose_mask, (const double *)h->d_points,
               (const double *)h->d_R, (const double *)h->d_t, (const double2 *)h->d_n1, (const double2 *)h->d_n2,
               (const unsigned short *)h->d_subsets, (const double *)h->d_K, r.cam, threshold_px, iters, h->cfg.ransac_max_iters,
               mm, kcap, min_shared, refine_iters, mm <= LP_LDS_MATCHES ? (double *)nullptr : h->d_lp_corr,
               h->d_lp_R, h->d_lp_t, h->d_lp_mask, h->d_lp_counts, h->d_lp_info, h->d_lp_rms);
    return RPE_OK;
}

// ------------------------------------------------------------ link bundles
// rpe_link_bundles / rpe_bundle_three_view (NOT in the reference; include/rpe_amd.h states the rule): bundle adjustment of
// the three views of a link -- the poses of A and C relative to the shared frame S and the points both pairs see, on one
// reprojection cost.  Two device steps, f64 throughout, no contraction:
//   gather   (run form only) bundle_gather_kernel, one workgroup per link: link_join's table, then per match of pair a its
//            view code (0 no point, 1 seen by S and A, 3 also by C: lp_inlier under the input pose of C), its three
//            observations and its start point (link_point), all indexed by pair a's match index; the two start poses in
//            the solved form (S -> A, S -> C) and the two focal scales.  The stage form uploads the same arrays.
//   bundle   bundle_kernel, one workgroup per problem, whichever form filled the arrays: the points are compacted in index
//            order (ordered_slot), their state (X and the trial X, 48 B per point) lives in LDS up to BA_LDS_MATCHES matches
//            and in d_ba_state above it, walked through the same pointers in the same order; the observations are read
//            where the gather left them.  refine_lm<11> with a solve policy of its own:
//              linearise  U (block diagonal: 15 + 21), g_c (11) and the cost: 48 sums, parked in LDS between the trials
//              solve      per point V = Jp'Jp + lambda diag, its adjugate inverse, W (11 x 3): 66 sums of W V^-1 W', 11 of
//                         W V^-1 g_p and the count of singular V: 78 sums per damping trial; the reduced 11 x 11 system by
//                         refine_solve<11> on every lane (identical operands)
//              trial      the points' back-substitution d_p = -V^-1 (g_p + W' d_c) and the cost at the new state
//            Every sum is block_sum_f64 over lane partials in strided order: bit-deterministic.
// A point's Jacobians are formed three times per trial (solve, trial, and linearise after an accepted step): arithmetic is
// small next to the barriers, and nothing per point but X is kept.
#define BA_LDS_MATCHES 1024
#define BA_NLIN 48                   // 15 U_AA + 21 U_CC + 11 g_c + 1 r'r
#define BA_NRED 78                   // 66 W V^-1 W' + 11 W V^-1 g_p + 1 singular V

// One point's rows of the Jacobian at the current state.  Rows: S x, S y, A x, A y, C x, C y; the C rows are zero without
// that observation.
struct BaPoint {
    double e[6];                     // residuals in pixels
    double JX[6][3];                 // by the point
    double JA[2][5];                 // the A rows by (w0 w1 w2 | b1 b2)
    double JC[2][6];                 // the C rows by (w0 w1 w2 | d0 d1 d2)
};

__device__ __forceinline__ void ba_point(const double (&RA)[9], const double (&tA)[3], const double (&b1)[3], const double (&b2)[3],
                                         const double (&RC)[9], const double (&tC)[3], double fa, double fc, const double *X,
                                         const double *q /*[6]*/, bool hc, BaPoint &p)
{
    {   // S: y = X
        const double ux = X[0] / X[2], uy = X[1] / X[2], s = fa / X[2];
        p.e[0] = fa * (ux - q[0]); p.e[1] = fa * (uy - q[1]);
        p.JX[0][0] = s; p.JX[0][1] = 0.; p.JX[0][2] = -s * ux;
        p.JX[1][0] = 0.; p.JX[1][1] = s; p.JX[1][2] = -s * uy;
    }
    double Jx[6], Jy[6];
    lp_residual<true>(RA, tA, fa, X, q + 2, p.e[2], p.e[3], Jx, Jy);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p.JA[0][k] = Jx[k]; p.JA[1][k] = Jy[k];
        p.JX[2][k] = (Jx[3] * RA[k] + Jx[4] * RA[3 + k]) + Jx[5] * RA[6 + k];
        p.JX[3][k] = (Jy[3] * RA[k] + Jy[4] * RA[3 + k]) + Jy[5] * RA[6 + k];
    }
    p.JA[0][3] = (Jx[3] * b1[0] + Jx[4] * b1[1]) + Jx[5] * b1[2]; p.JA[0][4] = (Jx[3] * b2[0] + Jx[4] * b2[1]) + Jx[5] * b2[2];
    p.JA[1][3] = (Jy[3] * b1[0] + Jy[4] * b1[1]) + Jy[5] * b1[2]; p.JA[1][4] = (Jy[3] * b2[0] + Jy[4] * b2[1]) + Jy[5] * b2[2];
    if (hc) {
        lp_residual<true>(RC, tC, fc, X, q + 4, p.e[4], p.e[5], Jx, Jy);
#pragma unroll
        for (int k = 0; k < 6; ++k) { p.JC[0][k] = Jx[k]; p.JC[1][k] = Jy[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p.JX[4][k] = (Jx[3] * RC[k] + Jx[4] * RC[3 + k]) + Jx[5] * RC[6 + k];
            p.JX[5][k] = (Jy[3] * RC[k] + Jy[4] * RC[3 + k]) + Jy[5] * RC[6 + k];
        }
    } else {
        p.e[4] = 0.; p.e[5] = 0.;
#pragma unroll
        for (int k = 0; k < 6; ++k) { p.JC[0][k] = 0.; p.JC[1][k] = 0.; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { p.JX[4][k] = 0.; p.JX[5][k] = 0.; }
    }
}

// the squared residual length of one point over its views
__device__ __forceinline__ double ba_cost(const double (&e)[6]) { return ((e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3])) + (e[4] * e[4] + e[5] * e[5]); }

// The point block of p under damping lambda: Vi = (Jp'Jp + lambda diag)^-1 by the adjugate (upper triangle 00 01 02 11 12
// 22), g_p = Jp'r and W = Jc'Jp (rows 0..4: A, 5..10: C).  False when V is singular.
__device__ __forceinline__ bool ba_block(const BaPoint &p, double lambda, double (&Vi)[6], double (&gp)[3], double (&W)[11][3])
{
    double v[6] = {0., 0., 0., 0., 0., 0.};
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[i] = 0.;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        v[0] += p.JX[r][0] * p.JX[r][0]; v[1] += p.JX[r][0] * p.JX[r][1]; v[2] += p.JX[r][0] * p.JX[r][2];
        v[3] += p.JX[r][1] * p.JX[r][1]; v[4] += p.JX[r][1] * p.JX[r][2]; v[5] += p.JX[r][2] * p.JX[r][2];
#pragma unroll
        for (int i = 0; i < 3; ++i) gp[i] += p.JX[r][i] * p.e[r];
    }
    v[0] = v[0] + lambda * v[0]; v[3] = v[3] + lambda * v[3]; v[5] = v[5] + lambda * v[5];
    const double c00 = v[3] * v[5] - v[4] * v[4], c01 = v[2] * v[4] - v[1] * v[5], c02 = v[1] * v[4] - v[2] * v[3];
    const double c11 = v[0] * v[5] - v[2] * v[2], c12 = v[1] * v[2] - v[0] * v[4], c22 = v[0] * v[3] - v[1] * v[1];
    const double det = (v[0] * c00 + v[1] * c01) + v[2] * c02;
    Vi[0] = c00 / det; Vi[1] = c01 / det; Vi[2] = c02 / det; Vi[3] = c11 / det; Vi[4] = c12 / det; Vi[5] = c22 / det;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 5; ++k) W[k][i] = p.JA[0][k] * p.JX[2][i] + p.JA[1][k] * p.JX[3][i];
#pragma unroll
        for (int k = 0; k < 6; ++k) W[5 + k][i] = p.JC[0][k] * p.JX[4][i] + p.JC[1][k] * p.JX[5][i];
    }
    return det > 0. && hg_finite(det);
}

// row i of the symmetric 3 x 3 held as its upper triangle, times u
__device__ __forceinline__ double ba_sym_row(const double (&S)[6], int i, const double (&u)[3])
{
    const double a = i == 0 ? S[0] : (i == 1 ? S[1] : S[2]), b = i == 0 ? S[1] : (i == 1 ? S[3] : S[4]);
    const double c = i == 0 ? S[2] : (i == 1 ? S[4] : S[5]);
    return (a * u[0] + b * u[1]) + c * u[2];
}

// R' and -R't: the inverse of x -> R x + t, by the expression of the link poses' output
__device__ __forceinline__ void ba_invert(const double (&R)[9], const double (&t)[3], double (&Ri)[9], double (&ti)[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Ri[r * 3 + c] = R[c * 3 + r];
        ti[r] = -((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]);
    }
}

template <bool CAM>
__global__ __launch_bounds__(256) void bundle_gather_kernel(const RpeLink *__restrict__ links, const int *__restrict__ m_q,
                                                             const int *__restrict__ m_t, const int *__restrict__ m_n,
                                                             const int *__restrict__ status, const uint8_t *__restrict__ ransac_mask,
                                                             const uint8_t *__restrict__ pose_mask, const double *__restrict__ points,
                                                             const double *__restrict__ Rall, const double *__restrict__ tall,
                                                             const double2 *__restrict__ n1, const double2 *__restrict__ n2,
                                                             const double *__restrict__ K, const RpeCamSrc cam,
                                                             const double *__restrict__ Rb_in, const double *__restrict__ tb_in,
                                                             double threshold_px, int max_matches, int kcap,
                                                             uint8_t *__restrict__ views, double *__restrict__ obs, double *__restrict__ X0,
                                                             double *__restrict__ pose0, double *__restrict__ focal,
                                                             int *__restrict__ pre, int *__restrict__ n_in)
{
    extern __shared__ unsigned s_ba_tab[];
    const int link = blockIdx.x, tid = threadIdx.x;
    const RpeLink lk = links[link];
    const long long om = (long long)link * max_matches;
    double Rb[9], tb[3];
    bool zero = true;
#pragma unroll
    for (int e = 0; e < 9; ++e) { Rb[e] = Rb_in[link * 9 + e]; zero = zero && Rb[e] == 0.; }
#pragma unroll
    for (int e = 0; e < 3; ++e) tb[e] = tb_in[link * 3 + e];
    const int code = status[lk.a] != RPE_PAIR_OK ? RPE_BUNDLE_PAIR_FAILED : (zero ? RPE_BUNDLE_SKIPPED : RPE_BUNDLE_OK);
    if (code == RPE_BUNDLE_PAIR_FAILED) {                                    // workgroup-uniform
        for (int i = tid; i < max_matches; i += 256) {
            views[om + i] = 0;
            X0[(om + i) * 3] = 0.; X0[(om + i) * 3 + 1] = 0.; X0[(om + i) * 3 + 2] = 0.;
        }
        if (tid < 24) pose0[link * 24 + tid] = 0.;
        if (tid < 2) focal[link * 2 + tid] = 0.;
        if (tid == 0) { pre[link] = code; n_in[link] = 0; }
        return;
    }
    const bool a2 = (lk.side & 1) != 0, b2 = (lk.side & 2) != 0;
    const int na = min(m_n[lk.a], max_matches), nb = min(m_n[lk.b], max_matches);
    const long long oa = (long long)lk.a * max_matches, ob = (long long)lk.b * max_matches;
    const int *key_a = (a2 ? m_t : m_q) + oa, *key_b = (b2 ? m_t : m_q) + ob;
    link_join<false>(s_ba_tab, kcap, key_a, na, oa, key_b, nb, ob, ransac_mask, pose_mask);
    double Ra[9], ta[3], RtC[LP_POSE_DOUBLES];
#pragma unroll
    for (int e = 0; e < 9; ++e) Ra[e] = Rall[lk.a * 9 + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) ta[e] = tall[lk.a * 3 + e];
    {   // the solved form of C: S -> C
        double Ri[9], ti[3];
        ba_invert(Rb, tb, Ri, ti);
#pragma unroll
        for (int e = 0; e < 9; ++e) RtC[e] = b2 ? Ri[e] : Rb[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) RtC[9 + e] = b2 ? ti[e] : tb[e];
    }
    const double fa = rpe_pair_focal<CAM>(K, cam, lk.a), fc = rpe_pair_focal<CAM>(K, cam, lk.b);
    const double thr = threshold_px / fc, thr2 = thr * thr;
    const double2 *oS = (a2 ? n2 : n1) + oa, *oA = (a2 ? n1 : n2) + oa, *oC = (b2 ? n1 : n2) + ob;
    for (int i = tid; i < max_matches; i += 256) {
        int v = 0;
        double X[3] = {0., 0., 0.};
        if (i < na && ransac_mask[oa + i] && pose_mask[oa + i]) {
            const int key = key_a[i];
            const unsigned e = (unsigned)key < (unsigned)kcap ? s_ba_tab[key] : 0xFFFFFFFFu;
            if ((e >> 16) == (unsigned)i) {
                v = 1;
                link_point(points + (oa + i) * 3, Ra, ta, a2, X[0], X[1], X[2]);
                double *o = obs + (om + i) * 6;
                const double2 s = oS[i], a = oA[i];
                o[0] = s.x; o[1] = s.y; o[2] = a.x; o[3] = a.y;
                if ((e & 0xFFFFu) != LINK_NONE) {
                    const double2 c = oC[e & 0xFFFFu];
                    const double q[2] = {c.x, c.y};
                    o[4] = c.x; o[5] = c.y;
                    if (lp_inlier(RtC, X, q, thr2)) v = 3;
                }
            }
        }
        views[om + i] = (uint8_t)v;
        X0[(om + i) * 3] = X[0]; X0[(om + i) * 3 + 1] = X[1]; X0[(om + i) * 3 + 2] = X[2];
    }
    if (tid == 0) {
        double Ri[9], ti[3];
        ba_invert(Ra, ta, Ri, ti);
        double *o = pose0 + link * 24;
#pragma unroll
        for (int e = 0; e < 9; ++e) { o[e] = a2 ? Ri[e] : Ra[e]; o[12 + e] = RtC[e]; }
#pragma unroll
        for (int e = 0; e < 3; ++e) { o[9 + e] = a2 ? ti[e] : ta[e]; o[21 + e] = RtC[9 + e]; }
        focal[link * 2] = fa; focal[link * 2 + 1] = fc;
        pre[link] = code; n_in[link] = na;
    }
}

// links == nullptr: the stage form, results in the solved form and in S's frame.  Otherwise the results go back into the
// two pairs' own conventions and pair a's camera-1 frame, and a rejected bundle returns the run's own poses and points
// (src_points / Rall / tall of pair a) and the caller's pose of pair b (Rb_in / tb_in).
__global__ __launch_bounds__(256) void bundle_kernel(const int *__restrict__ n_in, const int *__restrict__ pre, uint8_t *__restrict__ views,
                                                      const double *__restrict__ obs, double *__restrict__ points,
                                                      const double *__restrict__ pose0, const double *__restrict__ focal,
                                                      int min_shared, int max_iters, int max_matches, double *__restrict__ state,
                                                      const RpeLink *__restrict__ links, const double *__restrict__ src_points,
                                                      const double *__restrict__ Rall, const double *__restrict__ tall,
                                                      const double *__restrict__ Rb_in, const double *__restrict__ tb_in,
                                                      double *__restrict__ Ra_out, double *__restrict__ ta_out, double *__restrict__ Rb_out,
                                                      double *__restrict__ tb_out, int *__restrict__ counts, int *__restrict__ info,
                                                      double *__restrict__ rms)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_ba[];
    __shared__ double s_red[4 * BA_NRED], s_lin[BA_NLIN];
    __shared__ int s_wc[4];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const long long om = (long long)prob * max_matches;
    double *sX = state ? state + om * 6 : (double *)s_ba, *sXn = sX + 3 * (size_t)max_matches;     // [n][3] each
    unsigned short *s_idx = (unsigned short *)(s_ba + (state ? 0 : sizeof(double) * 6 * (size_t)max_matches));
    const int M = min(max(n_in[prob], 0), max_matches);
    uint8_t *vw = views + om;
    double *pts = points + om * 3;
    const double *ob = obs + om * 6;
    // ---- the points in index order, their state, the counts
    int n = 0, n3 = 0;
    for (int i0 = 0; i0 < M; i0 += 256) {
        const int i = i0 + tid;
        const int v = i < M ? vw[i] : 0;
        const int pos = ordered_slot(v != 0, s_wc, n);
        (void)ordered_slot(v == 3, s_wc, n3);
        if (v != 0) {
            s_idx[pos] = (unsigned short)i;
            sX[3 * pos] = pts[3 * i]; sX[3 * pos + 1] = pts[3 * i + 1]; sX[3 * pos + 2] = pts[3 * i + 2];
        }
    }
    __syncthreads();                                                         // the list is complete
    int code = pre[prob];
    if (code == RPE_BUNDLE_OK && n3 < max(min_shared, 6)) code = RPE_BUNDLE_TOO_FEW;
    if (code != RPE_BUNDLE_OK) {                                             // workgroup-uniform
        for (int i = tid; i < max_matches; i += 256) { vw[i] = 0; pts[3 * i] = 0.; pts[3 * i + 1] = 0.; pts[3 * i + 2] = 0.; }
        if (tid < 9) { Ra_out[prob * 9 + tid] = 0.; Rb_out[prob * 9 + tid] = 0.; }
        if (tid < 3) { ta_out[prob * 3 + tid] = 0.; tb_out[prob * 3 + tid] = 0.; }
        if (tid < 2) rms[prob * 2 + tid] = 0.;
        if (tid == 0) {
            counts[prob * 2] = n; counts[prob * 2 + 1] = n3;
            info[prob * 4] = code; info[prob * 4 + 1] = 0; info[prob * 4 + 2] = 0; info[prob * 4 + 3] = 0;
        }
        return;
    }
    double RA[9], tA[3], RC[9], tC[3], RCn[9], tCn[3], b1[3], b2[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) { RA[e] = pose0[prob * 24 + e]; RC[e] = pose0[prob * 24 + 12 + e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) { tA[e] = pose0[prob * 24 + 9 + e]; tC[e] = pose0[prob * 24 + 21 + e]; }
    const double fa = focal[prob * 2], fc = focal[prob * 2 + 1];
    double lam = 0.;                                                         // the damping solve() met last: trial() builds the same blocks
    auto point = [&](int j, BaPoint &p) {
        const int i = s_idx[j];
        ba_point(RA, tA, b1, b2, RC, tC, fa, fc, sX + 3 * j, ob + 6 * i, vw[i] == 3, p);
    };
    // also leaves the tangent basis at tA in (b1, b2)
    auto linearise = [&]() {
        refine_basis(tA, b1, b2);
        double s[BA_NLIN];
#pragma unroll
        for (int k = 0; k < BA_NLIN; ++k) s[k] = 0.;
        for (int j = tid; j < n; j += 256) {
            BaPoint p;
            point(j, p);
            int q = 0;
#pragma unroll
            for (int u = 0; u < 5; ++u)
#pragma unroll
                for (int v = u; v < 5; ++v, ++q) s[q] += p.JA[0][u] * p.JA[0][v] + p.JA[1][u] * p.JA[1][v];
#pragma unroll
            for (int u = 0; u < 6; ++u)
#pragma unroll
                for (int v = u; v < 6; ++v, ++q) s[q] += p.JC[0][u] * p.JC[0][v] + p.JC[1][u] * p.JC[1][v];
#pragma unroll
            for (int u = 0; u < 5; ++u) s[36 + u] += p.JA[0][u] * p.e[2] + p.JA[1][u] * p.e[3];
#pragma unroll
            for (int u = 0; u < 6; ++u) s[41 + u] += p.JC[0][u] * p.e[4] + p.JC[1][u] * p.e[5];
            s[47] += ba_cost(p.e);
        }
        block_sum_f64<BA_NLIN>(s, s_red, tid);
        __syncthreads();                                                     // readers of the previous s_lin are done
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < BA_NLIN; ++k) s_lin[k] = s[k];
        }
        __syncthreads();
    };
    // the reduced camera system (U + lambda diag U) - sum W V^-1 W', right-hand side g_c - sum W V^-1 g_p
    auto solve = [&](double lambda, double (&d)[11]) {
        lam = lambda;
        double r[BA_NRED];
#pragma unroll
        for (int k = 0; k < BA_NRED; ++k) r[k] = 0.;
        for (int j = tid; j < n; j += 256) {
            BaPoint p;
            point(j, p);
            double Vi[6], gp[3], W[11][3];
            if (!ba_block(p, lambda, Vi, gp, W)) { r[77] += 1.; continue; }
            int q = 0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double Y[3] = {ba_sym_row(Vi, 0, W[k]), ba_sym_row(Vi, 1, W[k]), ba_sym_row(Vi, 2, W[k])};
#pragma unroll
                for (int l = k; l < 11; ++l, ++q) r[q] += (Y[0] * W[l][0] + Y[1] * W[l][1]) + Y[2] * W[l][2];
                r[66 + k] += (Y[0] * gp[0] + Y[1] * gp[1]) + Y[2] * gp[2];
            }
        }
        block_sum_f64<BA_NRED>(r, s_red, tid);
        if (r[77] != 0.) return false;
        double g[11];
        int q = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
#pragma unroll
            for (int l = k; l < 11; ++l, ++q) {
                double u = 0.;                                               // no residual sees both cameras
                if (k < 5 && l < 5) u = s_lin[k * 5 - k * (k - 1) / 2 + (l - k)];
                if (k >= 5) u = s_lin[15 + (k - 5) * 6 - (k - 5) * (k - 6) / 2 + (l - k)];
                if (l == k) u = u + lambda * u;
                r[q] = u - r[q];
            }
            g[k] = s_lin[36 + k] - r[66 + k];
        }
        return refine_solve<11>(r, g, 0., d);
    };
    // RA <- exp([w]x) RA, tA <- normalise(tA + d3 b1 + d4 b2), RC <- exp([w']x) RC, tC <- tC + d', X <- X + d_p
    auto trial = [&](const double (&d)[11], double (&RAn)[9], double (&tAn)[3]) {
        refine_rotate(d, RA, RAn);
#pragma unroll
        for (int e = 0; e < 3; ++e) tAn[e] = (tA[e] + d[3] * b1[e]) + d[4] * b2[e];
        const double nt = sqrt((tAn[0] * tAn[0] + tAn[1] * tAn[1]) + tAn[2] * tAn[2]);
        tAn[0] /= nt; tAn[1] /= nt; tAn[2] /= nt;
        refine_rotate(d + 5, RC, RCn);
#pragma unroll
        for (int e = 0; e < 3; ++e) tCn[e] = tC[e] + d[8 + e];
        double c = 0.;
        for (int j = tid; j < n; j += 256) {
            BaPoint p;
            point(j, p);
            double Vi[6], gp[3], W[11][3];
            ba_block(p, lam, Vi, gp, W);
            double u[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double a = gp[i];
#pragma unroll
                for (int k = 0; k < 11; ++k) a += W[k][i] * d[k];
                u[i] = a;
            }
            double Xn[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { Xn[i] = sX[3 * j + i] - ba_sym_row(Vi, i, u); sXn[3 * j + i] = Xn[i]; }
            const double *q = ob + 6 * s_idx[j];
            double e[6];
            e[0] = fa * (Xn[0] / Xn[2] - q[0]); e[1] = fa * (Xn[1] / Xn[2] - q[1]);
            lp_residual<false>(RAn, tAn, fa, Xn, q + 2, e[2], e[3], nullptr, nullptr);
            e[4] = 0.; e[5] = 0.;
            if (vw[s_idx[j]] == 3) lp_residual<false>(RCn, tCn, fc, Xn, q + 4, e[4], e[5], nullptr, nullptr);
            c += ba_cost(e);
        }
        return c;
    };
    // a thread owns the same points in every pass: no barrier between its trial and its commit
    auto commit = [&]() {
#pragma unroll
        for (int e = 0; e < 9; ++e) RC[e] = RCn[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) tC[e] = tCn[e];
        for (int j = tid; j < n; j += 256) { sX[3 * j] = sXn[3 * j]; sX[3 * j + 1] = sXn[3 * j + 1]; sX[3 * j + 2] = sXn[3 * j + 2]; }
    };
    linearise();
    const double cost0 = s_lin[47];
    double cost = cost0;
    int iters = 0, acc = 0;
    if (isfinite(cost0)) refine_lm<11>(RA, tA, cost, max_iters, s_red, linearise, solve, trial, commit, iters, acc);
    // ---- the bundled state is returned only if a step was accepted, it is finite and every point lies in front of its views
    double bad[1] = {0.};
    if (acc > 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) if (!hg_finite(RA[e]) || !hg_finite(RC[e])) bad[0] = 1.;
#pragma unroll
        for (int e = 0; e < 3; ++e) if (!hg_finite(tA[e]) || !hg_finite(tC[e])) bad[0] = 1.;
        for (int j = tid; j < n; j += 256) {
            const double *X = sX + 3 * j;
            const double zA = ((RA[6] * X[0] + RA[7] * X[1]) + RA[8] * X[2]) + tA[2], zC = ((RC[6] * X[0] + RC[7] * X[1]) + RC[8] * X[2]) + tC[2];
            bool ok = hg_finite(X[0]) && hg_finite(X[1]) && hg_finite(X[2]) && X[2] > 0. && zA > 0.;
            if (vw[s_idx[j]] == 3) ok = ok && zC > 0.;
            if (!ok) bad[0] += 1.;
        }
        block_sum_f64<1>(bad, s_red, tid);
    }
    const bool take = acc > 0 && bad[0] == 0.;
    const int nobs = 2 * n + n3;
    // ---- outputs
    int sa = 0, sb = 0, pa = 0;
    if (links) { const RpeLink lk = links[prob]; sa = lk.side & 1; sb = lk.side & 2; pa = lk.a; }
    if (take) {
        for (int j = tid; j < n; j += 256) {
            const double *X = sX + 3 * j;
            double *o = pts + 3 * s_idx[j];
            if (sa) {                                                        // pair a's camera 1 is A
#pragma unroll
                for (int r = 0; r < 3; ++r) o[r] = ((RA[3 * r] * X[0] + RA[3 * r + 1] * X[1]) + RA[3 * r + 2] * X[2]) + tA[r];
            } else { o[0] = X[0]; o[1] = X[1]; o[2] = X[2]; }
        }
    } else if (links) {
        for (int j = tid; j < n; j += 256) {
            const int i = s_idx[j];
            const double *P = src_points + ((long long)pa * max_matches + i) * 3;
            pts[3 * i] = P[0]; pts[3 * i + 1] = P[1]; pts[3 * i + 2] = P[2];
        }
    }
    if (tid == 0) {
        double Ro[9], to[3], Ri[9], ti[3];
        if (take || !links) {
            if (!take) {
#pragma unroll
                for (int e = 0; e < 9; ++e) { RA[e] = pose0[prob * 24 + e]; RC[e] = pose0[prob * 24 + 12 + e]; }
#pragma unroll
                for (int e = 0; e < 3; ++e) { tA[e] = pose0[prob * 24 + 9 + e]; tC[e] = pose0[prob * 24 + 21 + e]; }
            }
            ba_invert(RA, tA, Ri, ti);
#pragma unroll
            for (int e = 0; e < 9; ++e) Ro[e] = sa ? Ri[e] : RA[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) to[e] = sa ? ti[e] : tA[e];
#pragma unroll
            for (int e = 0; e < 9; ++e) Ra_out[prob * 9 + e] = Ro[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) ta_out[prob * 3 + e] = to[e];
            ba_invert(RC, tC, Ri, ti);
#pragma unroll
            for (int e = 0; e < 9; ++e) Rb_out[prob * 9 + e] = sb ? Ri[e] : RC[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) tb_out[prob * 3 + e] = sb ? ti[e] : tC[e];
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) { Ra_out[prob * 9 + e] = Rall[pa * 9 + e]; Rb_out[prob * 9 + e] = Rb_in[prob * 9 + e]; }
#pragma unroll
            for (int e = 0; e < 3; ++e) { ta_out[prob * 3 + e] = tall[pa * 3 + e]; tb_out[prob * 3 + e] = tb_in[prob * 3 + e]; }
        }
        counts[prob * 2] = n; counts[prob * 2 + 1] = n3;
        info[prob * 4] = take ? RPE_BUNDLE_OK : RPE_BUNDLE_REJECTED; info[prob * 4 + 1] = iters; info[prob * 4 + 2] = acc; info[prob * 4 + 3] = 0;
        const double before = sqrt(cost0 / nobs);
        rms[prob * 2] = before;
        rms[prob * 2 + 1] = take ? sqrt(cost / nobs) : before;
    }
}

// dynamic LDS of bundle_kernel: the point state up to the cut, then the index list
static size_t bundle_lds(int mm) { return (mm <= BA_LDS_MATCHES ? sizeof(double) * 6 * (size_t)mm : 0) + sizeof(unsigned short) * (size_t)((mm + 7) & ~7); }

// the point state of this handle fits the kernel's LDS (else the callers create d_ba_state)
bool rpe_bundles_in_lds(const rpe_handle *h) { return h->cfg.max_matches <= BA_LDS_MATCHES; }

// n problems whose arrays are in d_ba_* (the stage form uploaded them, or the gather below wrote them) -> d_ba_* results
void rpe_launch_bundle(rpe_handle *h, int n, int min_shared, int max_iters, bool links)
{
    const int mm = h->cfg.max_matches;
    hipLaunchKernelGGL(bundle_kernel, dim3(n), dim3(256), bundle_lds(mm), h->stream, (const int *)h->d_ba_n, (const int *)h->d_ba_pre,
                       h->d_ba_views, (const double *)h->d_ba_obs, h->d_ba_points, (const double *)h->d_ba_pose0, (const double *)h->d_ba_focal,
                       min_shared, max_iters, mm, mm <= BA_LDS_MATCHES ? (double *)nullptr : h->d_ba_state,
                       links ? (const RpeLink *)h->d_links : (const RpeLink *)nullptr, (const double *)h->d_points,
                       (const double *)h->d_R, (const double *)h->d_t, (const double *)h->d_ba_Rin, (const double *)h->d_ba_tin,
                       h->d_ba_Ra, h->d_ba_ta, h->d_ba_Rb, h->d_ba_tb, h->d_ba_counts, h->d_ba_info, h->d_ba_rms);
}

// the links in d_links over the last run r, the callers' poses of pair b in d_ba_Rin / d_ba_tin -> the problems' arrays
int rpe_launch_bundle_gather(rpe_handle *h, const RpeRun &r, int L, double threshold_px)
{
    const int mm = h->cfg.max_matches, kcap = h->lay.kcap;
    const size_t lds = sizeof(unsigned) * (size_t)kcap;
    // the table is all of the kernel's LDS: the largest (uncapped SIFT, 16384 entries) is exactly the 64 KB a kernel gets
    // without the function attribute
    if (lds > 65536) return RPE_ERR_HIP;
    launch_cam(r, bundle_gather_kernel<true>, bundle_gather_kernel<false>, dim3(L), dim3(256), lds, h->stream, (const RpeLink *)h->d_links,
               (const int *)h->d_m_q, (const int *)h->d_m_t, (const int *)h->d_m_n, (const int *)h->d_status,
               (const uint8_t *)h->d_mask, (const uint8_t *)h->d_pose_mask, (const double *)h->d_points,
               (const double *)h->d_R, (const double *)h->d_t, (const double2 *)h->d_n1, (const double2 *)h->d_n2,
               (const double *)h->d_K, r.cam, (const double *)h->d_ba_Rin, (const double *)h->d_ba_tin, threshold_px, mm, kcap,
               h->d_ba_views, h->d_ba_obs, h->d_ba_points, h->d_ba_pose0, h->d_ba_focal, h->d_ba_pre, h->d_ba_n);
    return RPE_OK;
}
