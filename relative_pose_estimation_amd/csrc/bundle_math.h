// bundle_math.h -- the f64 mathematics that pose refinement, link poses, link bundles, track points, window bundles and pose
// graphs share: a view's rows, the point block, the scalar Cholesky factor and solve (bm_chol, bm_chol_solve, and refine_solve
// over them: the only ones of the per-lane code) and the rule of the Levenberg-Marquardt loop.  Written so that a GPU lane and
// the host (tests/native/bundle_math_host.cpp) run the same statements: nothing of HIP or the handle, no barrier, no thread
// index, no intrinsic.  Every caller is built with -ffp-contract=off and compared with a Python model
// (tests/bundle_math_model.py is this header's twin) bit for bit: the association of every expression is the contract; the
// order of a caller's rows, views, points is its own.
#pragma once
#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define BM_INLINE __device__ __forceinline__
#else
#define BM_INLINE static inline
#endif

#define REFINE_LAMBDA0 1e-3          // initial damping
#define REFINE_REL_TOL 1e-6          // stop when an accepted step lowers the cost by no more than this fraction
#define REFINE_STEP_TOL 1e-9         // ... or the step is no longer than this
#define REFINE_SMALL_ANGLE 1e-4      // Rodrigues: series for sin(th)/th and (1 - cos th)/th^2 below this angle

BM_INLINE bool bm_finite(double v) { return fabs(v) <= DBL_MAX; }

// One view of X: y = R X + t, the projection u = y / y2 and the residual (ex, ey) = scale (u - q) in pixels; yu, when given,
// receives y2, u0, u1.  With JAC, Jx[6] and Jy[6] receive the derivatives of ex and ey by (w0 w1 w2 | d0 d1 d2), where
// R <- exp([w]x) R and t <- t + d: d y / d w_k = e_k x (R X), d y / d d = I.  Without, they are not touched (nullptr will do)
template <bool JAC>
BM_INLINE void bm_view(const double *R, const double *t, double scale, const double *X, double qx, double qy, double &ex, double &ey,
                       double *Jx, double *Jy, double *yu = nullptr)
{
    const double a0 = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], a1 = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2];
    const double a2 = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
    const double y0 = a0 + t[0], y1 = a1 + t[1], y2 = a2 + t[2];
    const double ux = y0 / y2, uy = y1 / y2;
    ex = scale * (ux - qx); ey = scale * (uy - qy);
    if (yu) { yu[0] = y2; yu[1] = ux; yu[2] = uy; }
    if (JAC) {
        const double s = scale / y2;
        Jx[0] = -s * (ux * a1); Jx[1] = s * (a2 + ux * a0); Jx[2] = -s * a1; Jx[3] = s; Jx[4] = 0.; Jx[5] = -s * ux;
        Jy[0] = -s * (a2 + uy * a1); Jy[1] = s * (uy * a0); Jy[2] = s * a0; Jy[3] = 0.; Jy[4] = s; Jy[5] = -s * uy;
    }
}

// The rows by the point: the d columns of bm_view's rows times the view's rotation
BM_INLINE void bm_point_rows(const double *Jx, const double *Jy, const double *R, double (&JXx)[3], double (&JXy)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        JXx[k] = (Jx[3] * R[k] + Jx[4] * R[3 + k]) + Jx[5] * R[6 + k];
        JXy[k] = (Jy[3] * R[k] + Jy[4] * R[3 + k]) + Jy[5] * R[6 + k];
    }
}

// One row J of Jp with its residual e, added to the point block V = Jp'Jp (upper triangle 00 01 02 11 12 22) and to g_p = Jp'e
BM_INLINE void bm_block_row(const double (&J)[3], double e, double (&v)[6], double (&gp)[3])
{
    v[0] += J[0] * J[0]; v[1] += J[0] * J[1]; v[2] += J[0] * J[2];
    v[3] += J[1] * J[1]; v[4] += J[1] * J[2]; v[5] += J[2] * J[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[i] += J[i] * e;
}

// Vi = (V + lambda diag V)^-1 by the adjugate; v is damped in place.  False when V is singular (Vi is then not to be used)
BM_INLINE bool bm_damped_inverse(double (&v)[6], double lambda, double (&Vi)[6])
{
    v[0] = v[0] + lambda * v[0]; v[3] = v[3] + lambda * v[3]; v[5] = v[5] + lambda * v[5];
    const double c00 = v[3] * v[5] - v[4] * v[4], c01 = v[2] * v[4] - v[1] * v[5], c02 = v[1] * v[4] - v[2] * v[3];
    const double c11 = v[0] * v[5] - v[2] * v[2], c12 = v[1] * v[2] - v[0] * v[4], c22 = v[0] * v[3] - v[1] * v[1];
    const double det = (v[0] * c00 + v[1] * c01) + v[2] * c02;
    Vi[0] = c00 / det; Vi[1] = c01 / det; Vi[2] = c02 / det; Vi[3] = c11 / det; Vi[4] = c12 / det; Vi[5] = c22 / det;
    return det > 0. && bm_finite(det);
}

// row i of the symmetric 3 x 3 held as its upper triangle (00 01 02 11 12 22), times u
BM_INLINE double bm_sym_row(const double (&S)[6], int i, const double (&u)[3])
{
    const double a = i == 0 ? S[0] : (i == 1 ? S[1] : S[2]), b = i == 0 ? S[1] : (i == 1 ? S[3] : S[4]);
    const double c = i == 0 ? S[2] : (i == 1 ? S[4] : S[5]);
    return (a * u[0] + b * u[1]) + c * u[2];
}

// ---------------------------------------------------------------- the Cholesky solve, the only one of the scalar code
// A symmetric N x N matrix travels as its lower triangle, packed by rows: N (N + 1) / 2 entries, entry (i, k) at bm_tri(i, k)
BM_INLINE constexpr int bm_tri(int i, int k) { return i * (i + 1) / 2 + k; }   // k <= i

// H = L L' by columns, in place: L holds H's lower triangle on entry and the factor on return.  The pivot of column c is
// H(c, c) minus L(c, k)^2 for k = 0 .. c - 1, each subtracted serially in ascending k, then its square root; the entry
// (r, c) below it is H(r, c) minus L(r, k) L(c, k), subtracted the same way, divided by the pivot's root.  False when a
// pivot is not > 0 or not finite (bm_finite); L is then not to be used.  The factorisation carries on behind such a pivot
// instead of returning: a return inside the unrolled columns keeps every later column's operands alive across the branch
// (pose_refine_kernel 167 -> 231 / 255 VGPRs, tp_solve_kernel 126 -> 154: profiles/r25_kernel_resources.md).
template <int N>
BM_INLINE bool bm_chol(double (&L)[N * (N + 1) / 2])
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        double s = L[bm_tri(c, c)];
#pragma unroll
        for (int k = 0; k < c; ++k) s = s - L[bm_tri(c, k)] * L[bm_tri(c, k)];
        if (!(s > 0.) || !bm_finite(s)) ok = false;
        const double d = sqrt(s);
        L[bm_tri(c, c)] = d;
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            double v = L[bm_tri(r, c)];
#pragma unroll
            for (int k = 0; k < c; ++k) v = v - L[bm_tri(r, k)] * L[bm_tri(c, k)];
            L[bm_tri(r, c)] = v / d;
        }
    }
    return ok;
}

// z = (L L')^-1 r: forward (y_i = (r_i - sum_{k < i} L(i, k) y_k) / L(i, i), i ascending), then back (z_i = (y_i -
// sum_{k > i} L(k, i) z_k) / L(i, i), i descending), each inner sum subtracted serially in ascending k
template <int N>
BM_INLINE void bm_chol_solve(const double (&L)[N * (N + 1) / 2], const double (&r)[N], double (&z)[N])
{
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[bm_tri(i, k)] * y[k];
        y[i] = v / L[bm_tri(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v = v - L[bm_tri(k, i)] * z[k];
        z[i] = v / L[bm_tri(i, i)];
    }
}

// (H + lambda diag H) d = -g for N parameters, H given as its upper triangle (row-major, N (N + 1) / 2 entries), the
// diagonal damped as h + lambda * h, by bm_chol and bm_chol_solve with the right-hand side -g; false when the damped matrix
// is not positive definite (d is then not to be used).  Serves pose_refine_kernel (N = 5), link_pose_kernel (6),
// bundle_kernel (11) and tp_solve_kernel (3)
template <int N>
BM_INLINE bool refine_solve(const double *H, const double *g, double lambda, double *d)
{
    double L[N * (N + 1) / 2], r[N], z[N];
    int q = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j, ++q) L[bm_tri(j, i)] = H[q];
#pragma unroll
    for (int i = 0; i < N; ++i) { L[bm_tri(i, i)] = L[bm_tri(i, i)] + lambda * L[bm_tri(i, i)]; r[i] = -g[i]; }
    const bool ok = bm_chol<N>(L);
    bm_chol_solve<N>(L, r, z);
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = z[i];
    return ok;
}

// the length of a step of n parameters: d[0]^2 first, then ascending adds (d: anything indexable)
template <class D>
BM_INLINE double lm_step_norm(const D &d, int n)
{
    double dn = d[0] * d[0];
    for (int k = 1; k < n; ++k) dn = dn + d[k] * d[k];
    return sqrt(dn);
}

// The Levenberg-Marquardt acceptance rule, and nothing else.  The state, its step and its trial state are the caller's:
//   step(lambda)    forms the damped step at the caller's state; false when there is none
//   trial(lambda)   forms the trial state and returns its cost, summed over whoever takes part; non-finite vetoes the trial
//   step_norm()     the length of the step (lm_step_norm); called for an accepted step only, before accept()
//   accept()        the trial state becomes the state
// A missing step or a trial that does not strictly lower the cost multiplies lambda by 10; an accepted step divides it by
// 10, moves the cost and stops the loop when it lowered the cost by no more than REFINE_REL_TOL of it or is no longer than
// REFINE_STEP_TOL.  iters counts the iterations begun, acc the steps accepted (both are added to).
template <class Step, class Trial, class StepNorm, class Accept>
BM_INLINE void lm_loop(double &cost, int max_iters, Step step, Trial trial, StepNorm step_norm, Accept accept, int &iters, int &acc)
{
    double lambda = REFINE_LAMBDA0;
    for (int it = 0; it < max_iters; ++it) {
        ++iters;
        if (!step(lambda)) { lambda = lambda * 10.; continue; }
        const double c1 = trial(lambda);
        if (bm_finite(c1) && c1 < cost) {
            const double dec = cost - c1, prev = cost, dn = step_norm();
            accept();
            cost = c1; lambda = lambda / 10.; ++acc;
            if (dec <= REFINE_REL_TOL * prev || dn <= REFINE_STEP_TOL) break;
        } else {
            lambda = lambda * 10.;
        }
    }
}
