// geom_device.h -- what geom_kernels.hip (pairs) and link_kernels.hip (links) both use, and nothing else: the polynomial
// root chain, the deterministic f64 sums and the ordered compaction, the small 3-vector algebra, the Levenberg-Marquardt
// loop with its parts, and the host helper of their launchers.  A helper one file uses lives in that file; what needs nothing
// of the device (a view's rows, the point block, the Cholesky solve refine_solve, the rule of the loop) is in bundle_math.h,
// which the host tests compile too.
// All f64 arithmetic keeps the oracle's operation order (compiled with -ffp-contract=off).
#pragma once
#include "rpe_internal.h"
#include "bundle_math.h"

// ------------------------------------------------------------ polynomial root chain
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

// ------------------------------------------------------------ workgroup sums, ordered compaction
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

// ------------------------------------------------------------ Levenberg-Marquardt (refine_lm and its parts; lm_loop, refine_solve: bundle_math.h)
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

// The Levenberg-Marquardt loop over N parameters, shared by pose_refine_kernel, link_pose_kernel and bundle_kernel; all 256
// threads call it with identical operands.  lm_loop's rule, arranged for a workgroup whose state is a pose in registers:
//   linearise()        the normal equations at the caller's state, summed over the workgroup (block_sum_f64)
//   solve(lambda, d)   the damped step d from them; false when there is none (a matrix that is not positive definite).
//                      RefineNormalSolve is the plain form: s holds the upper triangle of J'J, then J'r, then r'r
//   trial(d, Rn, tn)   the pose (Rn, tn) that step d leads to from (R, t), and this thread's part of its cost
//   commit()           an accepted step: whatever state the caller keeps outside (R, t) moves with it
// The state is linearised again only when another iteration follows an accepted step (the step hook); the trial hook sums
// the threads' parts, the accept hook moves (R, t) and calls commit().  iters: the iterations begun, acc: the steps accepted.
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
    bool need_lin = false;
    double d[N], Rn[9], tn[3];
    auto step = [&](double lambda) { if (need_lin) { linearise(); need_lin = false; } return solve(lambda, d); };
    auto summed_trial = [&](double) { double c1[1] = {trial(d, Rn, tn)}; block_sum_f64<1>(c1, s_red, threadIdx.x); return c1[0]; };
    auto accept = [&]() {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = Rn[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) t[e] = tn[e];
        commit(); need_lin = true;
    };
    lm_loop(cost, max_iters, step, summed_trial, [&]() { return lm_step_norm(d, N); }, accept, iters, acc);
}

// ------------------------------------------------------------ 3-vectors by reference
__device__ __forceinline__ double hg_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void hg_cross(const double (&a)[3], const double (&b)[3], double (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ bool hg_finite(double v) { return bm_finite(v); }

// ------------------------------------------------------------ host: the launchers' helper
// Launches the camera instance of a kernel when the run carries a camera source, the shared-K instance otherwise (the
// single-K paths launch CAM = false only): the two instances share one signature
template <typename Kernel, typename... Args>
static void launch_cam(const RpeRun &r, Kernel with_cameras, Kernel with_K, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args)
{
    hipLaunchKernelGGL(r.cam.cams ? with_cameras : with_K, grid, block, lds, stream, args...);
}
