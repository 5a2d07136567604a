// pose_triangulate.h -- the one-sided Jacobi SVD and the DLT triangulation of recoverPose, written so that a GPU lane and
// the host (tests/native/triangulate_mirror_host.cpp) run the same statements.
//
//   jacobi_cols<M, N>      one-sided Jacobi (Hestenes) on the columns of A; decomposeEssentialMat, the similarity of
//                          scale_links and the triangulation below all use it
//   triangulate_one        DLT point of one match for one (R, t) and recoverPose's cheirality verdict (distance 50)
//   triangulate_pm         the verdicts of (R, t) AND (R, -t) from ONE SVD
//
// The mirror.  For a fixed R, replacing t by -t negates exactly one column of the DLT matrix: A' = A D, D = diag(1, 1, 1, -1)
// (A[11] = x2 t2 - t0 and A[15] = y2 t2 - t1 change sign, nothing else does).  IEEE negation is exact and round-to-nearest
// is symmetric, with or without fused multiply-add, so every quantity of jacobi_cols<4, 4> on A' is the one on A or its exact
// negative: al, be and c are the same; ga, zeta, t and s are negated for the pairs (p, 3); the convergence test and so the
// sweep count are the same; A'_k = A_k D and V'_k = D V_k D after every rotation.  The column norms are equal, the same
// column j is chosen, and the homogeneous point comes out as (X, Y, Z, -W) (j < 3) or (-X, -Y, -Z, W) (j = 3).  Either way
// Z' W' = -(Z W), the Euclidean point is -P bit for bit and z2' = -z2 bit for bit, so the verdict of -t is four comparisons
// on what the +t triangulation has already computed.
//
// The tie.  One statement is not symmetric: `zeta >= 0. ? 1. : -1.` takes +1 for +0 and for -0.  When a rotation (p, 3)
// meets be == al exactly with ga != 0, both paths rotate by t = +1 and the mirror breaks.  jacobi_cols<4, 4, true> reports
// it; triangulate_pm then triangulates (R, -t) directly.  (Random scenes do not raise it; R = I, t = (-1, -1, 0),
// x1 = y1 = x2 = 0 does: tests/test_triangulate_mirror_cpu.py.)
#pragma once

#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define PT_INLINE __device__ __forceinline__
#define PT_FN __device__ static
#else
#define PT_INLINE static inline
#define PT_FN static
#endif

// one-sided Jacobi (Hestenes) on the columns of A (M x N row-major); V accumulates rotations.  TIE = true: returns
// whether a rotation with the last column met zeta == +-0 (see above); TIE = false: returns false, nothing is tested.
template <int MM, int NN, bool TIE = false>
PT_INLINE bool jacobi_cols(double *A, double *V)
{
    const double eps = DBL_EPSILON * 10;
    bool tie = false;
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = 0; j < NN; ++j) V[i * NN + j] = (i == j) ? 1. : 0.;
    for (int sweep = 0; sweep < 30; ++sweep) {
        int changed = 0;
#pragma unroll
        for (int p = 0; p < NN - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < NN; ++q) {
                double al = 0., be = 0., ga = 0.;
#pragma unroll
                for (int k = 0; k < MM; ++k) {
                    double ap = A[k * NN + p], aq = A[k * NN + q];
                    al += ap * ap; be += aq * aq; ga += ap * aq;
                }
                if (!(fabs(ga) <= eps * sqrt(al * be))) {
                    changed = 1;
                    double zeta = (be - al) / (2. * ga);
                    if constexpr (TIE) { if (q == NN - 1 && zeta == 0.) tie = true; }
                    double t = (zeta >= 0. ? 1. : -1.) / (fabs(zeta) + sqrt(1. + zeta * zeta));
                    double c = 1. / sqrt(1. + t * t), s = c * t;
#pragma unroll
                    for (int k = 0; k < MM; ++k) {
                        double ap = A[k * NN + p], aq = A[k * NN + q];
                        A[k * NN + p] = c * ap - s * aq; A[k * NN + q] = s * ap + c * aq;
                    }
#pragma unroll
                    for (int k = 0; k < NN; ++k) {
                        double vp = V[k * NN + p], vq = V[k * NN + q];
                        V[k * NN + p] = c * vp - s * vq; V[k * NN + q] = s * vp + c * vq;
                    }
                }
            }
        if (!changed) break;
    }
    return tie;
}

// triangulate.cpp DLT with P0 = [I|0], P = [R|t]: the 4 x 4 system of one match ...
PT_INLINE void dlt_matrix(const double *R, const double *t, double x1, double y1, double x2, double y2, double *A)
{
    A[0] = -1.; A[1] = 0.;  A[2] = x1; A[3] = 0.;
    A[4] = 0.;  A[5] = -1.; A[6] = y1; A[7] = 0.;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[8 + k]  = x2 * R[6 + k] - R[k];
        A[12 + k] = y2 * R[6 + k] - R[3 + k];
    }
    A[11] = x2 * t[2] - t[0];
    A[15] = y2 * t[2] - t[1];
}

// ... and its solution after jacobi_cols<4, 4>(A, V): the column of V whose column of A = U S is the shortest (the first
// of equals)
PT_INLINE void dlt_solution(const double *A, const double *V, double &X, double &Y, double &Z, double &W)
{
    double best = 0.;
    X = 0.; Y = 0.; Z = 0.; W = 0.;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double nn = ((A[j] * A[j] + A[4 + j] * A[4 + j]) + A[8 + j] * A[8 + j]) + A[12 + j] * A[12 + j];
        if (j == 0 || nn < best) { best = nn; X = V[j]; Y = V[4 + j]; Z = V[8 + j]; W = V[12 + j]; }
    }
}

// One match, one (R, t): the DLT point and the cheirality test of recoverPose (dist 50).  P receives the point
// (X/W, Y/W, Z/W) in the camera-1 frame, whatever the test says.  recover_pose_kernel (through triangulate_pm, which
// falls back on this routine), pose_structure_kernel and pose_refine_kernel all count with it, so the structure's mask
// sums to the inlier count exactly.
PT_FN int triangulate_one(const double *R, const double *t, double x1, double y1, double x2, double y2, double *P)
{
    double A[16], V[16];
    dlt_matrix(R, t, x1, y1, x2, y2, A);
    jacobi_cols<4, 4>(A, V);
    double X, Y, Z, W;
    dlt_solution(A, V, X, Y, Z, W);
    int good = (Z * W) > 0.;
    X /= W; Y /= W; Z /= W;
    P[0] = X; P[1] = Y; P[2] = Z;
    good = good && (Z < 50.);
    double z2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    good = good && (z2 > 0.) && (z2 < 50.);
    return good;
}

// triangulate_one(R, t, ...) into good_plus and P_plus, and the verdict of triangulate_one(R, -t, ...) into good_minus,
// from one SVD (the mirror above: Z' W' = -(Z W), P' = -P_plus, z2' = -z2).  On the tie the -t hypothesis is triangulated
// directly, so both verdicts are triangulate_one's in every case.  Returns whether the tie occurred; mirror_minus, when
// given, receives the mirrored verdict as it is before the fallback (for the host test).
PT_INLINE bool triangulate_pm(const double *R, const double *t, double x1, double y1, double x2, double y2, int &good_plus,
                              int &good_minus, double *P_plus, int *mirror_minus = nullptr)
{
    double A[16], V[16];
    dlt_matrix(R, t, x1, y1, x2, y2, A);
    const bool tie = jacobi_cols<4, 4, true>(A, V);
    double X, Y, Z, W;
    dlt_solution(A, V, X, Y, Z, W);
    const double zw = Z * W;
    X /= W; Y /= W; Z /= W;
    P_plus[0] = X; P_plus[1] = Y; P_plus[2] = Z;
    const double z2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    good_plus = (zw > 0.) && (Z < 50.) && (z2 > 0.) && (z2 < 50.);
    good_minus = (zw < 0.) && (-Z < 50.) && (-z2 > 0.) && (-z2 < 50.);
    if (mirror_minus) *mirror_minus = good_minus;
    if (tie) {
        const double tn[3] = {-t[0], -t[1], -t[2]};
        double Pn[3];
        good_minus = triangulate_one(R, tn, x1, y1, x2, y2, Pn);
    }
    return tie;
}
