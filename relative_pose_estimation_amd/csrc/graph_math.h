// graph_math.h -- what one lane of pg_solve_kernel (graph_kernels.hip) computes, written like bundle_math.h so that a GPU lane
// and the host (tests/native/graph_math_host.cpp) run the same statements: nothing of HIP or the handle, no barrier, no thread
// index, no intrinsic.  The rule is include/rpe_amd.h, "pose graphs"; every caller is built with -ffp-contract=off and compared
// with tests/pose_graph_model.py bit for bit, so the association of every expression here is the contract.  All f64,
// + - * / sqrt only.  Every sum starts at +0.0 and adds its terms in ascending order; a 3-vector dot product is
// (a0*b0 + a1*b1) + a2*b2.  The factor and the solve of a frame's 6 x 6 block are bundle_math.h's bm_chol<6> and
// bm_chol_solve<6>, with their order of operations.
#pragma once
#include "bundle_math.h"

#define GM_EDGE_METRIC 0
#define GM_EDGE_DIRECTION 1

BM_INLINE double gm_dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// The 12 rows of an edge and their derivatives by (w | d) of frame i and of frame j.  The d columns of the nine rotation rows
// are structurally zero and are not held: W[row][c] is the derivative of row 0 .. 11 by w_c, D[t][c] that of translation
// row 9 + t by d_c
struct GmEdge {
    double r[12];
    double JiW[12][3], JjW[12][3], JiD[3][3], JjD[3][3];
};

// Frame i (Ri, Ti), frame j (Rj, Tj), the measurement X_j = M X_i + m, the weights and the kind.  Without JAC only r is written
template <bool JAC>
BM_INLINE void gm_edge_rows(const double *Ri, const double *Ti, const double *Rj, const double *Tj, const double *M, const double *m,
                            double w_rot, double w_trans, int kind, GmEdge &e)
{
    double Q[9], D[9], qt[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Q[r * 3 + c] = gm_dot3(Rj[r * 3], Rj[r * 3 + 1], Rj[r * 3 + 2], Ri[c * 3], Ri[c * 3 + 1], Ri[c * 3 + 2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        qt[r] = gm_dot3(Q[r * 3], Q[r * 3 + 1], Q[r * 3 + 2], Ti[0], Ti[1], Ti[2]);
        p[r] = Tj[r] - qt[r];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) D[r * 3 + c] = gm_dot3(Q[r * 3], Q[r * 3 + 1], Q[r * 3 + 2], M[c * 3], M[c * 3 + 1], M[c * 3 + 2]);
    const double a = w_rot / sqrt(2.);
    // rotation rows: column k of a (D - I); by w_j: -a [D_k]x; by w_i: a D [e_k]x M
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) e.r[3 * k + r] = a * (D[r * 3 + k] - (r == k ? 1. : 0.));
        if (JAC) {
            const double v0 = a * D[k], v1 = a * D[3 + k], v2 = a * D[6 + k];
            e.JjW[3 * k][0] = 0.;      e.JjW[3 * k][1] = v2;      e.JjW[3 * k][2] = -v1;
            e.JjW[3 * k + 1][0] = -v2; e.JjW[3 * k + 1][1] = 0.;  e.JjW[3 * k + 1][2] = v0;
            e.JjW[3 * k + 2][0] = v1;  e.JjW[3 * k + 2][1] = -v0; e.JjW[3 * k + 2][2] = 0.;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) e.JiW[3 * k + r][c] = a * (D[r * 3 + k2] * M[k1 * 3 + c] - D[r * 3 + k1] * M[k2 * 3 + c]);
        }
    }
    // p by w_j: [Q T_i]x; by w_i: -Q [T_i]x; by d_j: I; by d_i: -Q
    double Pj[3][3], Pi[3][3];
    if (JAC) {
        Pj[0][0] = 0.;     Pj[0][1] = -qt[2]; Pj[0][2] = qt[1];
        Pj[1][0] = qt[2];  Pj[1][1] = 0.;     Pj[1][2] = -qt[0];
        Pj[2][0] = -qt[1]; Pj[2][1] = qt[0];  Pj[2][2] = 0.;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Pi[r][0] = Q[r * 3 + 2] * Ti[1] - Q[r * 3 + 1] * Ti[2];
            Pi[r][1] = Q[r * 3] * Ti[2] - Q[r * 3 + 2] * Ti[0];
            Pi[r][2] = Q[r * 3 + 1] * Ti[0] - Q[r * 3] * Ti[1];
        }
    }
    if (kind == GM_EDGE_METRIC) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            e.r[9 + r] = w_trans * (p[r] - m[r]);
            if (JAC) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    e.JjW[9 + r][c] = w_trans * Pj[r][c]; e.JiW[9 + r][c] = w_trans * Pi[r][c];
                    e.JjD[r][c] = r == c ? w_trans : 0.; e.JiD[r][c] = -(w_trans * Q[r * 3 + c]);
                }
            }
        }
        return;
    }
    const double n = sqrt(gm_dot3(p[0], p[1], p[2], p[0], p[1], p[2]));
    if (!(n > 0.)) {                                                        // coincident centres (or a NaN): no rows here
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            e.r[9 + r] = 0.;
            if (JAC) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { e.JjW[9 + r][c] = 0.; e.JiW[9 + r][c] = 0.; e.JjD[r][c] = 0.; e.JiD[r][c] = 0.; }
            }
        }
        return;
    }
    const double mn = sqrt(gm_dot3(m[0], m[1], m[2], m[0], m[1], m[2]));
    const double u[3] = {p[0] / n, p[1] / n, p[2] / n};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        e.r[9 + r] = w_trans * (u[r] - m[r] / mn);
        if (JAC) {
            const double N0 = ((r == 0 ? 1. : 0.) - u[r] * u[0]) / n, N1 = ((r == 1 ? 1. : 0.) - u[r] * u[1]) / n;
            const double N2 = ((r == 2 ? 1. : 0.) - u[r] * u[2]) / n;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e.JjW[9 + r][c] = w_trans * gm_dot3(N0, N1, N2, Pj[0][c], Pj[1][c], Pj[2][c]);
                e.JiW[9 + r][c] = w_trans * gm_dot3(N0, N1, N2, Pi[0][c], Pi[1][c], Pi[2][c]);
                e.JjD[r][c] = w_trans * (c == 0 ? N0 : (c == 1 ? N1 : N2));
                e.JiD[r][c] = -(w_trans * gm_dot3(N0, N1, N2, Q[c], Q[3 + c], Q[6 + c]));
            }
        }
    }
}

// The length s of an edge's rows, its Huber weight h and its cost term (huber == 0: off)
BM_INLINE void gm_huber(const double (&r)[12], double huber, double &s, double &h, double &cost)
{
    double s2 = 0.;
#pragma unroll
    for (int k = 0; k < 12; ++k) s2 = s2 + r[k] * r[k];
    s = sqrt(s2);
    const bool plain = huber == 0. || s <= huber;
    h = plain ? 1. : huber / s;
    cost = plain ? s2 : (2. * huber) * s - huber * huber;
}

// Entry [a][b] of h Ja'Jb for a, b in 0 .. 5: the sum over the rows in which neither factor is structurally zero (all 12
// for two w columns, the three translation rows otherwise)
BM_INLINE double gm_block_entry(double h, const double (&AW)[12][3], const double (&AD)[3][3], const double (&BW)[12][3],
                                const double (&BD)[3][3], int a, int b)
{
    double s = 0.;
    if (a < 3 && b < 3) {
#pragma unroll
        for (int r = 0; r < 12; ++r) s = s + AW[r][a] * BW[r][b];
    } else {
#pragma unroll
        for (int t = 0; t < 3; ++t) s = s + (a < 3 ? AW[9 + t][a] : AD[t][a - 3]) * (b < 3 ? BW[9 + t][b] : BD[t][b - 3]);
    }
    return h * s;
}

// Entry a of h J'r
BM_INLINE double gm_grad_entry(double h, const double (&W)[12][3], const double (&D)[3][3], const double (&r)[12], int a)
{
    double s = 0.;
    if (a < 3) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s = s + W[k][a] * r[k];
    } else {
#pragma unroll
        for (int t = 0; t < 3; ++t) s = s + D[t][a - 3] * r[9 + t];
    }
    return h * s;
}

// row a of a 6 x 6 block (row-major) times p, and row a of its transpose times p
BM_INLINE double gm_row6(const double *H, int a, const double (&p)[6])
{
    double s = 0.;
#pragma unroll
    for (int b = 0; b < 6; ++b) s = s + H[a * 6 + b] * p[b];
    return s;
}
BM_INLINE double gm_col6(const double *H, int a, const double (&p)[6])
{
    double s = 0.;
#pragma unroll
    for (int b = 0; b < 6; ++b) s = s + H[b * 6 + a] * p[b];
    return s;
}
BM_INLINE double gm_dot6(const double (&a)[6], const double (&b)[6])
{
    double s = 0.;
#pragma unroll
    for (int k = 0; k < 6; ++k) s = s + a[k] * b[k];
    return s;
}

// The lower triangle of a 6 x 6 block (row-major) as bm_chol<6> takes it (bundle_math.h: the factor and the solve of a
// frame's block are the shared ones)
BM_INLINE void gm_lower6(const double (&H)[36], double (&L)[21])
{
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) L[bm_tri(i, k)] = H[i * 6 + k];
}

// Rn = C(w) R with the Cayley map C = I + (2 / (1 + a.a)) ([a]x + [a]x [a]x), a = w / 2: a rotation for every w
BM_INLINE void gm_cayley(const double (&w)[3], const double *R, double *Rn)
{
    const double a[3] = {w[0] / 2., w[1] / 2., w[2] / 2.};
    const double n2 = gm_dot3(a[0], a[1], a[2], a[0], a[1], a[2]);
    const double f = 2. / (1. + n2);
    double Cm[9];
    Cm[0] = 1. + f * (a[0] * a[0] - n2); Cm[1] = f * (a[0] * a[1] - a[2]);    Cm[2] = f * (a[0] * a[2] + a[1]);
    Cm[3] = f * (a[1] * a[0] + a[2]);    Cm[4] = 1. + f * (a[1] * a[1] - n2); Cm[5] = f * (a[1] * a[2] - a[0]);
    Cm[6] = f * (a[2] * a[0] - a[1]);    Cm[7] = f * (a[2] * a[1] + a[0]);    Cm[8] = 1. + f * (a[2] * a[2] - n2);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = gm_dot3(Cm[r * 3], Cm[r * 3 + 1], Cm[r * 3 + 2], R[c], R[3 + c], R[6 + c]);
}
