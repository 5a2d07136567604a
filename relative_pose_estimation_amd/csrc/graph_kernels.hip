// graph_kernels.hip -- pose graphs (include/rpe_amd.h, "pose graphs"): the poses of a graph's free frames moved onto the
// relative-pose measurements of its edges.  All f64, + - * / sqrt only, in the header's operation order.
//
// One launch on the handle's stream, one workgroup of 256 lanes per graph.  The host (rpe_optimise_graphs, rpe_features.hip, by
// graph_plan.h) has built the active set: the free frames, the used edges, the adjacency of every free frame (its used edges
// in ascending position, one side bit, the free index of the other end) and the codes that need no arithmetic; the kernel
// indexes with these tables without a check of its own, the host tests of graph_plan.h are their check.  Everything of a graph
// lives in the call's device buffers, one path for every size; LDS holds the four wave totals of a reduction only.
//   state        R, T and the trial Rn, Tn per graph position (the state arrays are the output arrays)
//   edge blocks  per used edge 120 f64, component-major ([component][used edge]: lanes of consecutive edges coalesce):
//                h Ji'Ji, h Jj'Jj, h Ji'Jj, h Ji'r, h Jj'r
//   frame block  per free frame 87 f64, component-major: the damped diagonal block, its Cholesky factor and the PCG vectors
// A Levenberg-Marquardt iteration is
//   edges   lane per used edge: rows, Huber weight, blocks (only when the state has moved since the last linearisation)
//   frames  lane per free frame: gather over its adjacency, damp, factor, r = -g, z = M^-1 r, p = z
//   PCG     H p: lane per free frame over its own block and the off-diagonal blocks of its edges (transposed on the j side);
//           three block reductions per iteration (p.Hp, r.z; the step length once per accepted step)
//   trial   the Cayley update of every free frame, then the cost over the used edges
// A barrier separates the phases; every decision is taken on a block-reduced value, so the control flow is uniform.
// What a lane computes is graph_math.h's; the block's Cholesky (bm_chol<6>, bm_chol_solve<6>) and the rule of the loop
// (lm_loop) are bundle_math.h's.
#include "geom_device.h"
#include "graph_math.h"

#define PG_EB 120                  // f64 per used edge
#define PG_EB_JJ 36
#define PG_EB_IJ 72
#define PG_EB_GI 108
#define PG_EB_GJ 114
#define PG_FB 87                   // f64 per free frame
#define PG_FB_L 36
#define PG_FB_R 57
#define PG_FB_Z 63
#define PG_FB_P 69
#define PG_FB_X 75
#define PG_FB_HP 81
static_assert(PG_EB == RPE_GRAPH_EDGE_DOUBLES && PG_EB_GJ + 6 == PG_EB, "pg.eb holds one edge block per used edge");
static_assert(PG_FB == RPE_GRAPH_FRAME_DOUBLES && PG_FB_HP + 6 == PG_FB, "pg.fb holds one frame block per free frame");

struct PgArgs {
    RpeGraphJob job;
    double *R, *T, *Rn, *Tn;       // [9 n], [3 n] with n = graph_start[n_graphs]
    double *eb, *fb;               // [PG_EB * used edges], [PG_FB * free frames]
    double *chi, *cost;            // [2 * edges] (zeroed by the caller), [2 * n_graphs]
    int *info;                     // [4 * n_graphs]
};

// One graph as its workgroup sees it
struct PgGraph {
    int tid, F, nf, nu, es;
    const int *fpos, *uedge, *ei, *ej, *kind;
    const double *eR, *et, *ew;
    double huber;
    double *eb, *chi;
};

// The pass over the used edges at the state (Rs, Ts): the cost, summed by the header's rule; with JAC the edge blocks;
// chi_slot 0 / 1: the edge's s into chi, -1: nowhere
template <bool JAC>
__device__ __forceinline__ double pg_edges(const PgGraph &g, const double *Rs, const double *Ts, int chi_slot, double *s_red)
{
    double c[1] = {0.};
    for (int u = g.tid; u < g.nu; u += 256) {
        const int e = g.es + g.uedge[u], pi = g.ei[e], pj = g.ej[e];
        GmEdge ed;
        gm_edge_rows<JAC>(Rs + 9 * (size_t)pi, Ts + 3 * (size_t)pi, Rs + 9 * (size_t)pj, Ts + 3 * (size_t)pj, g.eR + 9 * (size_t)e,
                          g.et + 3 * (size_t)e, g.ew[2 * (size_t)e], g.ew[2 * (size_t)e + 1], g.kind[e], ed);
        double s, h, ce;
        gm_huber(ed.r, g.huber, s, h, ce);
        c[0] = c[0] + ce;
        if (chi_slot >= 0) g.chi[2 * (size_t)e + chi_slot] = s;
        if (JAC) {
            double *b = g.eb + u;
            const size_t nu = (size_t)g.nu;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    b[(a * 6 + k) * nu] = gm_block_entry(h, ed.JiW, ed.JiD, ed.JiW, ed.JiD, a, k);
                    b[(PG_EB_JJ + a * 6 + k) * nu] = gm_block_entry(h, ed.JjW, ed.JjD, ed.JjW, ed.JjD, a, k);
                    b[(PG_EB_IJ + a * 6 + k) * nu] = gm_block_entry(h, ed.JiW, ed.JiD, ed.JjW, ed.JjD, a, k);
                }
                b[(PG_EB_GI + a) * nu] = gm_grad_entry(h, ed.JiW, ed.JiD, ed.r, a);
                b[(PG_EB_GJ + a) * nu] = gm_grad_entry(h, ed.JjW, ed.JjD, ed.r, a);
            }
        }
    }
    block_sum_f64<1>(c, s_red, g.tid);
    return c[0];
}

__device__ __forceinline__ void pg_load6(const double *fb, int comp, size_t nf, int k, double (&v)[6])
{
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = fb[(comp + c) * nf + k];
}
__device__ __forceinline__ void pg_store6(double *fb, int comp, size_t nf, int k, const double (&v)[6])
{
#pragma unroll
    for (int c = 0; c < 6; ++c) fb[(comp + c) * nf + k] = v[c];
}

__global__ __launch_bounds__(256) void pg_solve_kernel(const PgArgs a)
{
    __shared__ double s_red[8];
    const int gi = blockIdx.x, tid = threadIdx.x;
    const RpeGraphJob &jb = a.job;
    const int gs = jb.graph_start[gi], F = jb.graph_start[gi + 1] - gs;
    const int es = jb.edge_start[gi];
    const int fs = jb.free_start[gi], nf = jb.free_start[gi + 1] - fs;
    const int us = jb.used_start[gi], nu = jb.used_start[gi + 1] - us;
    const int precode = jb.precode[gi];
    const int *gframe = jb.graph_frame + gs, *fpos = jb.free_pos + fs, *astart = jb.adj_start + fs;
    const int2 *adj = jb.adj;
    double *R = a.R + 9 * (size_t)gs, *T = a.T + 3 * (size_t)gs, *Rn = a.Rn + 9 * (size_t)gs, *Tn = a.Tn + 3 * (size_t)gs;
    double *fb = a.fb + PG_FB * (size_t)fs;
    const size_t nfs = (size_t)nf;
    const PgGraph g{tid, F, nf, nu, es, fpos, jb.used_edge + us, jb.edge_i, jb.edge_j, jb.edge_kind, jb.edge_R, jb.edge_t, jb.edge_w,
                    jb.huber, a.eb + PG_EB * (size_t)us, a.chi};
    // ---- the caller's poses as the state and as the trial state (a frame that is not free never moves)
    auto input_pose = [&](int p) {
        const double *Rp = jb.R_abs + 9 * (size_t)gframe[p], *Tp = jb.T_abs + 3 * (size_t)gframe[p];
#pragma unroll
        for (int e = 0; e < 9; ++e) { R[9 * (size_t)p + e] = Rp[e]; Rn[9 * (size_t)p + e] = Rp[e]; }
#pragma unroll
        for (int e = 0; e < 3; ++e) { T[3 * (size_t)p + e] = Tp[e]; Tn[3 * (size_t)p + e] = Tp[e]; }
    };
    for (int p = tid; p < F; p += 256) input_pose(p);
    __syncthreads();
    auto chi_unchanged = [&]() {
        for (int u = tid; u < nu; u += 256) { const size_t e = (size_t)es + g.uedge[u]; a.chi[2 * e + 1] = a.chi[2 * e]; }
    };
    if (precode >= 0) {                                                      // workgroup-uniform: a code the host has found
        const double c0 = pg_edges<false>(g, R, T, 0, s_red);
        chi_unchanged();
        if (tid == 0) {
            a.info[gi * 4] = precode; a.info[gi * 4 + 1] = 0; a.info[gi * 4 + 2] = 0; a.info[gi * 4 + 3] = 0;
            a.cost[gi * 2] = c0; a.cost[gi * 2 + 1] = c0;
        }
        return;
    }
    const double cost0 = pg_edges<true>(g, R, T, 0, s_red);
    double cost = cost0, rz = 0.;
    const double tol2 = jb.cg_tol * jb.cg_tol;
    int iters = 0, acc = 0, npcg = 0;
    bool need_lin = false;
    // the sum of one term per free frame: lane partials in strided order, butterfly, wave totals
    auto frame_sum = [&](auto term) {
        double v[1] = {0.};
        for (int k = tid; k < nf; k += 256) v[0] = v[0] + term(k);
        block_sum_f64<1>(v, s_red, tid);
        return v[0];
    };
    // ---- the step at damping lambda into the frame blocks' x; false when there is none
    auto step = [&](double lambda) {
        if (need_lin) { pg_edges<true>(g, R, T, -1, s_red); need_lin = false; }
        double v[2] = {0., 0.};                                              // blocks that are not positive definite; r.z
        for (int k = tid; k < nf; k += 256) {
            double H[36], gr[6], L[21], r[6], z[6] = {0., 0., 0., 0., 0., 0.}, x[6] = {0., 0., 0., 0., 0., 0.};
#pragma unroll
            for (int c = 0; c < 36; ++c) H[c] = 0.;
#pragma unroll
            for (int c = 0; c < 6; ++c) gr[c] = 0.;
            for (int ad = astart[k]; ad < astart[k + 1]; ++ad) {
                const int u = adj[ad].x >> 1, side = adj[ad].x & 1;
                const double *b = g.eb + u;
#pragma unroll
                for (int c = 0; c < 36; ++c) H[c] = H[c] + b[((side ? PG_EB_JJ : 0) + c) * (size_t)nu];
#pragma unroll
                for (int c = 0; c < 6; ++c) gr[c] = gr[c] + b[((side ? PG_EB_GJ : PG_EB_GI) + c) * (size_t)nu];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) { H[c * 7] = H[c * 7] + lambda * H[c * 7]; r[c] = -gr[c]; }
            gm_lower6(H, L);
            const bool ok = bm_chol<6>(L);
            if (ok) bm_chol_solve<6>(L, r, z); else v[0] = v[0] + 1.;
#pragma unroll
            for (int c = 0; c < 36; ++c) fb[c * nfs + k] = H[c];
#pragma unroll
            for (int c = 0; c < 21; ++c) fb[(PG_FB_L + c) * nfs + k] = ok ? L[c] : 0.;
            pg_store6(fb, PG_FB_R, nfs, k, r); pg_store6(fb, PG_FB_Z, nfs, k, z); pg_store6(fb, PG_FB_P, nfs, k, z);
            pg_store6(fb, PG_FB_X, nfs, k, x);
            v[1] = v[1] + gm_dot6(r, z);
        }
        block_sum_f64<2>(v, s_red, tid);
        if (v[0] != 0.) return false;
        rz = v[1];
        const double rz0 = rz;
        bool any = false;
        for (int it = 0; it < jb.cg_iters; ++it) {
            __syncthreads();                                                 // every p is written
            const double pHp = frame_sum([&](int k) {
                double p[6], hp[6];
                pg_load6(fb, PG_FB_P, nfs, k, p);
                double H[36];
#pragma unroll
                for (int c = 0; c < 36; ++c) H[c] = fb[c * nfs + k];
#pragma unroll
                for (int c = 0; c < 6; ++c) hp[c] = gm_row6(H, c, p);
                for (int ad = astart[k]; ad < astart[k + 1]; ++ad) {
                    const int o = adj[ad].y;
                    if (o < 0) continue;
                    const int u = adj[ad].x >> 1, side = adj[ad].x & 1;
                    double po[6], A[36];
                    pg_load6(fb, PG_FB_P, nfs, o, po);
#pragma unroll
                    for (int c = 0; c < 36; ++c) A[c] = g.eb[(PG_EB_IJ + c) * (size_t)nu + u];
#pragma unroll
                    for (int c = 0; c < 6; ++c) hp[c] = hp[c] + (side ? gm_col6(A, c, po) : gm_row6(A, c, po));
                }
                pg_store6(fb, PG_FB_HP, nfs, k, hp);
                return gm_dot6(p, hp);
            });
            if (!(pHp > 0.)) break;
            const double alpha = rz / pHp;
            const double rzn = frame_sum([&](int k) {
                double p[6], hp[6], x[6], r[6], z[6], L[21];
                pg_load6(fb, PG_FB_P, nfs, k, p); pg_load6(fb, PG_FB_HP, nfs, k, hp);
                pg_load6(fb, PG_FB_X, nfs, k, x); pg_load6(fb, PG_FB_R, nfs, k, r);
#pragma unroll
                for (int c = 0; c < 21; ++c) L[c] = fb[(PG_FB_L + c) * nfs + k];
#pragma unroll
                for (int c = 0; c < 6; ++c) { x[c] = x[c] + alpha * p[c]; r[c] = r[c] - alpha * hp[c]; }
                bm_chol_solve<6>(L, r, z);
                pg_store6(fb, PG_FB_X, nfs, k, x); pg_store6(fb, PG_FB_R, nfs, k, r); pg_store6(fb, PG_FB_Z, nfs, k, z);
                return gm_dot6(r, z);
            });
            any = true; ++npcg;
            if (rzn <= tol2 * rz0) break;
            const double beta = rzn / rz;
            for (int k = tid; k < nf; k += 256) {                            // a lane's own frames: no barrier in front
                double p[6], z[6];
                pg_load6(fb, PG_FB_P, nfs, k, p); pg_load6(fb, PG_FB_Z, nfs, k, z);
#pragma unroll
                for (int c = 0; c < 6; ++c) p[c] = z[c] + beta * p[c];
                pg_store6(fb, PG_FB_P, nfs, k, p);
            }
            rz = rzn;
        }
        return any;
    };
    // ---- the trial state of step x, and its cost
    auto trial = [&](double) {
        for (int k = tid; k < nf; k += 256) {
            double x[6];
            pg_load6(fb, PG_FB_X, nfs, k, x);
            const size_t p = (size_t)fpos[k];
            const double w[3] = {x[0], x[1], x[2]};
            gm_cayley(w, R + 9 * p, Rn + 9 * p);
#pragma unroll
            for (int e = 0; e < 3; ++e) Tn[3 * p + e] = T[3 * p + e] + x[3 + e];
        }
        __syncthreads();
        return pg_edges<false>(g, Rn, Tn, -1, s_red);
    };
    auto step_norm = [&]() {
        return sqrt(frame_sum([&](int k) { double x[6]; pg_load6(fb, PG_FB_X, nfs, k, x); return gm_dot6(x, x); }));
    };
    auto accept = [&]() {
        __syncthreads();                                                     // every reader of the old state is done
        for (int k = tid; k < nf; k += 256) {
            const size_t p = (size_t)fpos[k];
#pragma unroll
            for (int e = 0; e < 9; ++e) R[9 * p + e] = Rn[9 * p + e];
#pragma unroll
            for (int e = 0; e < 3; ++e) T[3 * p + e] = Tn[3 * p + e];
        }
        __syncthreads();
        need_lin = true;
    };
    if (hg_finite(cost0)) lm_loop(cost, jb.max_iters, step, trial, step_norm, accept, iters, acc);
    // ---- the optimised state is returned only if a step was accepted and it is finite
    const double bad = acc > 0 ? frame_sum([&](int k) {
        const size_t p = (size_t)fpos[k];
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 9; ++e) ok = ok && hg_finite(R[9 * p + e]);
#pragma unroll
        for (int e = 0; e < 3; ++e) ok = ok && hg_finite(T[3 * p + e]);
        return ok ? 0. : 1.;
    }) : 0.;
    const bool take = acc > 0 && bad == 0.;
    if (take) {
        pg_edges<false>(g, R, T, 1, s_red);
    } else {
        __syncthreads();
        for (int k = tid; k < nf; k += 256) input_pose(fpos[k]);
        chi_unchanged();
    }
    if (tid == 0) {
        a.info[gi * 4] = take ? RPE_GRAPH_OK : RPE_GRAPH_REJECTED; a.info[gi * 4 + 1] = iters; a.info[gi * 4 + 2] = acc; a.info[gi * 4 + 3] = npcg;
        a.cost[gi * 2] = cost0; a.cost[gi * 2 + 1] = take ? cost : cost0;
    }
}

// The launch of one job.  The buffers are the caller's business (rpe_optimise_graphs, rpe_features.hip)
void rpe_launch_graphs(rpe_handle *h, const RpeGraphJob &job)
{
    PgArgs a{};
    a.job = job;
    a.R = h->pg.Rout; a.T = h->pg.Tout; a.Rn = h->pg.Rn; a.Tn = h->pg.Tn;
    a.eb = h->pg.eb; a.fb = h->pg.fb; a.chi = h->pg.chi; a.cost = h->pg.cost; a.info = h->pg.info;
    hipLaunchKernelGGL(pg_solve_kernel, dim3(job.n_graphs), dim3(256), 0, h->stream, a);
}
