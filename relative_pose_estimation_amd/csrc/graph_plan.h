// graph_plan.h -- the host side of rpe_optimise_graphs (include/rpe_amd.h, "pose graphs") in front of the device: the caller's
// view of a call, its argument check, and the plan, the active set and the tables pg_solve_kernel (graph_kernels.hip) reads
// without a bounds check of its own.  Plain C++, nothing of HIP or the handle: pointers in, a refusal or vectors out, so
// tests/native/graph_plan_host.cpp runs it on the host against tests/pose_graph_model.py's active_set.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rpe_amd.h"

struct RpeGraphArgs {
    int n_frames;
    const double *R_abs, *T_abs;              // [n_frames][9], [n_frames][3]
    int n_graphs;
    const int32_t *graph_start, *graph_frame; // [n_graphs + 1], [graph_start[n_graphs]]
    const uint8_t *fixed;                     // per graph position, or null: position 0 only
    const int32_t *edge_start, *edge_i, *edge_j;   // [n_graphs + 1], [edge_start[n_graphs]] frame indices
    const double *edge_R, *edge_t, *edge_w;   // per edge [9], [3], [2] = w_rot, w_trans
    const int32_t *edge_kind;
    double huber;
    int max_iters, cg_iters;
    double cg_tol;
};

// code RPE_OK: accepted.  Otherwise RPE_ERR_INVALID or RPE_ERR_CAPACITY with the refusal's text; a null text is the refusal
// that names no argument (rpe_invalid's default)
struct RpeGraphRefusal {
    int code;
    const char *text;
};

// Graph g owns the frames free_start[g] .. free_start[g + 1] of free_pos and adj_start, and the used edges used_start[g] ..
// of used_edge; adj holds pairs (used-edge number within the graph << 1 | side, free index of the other end or -1), per
// free frame in ascending used-edge number
struct RpeGraphPlan {
    std::vector<int> ei, ej;                  // per edge: the graph positions of its ends
    std::vector<int> free_start, used_start;  // [n_graphs + 1]
    std::vector<int> precode;                 // per graph: the code that needs no arithmetic, or -1
    std::vector<int> free_pos;                // per free frame: its graph position
    std::vector<int> used_edge;               // per used edge: its number within the graph's edges
    std::vector<int> adj_start, adj;          // [free frames + 1], [2 * entries]
    std::vector<int> counts;                  // per graph: frames, free frames, used edges, unused edges
    std::vector<uint8_t> used;                // per edge
};

static inline bool rpe_graph_finite(const double *v, size_t n)
{
    bool fin = true;
    for (size_t i = 0; i < n; ++i) fin = fin && std::isfinite(v[i]);
    return fin;
}

// The check, in this order: the scalars; nothing more of a call without graphs; the pointers; the two CSR tables (every
// graph's sizes, before any frame or edge is read); the edge pointers; then graph by graph the frames and the edges.  It
// leaves the positions of every edge's ends in p.ei and p.ej.  The frame-to-position map serves one graph and is cleared
// for the next.
static inline RpeGraphRefusal rpe_graph_check(const RpeGraphArgs &a, RpeGraphPlan &p)
{
    const auto invalid = [](const char *text) { return RpeGraphRefusal{RPE_ERR_INVALID, text}; };
    if (a.n_frames < 1) return invalid("n_frames must be >= 1");
    if (a.n_graphs < 0) return invalid("n_graphs must be >= 0");
    if (!(std::isfinite(a.huber) && a.huber >= 0.)) return invalid("huber must be finite and >= 0");
    if (a.max_iters < 1 || a.max_iters > 100) return invalid("max_iters must be 1 ... 100");
    if (a.cg_iters < 1 || a.cg_iters > 1000) return invalid("cg_iters must be 1 ... 1000");
    if (!(a.cg_tol >= 0. && a.cg_tol < 1.)) return invalid("cg_tol must lie in [0, 1)");
    if (a.n_graphs == 0) return {RPE_OK, nullptr};
    if (!a.R_abs || !a.T_abs || !a.graph_start || !a.graph_frame || !a.edge_start) return invalid(nullptr);
    if (a.graph_start[0] != 0 || a.edge_start[0] != 0) return invalid("graph_start[0] and edge_start[0] must be 0");
    for (int g = 0; g < a.n_graphs; ++g) {
        const int F = a.graph_start[g + 1] - a.graph_start[g], E = a.edge_start[g + 1] - a.edge_start[g];
        if (F < 0 || E < 0) return invalid("graph_start and edge_start must not decrease");
        if (F < 2) return invalid("a graph must have at least 2 frames");
        if (F > RPE_GRAPH_MAX_FRAMES) return {RPE_ERR_CAPACITY, "a graph exceeds RPE_GRAPH_MAX_FRAMES"};
        if (E > RPE_GRAPH_MAX_EDGES) return {RPE_ERR_CAPACITY, "a graph exceeds RPE_GRAPH_MAX_EDGES"};
    }
    const size_t ne = (size_t)a.edge_start[a.n_graphs];
    if (ne > 0 && (!a.edge_i || !a.edge_j || !a.edge_R || !a.edge_t || !a.edge_w || !a.edge_kind)) return invalid(nullptr);
    std::vector<int> pos_of((size_t)a.n_frames, -1);
    p.ei.assign(ne, 0); p.ej.assign(ne, 0);
    for (int g = 0; g < a.n_graphs; ++g) {
        const int gs = a.graph_start[g], F = a.graph_start[g + 1] - gs, es = a.edge_start[g], E = a.edge_start[g + 1] - es;
        const int32_t *f = a.graph_frame + gs;
        const char *bad = nullptr;
        for (int q = 0; q < F && !bad; ++q) {
            if (f[q] < 0 || f[q] >= a.n_frames) bad = "a graph frame outside 0 ... n_frames - 1";
            else if (pos_of[f[q]] >= 0) bad = "a frame repeated inside a graph";
            else if (!rpe_graph_finite(a.R_abs + (size_t)f[q] * 9, 9) || !rpe_graph_finite(a.T_abs + (size_t)f[q] * 3, 3))
                bad = "a non-finite pose of a frame that a graph names";
            else pos_of[f[q]] = q;
        }
        for (int k = 0; k < E && !bad; ++k) {
            const size_t e = (size_t)es + k;
            const int i = a.edge_i[e], j = a.edge_j[e];
            const double *M = a.edge_R + 9 * e, *m = a.edge_t + 3 * e, *w = a.edge_w + 2 * e;
            if (i < 0 || i >= a.n_frames || j < 0 || j >= a.n_frames || pos_of[i] < 0 || pos_of[j] < 0) bad = "an edge end that is no frame of its graph";
            else if (i == j) bad = "an edge from a frame to itself";
            else if (!rpe_graph_finite(M, 9) || !rpe_graph_finite(m, 3) || !rpe_graph_finite(w, 2)) bad = "a non-finite measurement or weight";
            else if (!(w[0] > 0.) || !(w[1] >= 0.)) bad = "edge_w must hold w_rot > 0 and w_trans >= 0";
            else if (a.edge_kind[e] != RPE_EDGE_METRIC && a.edge_kind[e] != RPE_EDGE_DIRECTION) bad = "an unknown edge kind";
            else if (a.edge_kind[e] == RPE_EDGE_DIRECTION && m[0] == 0. && m[1] == 0. && m[2] == 0.) bad = "a direction edge with a zero direction";
            for (int r = 0; r < 3 && !bad; ++r)
                for (int c = 0; c < 3 && !bad; ++c) {
                    const double d = (M[r * 3] * M[c * 3] + M[r * 3 + 1] * M[c * 3 + 1]) + M[r * 3 + 2] * M[c * 3 + 2];
                    if (!(std::fabs(d - (r == c ? 1. : 0.)) <= 1e-6)) bad = "an edge_R that is not orthonormal to 1e-6";
                }
            if (!bad) { p.ei[e] = pos_of[i]; p.ej[e] = pos_of[j]; }
        }
        if (bad) return invalid(bad);
        for (int q = 0; q < F; ++q) pos_of[f[q]] = -1;                       // the map serves the next graph
    }
    return {RPE_OK, nullptr};
}

// The plan of a call that rpe_graph_check has accepted (p.ei, p.ej are its): per graph the flood fill from the fixed
// frames, the free index per frame, the used edges, the adjacency per free frame, the code that needs no arithmetic, counts
static inline void rpe_graph_build(const RpeGraphArgs &a, RpeGraphPlan &p)
{
    const size_t ng = (size_t)a.n_graphs, ne = (size_t)a.edge_start[a.n_graphs];
    p.free_start.assign(ng + 1, 0); p.used_start.assign(ng + 1, 0); p.precode.assign(ng, -1);
    p.free_pos.clear(); p.used_edge.clear(); p.adj_start.assign(1, 0); p.adj.clear(); p.counts.assign(4 * ng, 0);
    p.used.assign(ne, 0);
    std::vector<int> fidx, comp, stack;
    std::vector<std::vector<int>> nb;
    for (int g = 0; g < a.n_graphs; ++g) {
        const int gs = a.graph_start[g], F = a.graph_start[g + 1] - gs, es = a.edge_start[g], E = a.edge_start[g + 1] - es;
        // active: joined to a fixed frame by a path of edges
        nb.assign(F, {});
        for (int k = 0; k < E; ++k) { nb[p.ei[es + k]].push_back(p.ej[es + k]); nb[p.ej[es + k]].push_back(p.ei[es + k]); }
        comp.assign(F, 0);                                                  // 1: active
        stack.clear();
        auto is_fixed = [&](int q) { return q == 0 || (a.fixed && a.fixed[gs + q]); };
        for (int q = 0; q < F; ++q) if (is_fixed(q)) { comp[q] = 1; stack.push_back(q); }
        while (!stack.empty()) {
            const int q = stack.back(); stack.pop_back();
            for (int o : nb[q]) if (!comp[o]) { comp[o] = 1; stack.push_back(o); }
        }
        fidx.assign(F, -1);
        int nfree = 0;
        for (int q = 0; q < F; ++q) if (comp[q] && !is_fixed(q)) { fidx[q] = nfree++; p.free_pos.push_back(q); }
        // used edges, and per free frame its adjacency in ascending used-edge number
        std::vector<std::vector<int>> &inc = nb;                            // reused: per free frame (x, y) pairs
        inc.assign(nfree, {});
        std::vector<uint8_t> has_trans(nfree, 0);
        int nused = 0;
        for (int k = 0; k < E; ++k) {
            const size_t e = (size_t)es + k;
            const int pi = p.ei[e], pj = p.ej[e];
            if (!comp[pi] || !comp[pj] || (fidx[pi] < 0 && fidx[pj] < 0)) continue;
            p.used[e] = 1; p.used_edge.push_back(k);
            const bool trans = a.edge_w[2 * e + 1] > 0.;
            if (fidx[pi] >= 0) { inc[fidx[pi]].push_back(nused << 1); inc[fidx[pi]].push_back(fidx[pj]); if (trans) has_trans[fidx[pi]] = 1; }
            if (fidx[pj] >= 0) { inc[fidx[pj]].push_back(nused << 1 | 1); inc[fidx[pj]].push_back(fidx[pi]); if (trans) has_trans[fidx[pj]] = 1; }
            ++nused;
        }
        for (int k = 0; k < nfree; ++k) {
            p.adj.insert(p.adj.end(), inc[k].begin(), inc[k].end());
            p.adj_start.push_back((int)(p.adj.size() / 2));
        }
        p.free_start[g + 1] = p.free_start[g] + nfree; p.used_start[g + 1] = p.used_start[g] + nused;
        if (nused == 0) p.precode[g] = RPE_GRAPH_NO_EDGES;
        else for (int k = 0; k < nfree; ++k) if (!has_trans[k]) p.precode[g] = RPE_GRAPH_UNDERDETERMINED;
        p.counts[4 * g] = F; p.counts[4 * g + 1] = nfree; p.counts[4 * g + 2] = nused; p.counts[4 * g + 3] = E - nused;
    }
}
