// Stand-alone run of relative_pose_estimation_amd/csrc/graph_plan.h (the argument check of rpe_optimise_graphs and the plan
// pg_solve_kernel trusts), built by tests/test_graph_plan_cpu.py with the address and undefined-behaviour sanitizers.  Every
// array is a heap block of exactly the length the caller gives, so a read in front of the check that guards it, or past a
// table the plan indexes, is a sanitizer error.  The check and the builder run as the entry point runs them: the builder
// only behind a check that passed, and not for a call without graphs.
//
//   graph_plan_host          stdin: calls of doubles: n_frames n_graphs huber max_iters cg_iters cg_tol, then the length of
//                            each of the 12 arrays in RpeGraphArgs' order (-1: a null pointer), then the arrays' values
//                            stdout: per call "refused <code> <text or ->" or "accepted" followed by one line per table:
//                            its name and its entries
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../relative_pose_estimation_amd/csrc/graph_plan.h"

template <class T>
static std::unique_ptr<T[]> block(const double *&in, long n)
{
    if (n < 0) return nullptr;
    std::unique_ptr<T[]> b(new T[(size_t)n]);
    for (long k = 0; k < n; ++k) b[(size_t)k] = (T)in[k];
    in += n;
    return b;
}

template <class V>
static void line(const char *name, const V &v)
{
    std::printf("%s", name);
    for (auto x : v) std::printf(" %d", (int)x);
    std::printf("\n");
}

int main()
{
    std::vector<double> in;
    double buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + n);
    const double *p = in.data(), *end = p + in.size();
    while (p < end) {
        if (end - p < 18) return 2;
        const double *head = p;
        long len[12], total = 0;
        for (int k = 0; k < 12; ++k) { len[k] = (long)head[6 + k]; total += len[k] > 0 ? len[k] : 0; }
        p += 18;
        if (end - p < total) return 2;
        auto R = block<double>(p, len[0]), T = block<double>(p, len[1]);
        auto gs = block<int32_t>(p, len[2]), gf = block<int32_t>(p, len[3]);
        auto fx = block<uint8_t>(p, len[4]);
        auto es = block<int32_t>(p, len[5]), ei = block<int32_t>(p, len[6]), ej = block<int32_t>(p, len[7]);
        auto eR = block<double>(p, len[8]), et = block<double>(p, len[9]), ew = block<double>(p, len[10]);
        auto ek = block<int32_t>(p, len[11]);
        const RpeGraphArgs a = {(int)head[0], R.get(), T.get(), (int)head[1], gs.get(), gf.get(), fx.get(), es.get(), ei.get(), ej.get(),
                                eR.get(), et.get(), ew.get(), ek.get(), head[2], (int)head[3], (int)head[4], head[5]};
        RpeGraphPlan plan;
        const RpeGraphRefusal no = rpe_graph_check(a, plan);
        if (no.code) { std::printf("refused %d %s\n", no.code, no.text ? no.text : "-"); continue; }
        std::printf("accepted\n");
        if (a.n_graphs > 0) rpe_graph_build(a, plan);
        line("ei", plan.ei); line("ej", plan.ej); line("free_start", plan.free_start); line("used_start", plan.used_start);
        line("precode", plan.precode); line("free_pos", plan.free_pos); line("used_edge", plan.used_edge);
        line("adj_start", plan.adj_start); line("adj", plan.adj); line("counts", plan.counts); line("used", plan.used);
    }
    return 0;
}
