// Host run of relative_pose_estimation_amd/csrc/bundle_math.h: the statements the bundle kernels run on a GPU lane, here on
// the CPU.  Stand-alone; tests/test_bundle_math_cpu.py builds it without floating-point contraction (the device build's
// setting), plain and with the host sanitizers, feeds it seeded cases and compares what it returns bit for bit.
//
//   bundle_math_host view     stdin: records of 18 doubles R[9] t[3] X[3] scale qx qy
//                             stdout: per record 28 doubles: bm_view<false>'s e[2] y2 u[2], then bm_view<true>'s e[2] y2 u[2],
//                             Jx[6] Jy[6] and bm_point_rows' JXx[3] JXy[3]
//   bundle_math_host block    stdin: records of 66 doubles: the number of rows, lambda, 16 rows of J[3] e (the first rows count)
//                             stdout: per record 19 doubles: V[6] and g_p[3] after bm_block_row over the rows in order,
//                             bm_damped_inverse's Vi[6] and verdict, bm_sym_row(Vi, 0 .. 2, g_p)
//   bundle_math_host lm       stdin: scripts of doubles: max_iters, cost, n, then n triples (a step exists, the trial's cost,
//                             the step's length), one per iteration
//                             stdout: per script one line: iters acc cost accepts, then the hooks' calls in order: L (the
//                             state is linearised: the arrangement of refine_lm, geom_device.h), S:lambda, T:lambda, N, A
//   bundle_math_host solve    stdin: records of 2 + N (N + 1) / 2 + N doubles: N (3, 5, 6 or 11), lambda, H's upper triangle
//                             (row-major), g
//                             stdout: per record 1 + N doubles: refine_solve<N>'s verdict and d (zeros when it refused)
// Doubles travel as raw bytes, in the lm lines as hex floats.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../relative_pose_estimation_amd/csrc/bundle_math.h"

static std::vector<double> read_all()
{
    std::vector<double> v;
    double buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(double), 4096, stdin)) > 0) v.insert(v.end(), buf, buf + n);
    return v;
}

template <int N>
static void solve_record(const double *rec)
{
    double out[1 + N], d[N];
    const bool ok = refine_solve<N>(rec + 2, rec + 2 + N * (N + 1) / 2, rec[1], d);
    out[0] = ok ? 1. : 0.;
    for (int i = 0; i < N; ++i) out[1 + i] = ok ? d[i] : 0.;
    fwrite(out, sizeof(double), 1 + N, stdout);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s view | block | lm | solve  (cases on stdin)\n", argv[0]); return 2; }
    const std::vector<double> in = read_all();
    if (!strcmp(argv[1], "view")) {
        const size_t REC = 18;
        if (in.size() % REC) return 2;
        for (size_t o = 0; o < in.size(); o += REC) {
            const double *R = in.data() + o, *t = R + 9, *X = t + 3;
            const double scale = in[o + 15], qx = in[o + 16], qy = in[o + 17];
            double out[28], Jx[6], Jy[6], JXx[3], JXy[3];
            bm_view<false>(R, t, scale, X, qx, qy, out[0], out[1], nullptr, nullptr, out + 2);
            bm_view<true>(R, t, scale, X, qx, qy, out[5], out[6], Jx, Jy, out + 7);
            bm_point_rows(Jx, Jy, R, JXx, JXy);
            memcpy(out + 10, Jx, sizeof Jx); memcpy(out + 16, Jy, sizeof Jy);
            memcpy(out + 22, JXx, sizeof JXx); memcpy(out + 25, JXy, sizeof JXy);
            fwrite(out, sizeof(double), 28, stdout);
        }
        return 0;
    }
    if (!strcmp(argv[1], "block")) {
        const size_t REC = 66;
        if (in.size() % REC) return 2;
        for (size_t o = 0; o < in.size(); o += REC) {
            const int rows = (int)in[o];
            const double lambda = in[o + 1];
            if (rows < 0 || rows > 16) return 2;
            double v[6] = {0., 0., 0., 0., 0., 0.}, gp[3] = {0., 0., 0.}, Vi[6], out[19];
            for (int r = 0; r < rows; ++r) {
                const double J[3] = {in[o + 2 + 4 * r], in[o + 3 + 4 * r], in[o + 4 + 4 * r]};
                bm_block_row(J, in[o + 5 + 4 * r], v, gp);
            }
            memcpy(out, v, sizeof v); memcpy(out + 6, gp, sizeof gp);
            out[15] = bm_damped_inverse(v, lambda, Vi) ? 1. : 0.;
            memcpy(out + 9, Vi, sizeof Vi);
            for (int i = 0; i < 3; ++i) out[16 + i] = bm_sym_row(Vi, i, gp);
            fwrite(out, sizeof(double), 19, stdout);
        }
        return 0;
    }
    if (!strcmp(argv[1], "solve")) {
        size_t o = 0;
        while (o < in.size()) {
            const int N = (int)in[o];
            if (N != 3 && N != 5 && N != 6 && N != 11) return 2;
            const size_t rec = 2 + (size_t)N * (N + 1) / 2 + N;
            if (o + rec > in.size()) return 2;
            // a block of the record's own length: a read past the triangle or g is a sanitizer error
            const std::vector<double> r(in.begin() + o, in.begin() + o + rec);
            if (N == 3) solve_record<3>(r.data());
            else if (N == 5) solve_record<5>(r.data());
            else if (N == 6) solve_record<6>(r.data());
            else solve_record<11>(r.data());
            o += rec;
        }
        return 0;
    }
    if (!strcmp(argv[1], "lm")) {
        size_t o = 0;
        while (o < in.size()) {
            if (o + 3 > in.size()) return 2;
            const int max_iters = (int)in[o];
            double cost = in[o + 1];
            const size_t n = (size_t)in[o + 2];
            const double *script = in.data() + o + 3;
            o += 3 + 3 * n;
            if (o > in.size()) return 2;
            int iters = 0, acc = 0, accepts = 0;
            long it = -1;                                  // the iteration the hooks are in
            bool need_lin = false, overrun = false;
            std::vector<char> log(1, '\0');
            auto note = [&](const char *what, double lambda) {
                char b[64];
                if (what[0] == 'S' || what[0] == 'T') snprintf(b, sizeof b, " %s:%a", what, lambda);
                else snprintf(b, sizeof b, " %s", what);
                log.pop_back();
                log.insert(log.end(), b, b + strlen(b) + 1);
            };
            // refine_lm's arrangement: linearise in the step hook after an accepted step, the flag set in accept
            lm_loop(cost, max_iters,
                    [&](double lambda) {
                        ++it;
                        if ((size_t)it >= n) { overrun = true; return false; }
                        if (need_lin) { note("L", 0.); need_lin = false; }
                        note("S", lambda);
                        return script[3 * it] != 0.;
                    },
                    [&](double lambda) { note("T", lambda); return script[3 * it + 1]; },
                    [&]() { note("N", 0.); return script[3 * it + 2]; },
                    [&]() { note("A", 0.); ++accepts; need_lin = true; },
                    iters, acc);
            if (overrun) return 3;
            printf("%d %d %a %d%s\n", iters, acc, cost, accepts, log.data());
        }
        return 0;
    }
    return 2;
}
