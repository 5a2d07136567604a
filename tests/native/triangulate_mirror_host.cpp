// Host check of relative_pose_estimation_amd/csrc/pose_triangulate.h: triangulate_pm (one SVD, the verdicts of t and -t)
// against triangulate_one called for t and for -t.  Stand-alone; tests/test_triangulate_mirror_cpu.py builds it with and
// without floating-point contraction and reads the one line it prints.
//
//   triangulate_mirror_host random N SEED      N seeded random (R, unit t, x1, y1, x2, y2), a third near-identity rotations
//   triangulate_mirror_host crafted X1 Y1 Y2   R = I, t = (-1, -1, 0), x2 = 0: the case that raises the tie (for X1 = 0)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../relative_pose_estimation_amd/csrc/pose_triangulate.h"

static uint64_t g_state;
static uint64_t next_u64()                       // splitmix64
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * ((next_u64() >> 11) * (1. / 9007199254740992.)); }

static void unit3(double *v)
{
    double n;
    do { for (int i = 0; i < 3; ++i) v[i] = uni(-1., 1.); n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); } while (n < 1e-3 || n > 1.);
    for (int i = 0; i < 3; ++i) v[i] /= n;
}

static void rodrigues(const double *axis, double ang, double *R)
{
    const double c = cos(ang), s = sin(ang), x = axis[0], y = axis[1], z = axis[2];
    R[0] = c + x * x * (1 - c);     R[1] = x * y * (1 - c) - z * s; R[2] = x * z * (1 - c) + y * s;
    R[3] = y * x * (1 - c) + z * s; R[4] = c + y * y * (1 - c);     R[5] = y * z * (1 - c) - x * s;
    R[6] = z * x * (1 - c) - y * s; R[7] = z * y * (1 - c) + x * s; R[8] = c + z * z * (1 - c);
}

struct Outcome { int tie, verdicts_equal, plus_equal, point_mirrors, raw_mirror_verdict_equal; };

// one case through the three routes
static Outcome check(const double *R, const double *t, double x1, double y1, double x2, double y2)
{
    Outcome o;
    const double tn[3] = {-t[0], -t[1], -t[2]};
    int gp, gm, raw;
    double Pp[3], P0[3], Pd[3];
    o.tie = triangulate_pm(R, t, x1, y1, x2, y2, gp, gm, Pp, &raw) ? 1 : 0;   // raw: the mirror without its fallback
    const int g0 = triangulate_one(R, t, x1, y1, x2, y2, P0);
    const int gd = triangulate_one(R, tn, x1, y1, x2, y2, Pd);
    o.verdicts_equal = gm == gd;
    o.plus_equal = gp == g0 && memcmp(Pp, P0, sizeof Pp) == 0;
    const double neg[3] = {-Pp[0], -Pp[1], -Pp[2]};
    o.point_mirrors = memcmp(neg, Pd, sizeof neg) == 0;
    o.raw_mirror_verdict_equal = raw == gd;
    return o;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "crafted")) {
        const double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.}, t[3] = {-1., -1., 0.};
        const Outcome o = check(R, t, atof(argv[2]), atof(argv[3]), 0., atof(argv[4]));
        printf("tie=%d verdicts_equal=%d plus_equal=%d point_mirrors=%d raw_mirror_verdict_equal=%d\n", o.tie, o.verdicts_equal,
               o.plus_equal, o.point_mirrors, o.raw_mirror_verdict_equal);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "random")) {
        const long n = atol(argv[2]);
        g_state = strtoull(argv[3], 0, 10);
        long ties = 0, bad_verdict = 0, bad_plus = 0, bad_point = 0, minus_good = 0, plus_good = 0;
        for (long i = 0; i < n; ++i) {
            double axis[3], R[9], t[3];
            unit3(axis);
            const double ang = (i % 3 == 0) ? uni(-1., 1.) * pow(10., uni(-7., -1.)) : uni(-3.1, 3.1);
            rodrigues(axis, ang, R);
            unit3(t);
            double x1, y1, x2, y2;
            if (i & 1) {                         // a scene point, in front of or behind camera 1, seen with a little noise
                double X[3] = {uni(-4., 4.), uni(-3., 3.), uni(0.5, 20.) * (next_u64() & 1 ? 1. : -1.)};
                const double s = (next_u64() & 1) ? 1. : -1.;
                double Y[3];
                for (int r = 0; r < 3; ++r) Y[r] = (R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2]) + s * t[r];
                if (fabs(Y[2]) < 1e-2) Y[2] = 1e-2;
                x1 = X[0] / X[2] + uni(-1e-3, 1e-3); y1 = X[1] / X[2] + uni(-1e-3, 1e-3);
                x2 = Y[0] / Y[2] + uni(-1e-3, 1e-3); y2 = Y[1] / Y[2] + uni(-1e-3, 1e-3);
            } else {
                x1 = uni(-0.7, 0.7); y1 = uni(-0.5, 0.5); x2 = uni(-0.7, 0.7); y2 = uni(-0.5, 0.5);
            }
            const Outcome o = check(R, t, x1, y1, x2, y2);
            ties += o.tie;
            bad_verdict += !o.verdicts_equal;
            bad_plus += !o.plus_equal;
            if (!o.tie) bad_point += !o.point_mirrors;
            int gp, gm; double P[3];
            triangulate_pm(R, t, x1, y1, x2, y2, gp, gm, P);
            plus_good += gp; minus_good += gm;
        }
        printf("cases=%ld ties=%ld bad_verdict=%ld bad_plus=%ld bad_point=%ld plus_good=%ld minus_good=%ld\n", n, ties, bad_verdict,
               bad_plus, bad_point, plus_good, minus_good);
        return 0;
    }
    fprintf(stderr, "usage: %s random N SEED | crafted X1 Y1 Y2\n", argv[0]);
    return 2;
}
