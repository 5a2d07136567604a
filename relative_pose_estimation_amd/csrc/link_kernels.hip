// link_kernels.hip -- the calls over links on gfx950: two pairs of the last run that share a frame (NOT in the reference;
// include/rpe_amd.h states the rules).
//   scale links   : the baseline of pair b in units of pair a's, from the shared frame's keypoints both triangulated
//   link poses    : P3P RANSAC of pair b's other frame against the points pair a triangulated, polished by refine_lm<6>
//   link bundles  : bundle adjustment of the link's three views (gather + bundle, refine_lm<11> on the reduced system)
// One 256-thread workgroup per link, f64 throughout; what the pair kernels of geom_kernels.hip use as well is in
// geom_device.h.  The reprojection view (bm_view), the rows by the point, the point block with its adjugate inverse and the
// rule under refine_lm (lm_loop) are bundle_math.h's, shared with the track points and the window bundles.  All f64 arithmetic keeps the oracle's operation order (compiled with -ffp-contract=off).
#include "rpe_internal.h"
#include "geom_device.h"
#include <algorithm>
// ------------------------------------------------------------ scale links
// rpe_scale_links (NOT in the reference; include/rpe_amd.h states the rules): the baseline of pair b in units of the
// baseline of pair a, from the keypoints of the frame the two pairs share that both triangulated.  One 256-thread
// workgroup per link, f64 throughout, everything between the per-match buffers and the three results stays in LDS.
//   table   (link_join) one word per keypoint of the shared frame: high half = lowest usable match index of pair a, low
//           half = of pair b, 0xFFFF = none (max_matches <= 8064 < 0xFFFF).  Pass 1: a's usable matches atomicMin (index << 16 |
//           0xFFFF): every low half is still 0xFFFF, so the minimum orders the high halves.  Pass 2: b's usable matches
//           whose key has an a entry atomicMin (that high half << 16 | index): equal high halves, the minimum orders the
//           low ones.
//   ratios  pass 3: b's matches that won their key compute d_a / d_b and append it to an LDS array (integer atomicAdd on
//           the fill count: the order inside the array varies run to run, the set does not)
//   ranks   bitonic sort of the array, padded with +inf to a power of two; the three results are elements of the sorted
//           array, so they are bit-deterministic whatever order pass 3 left (ties are equal values)
// Dynamic LDS (all of the kernel's LDS, base 16-byte aligned; ScaleLinksLds states it for kernel and launcher): [sort_cap
// f64 ratios][kcap u32 table][fill count], sort_cap = next power of two >= max_matches.  Defaults (500 matches, 4064
// keypoints): 4 + 15.9 KB; uncapped SIFT (8064 matches, 16384 keypoints): 64 + 64 KB, the most (rpe_link_lds_ceilings).
// The link, the two pairs' status, match counts, R and t come from blockIdx-indexed reads: uniform, scalar loads.
#define LINK_NONE 0xFFFFu
static_assert(RPE_MAX_MATCHES_LIMIT < LINK_NONE, "a match index fits half a table word beside the empty value");

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

// the nine R and three t of one pose, from / to wherever the two parts lie
__device__ __forceinline__ void pose_load(const double *__restrict__ Rp, const double *__restrict__ tp, double (&R)[9], double (&t)[3])
{
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = Rp[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = tp[e];
}
__device__ __forceinline__ void pose_store(double *__restrict__ Rp, double *__restrict__ tp, const double (&R)[9], const double (&t)[3])
{
#pragma unroll
    for (int e = 0; e < 9; ++e) Rp[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) tp[e] = t[e];
}

// R' and -R't: the inverse of x -> R x + t
__device__ __forceinline__ void rigid_invert(const double (&R)[9], const double (&t)[3], double (&Ri)[9], double (&ti)[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Ri[r * 3 + c] = R[c * 3 + r];
        ti[r] = -((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]);
    }
}

// (R, t) itself, or its inverse when `inverted`: between a pair's own convention (image 1 -> image 2) and the solved form
// (shared frame -> the other frame), which differ when the shared frame is the pair's image 2
__device__ __forceinline__ void rigid_convention(bool inverted, const double (&R)[9], const double (&t)[3], double (&Ro)[9], double (&to)[3])
{
    double Ri[9], ti[3];
    rigid_invert(R, t, Ri, ti);
#pragma unroll
    for (int e = 0; e < 9; ++e) Ro[e] = inverted ? Ri[e] : R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) to[e] = inverted ? ti[e] : t[e];
}

// One link as its workgroup sees it, built once from the source and the workgroup's index (uniform: scalar loads and
// SGPRs): a2 / b2 the shared frame is image 2 of pair a / of pair b, na / nb the two pairs' match counts, oa / ob the
// offsets of their matches in the per-match arrays, key_a / key_b their matches' keypoint indices in the shared frame.
struct LinkView {
    RpeLink lk;
    bool a2, b2;
    int na, nb;
    long long oa, ob;
    const int *key_a, *key_b;
    __device__ __forceinline__ LinkView(const RpeLinkSrc &s, int link) : lk(s.links[link])
    {
        a2 = (lk.side & 1) != 0; b2 = (lk.side & 2) != 0;
        na = min(s.m_n[lk.a], s.max_matches); nb = min(s.m_n[lk.b], s.max_matches);
        oa = (long long)lk.a * s.max_matches; ob = (long long)lk.b * s.max_matches;
        key_a = (a2 ? s.m_t : s.m_q) + oa; key_b = (b2 ? s.m_t : s.m_q) + ob;
    }
};

// match i at offset o of the per-match arrays is usable: both structure masks hold it
__device__ __forceinline__ bool link_usable(const RpeLinkSrc &s, long long o, int i) { return s.ransac_mask[o + i] && s.pose_mask[o + i]; }
// the table's word of keypoint `key`; a key outside the table has the empty word
__device__ __forceinline__ unsigned link_entry(const unsigned *s_tab, int kcap, int key)
{
    return (unsigned)key < (unsigned)kcap ? s_tab[key] : 0xFFFFFFFFu;
}
// e = the word of its key: match i of pair b won the key (pair a has a usable match there and i is b's lowest) ...
__device__ __forceinline__ bool link_b_won(unsigned e, int i) { return (e >> 16) != LINK_NONE && (e & 0xFFFFu) == (unsigned)i; }
// ... match i of pair a won it (i is a's lowest usable match there)
__device__ __forceinline__ bool link_a_won(unsigned e, int i) { return (e >> 16) == (unsigned)i; }

// The table of the header in s_tab[kcap], for pairs a and b of link lv.  A match of a is usable when both masks hold it;
// FILTER_B asks the same of b's matches, else every match of b takes part.  All 256 threads call it (three barriers, the
// last behind pass 2: the table is final on return).
template <bool FILTER_B>
__device__ __forceinline__ void link_join(unsigned *s_tab, const RpeLinkSrc &s, const LinkView &lv)
{
    const int tid = threadIdx.x;
    for (int k = tid; k < s.kcap; k += 256) s_tab[k] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = tid; i < lv.na; i += 256) {
        if (!link_usable(s, lv.oa, i)) continue;
        const int key = lv.key_a[i];
        if ((unsigned)key < (unsigned)s.kcap) atomicMin(&s_tab[key], ((unsigned)i << 16) | LINK_NONE);
    }
    __syncthreads();
    for (int i = tid; i < lv.nb; i += 256) {
        if (FILTER_B && !link_usable(s, lv.ob, i)) continue;
        const int key = lv.key_b[i];
        const unsigned e = link_entry(s_tab, s.kcap, key);  // the high half is final since the barrier
        if ((e >> 16) != LINK_NONE) atomicMin(&s_tab[key], (e & 0xFFFF0000u) | (unsigned)i);
    }
    __syncthreads();
}

// The kernel's dynamic LDS, for the kernel's carve-up and the launcher's size: the ratios at 0, sort_cap = the power of two
// >= max(max_matches, 8) of them; byte offsets of the table and of the fill count; the size
struct ScaleLinksLds {
    size_t tab = 0, fill = 0, total = 0;
    __host__ __device__ constexpr ScaleLinksLds(int max_matches, int kcap)
    {
        int sort_cap = 8;
        while (sort_cap < max_matches) sort_cap <<= 1;
        tab = sizeof(double) * (size_t)sort_cap;
        fill = tab + sizeof(unsigned) * (size_t)kcap;
        total = fill + 16;
    }
};
constexpr size_t SCALE_LINKS_LDS_MAX = ScaleLinksLds(RPE_MAX_MATCHES_LIMIT, RPE_MAX_KCAP).total;   // the largest max_matches over uncapped SIFT's keypoints
static_assert(SCALE_LINKS_LDS_MAX <= RPE_CU_LDS_BYTES, "the largest handle's ratios and table fit a CU's LDS");

__global__ __launch_bounds__(256) void scale_links_kernel(const RpeLinkSrc src, int min_shared, double *__restrict__ stats,
                                                           int *__restrict__ n_shared, int *__restrict__ code)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_link[];
    const ScaleLinksLds lay(src.max_matches, src.kcap);
    double *s_ratio = (double *)s_link;
    unsigned *s_tab = (unsigned *)(s_link + lay.tab);
    int *s_fill = (int *)(s_link + lay.fill);
    const int link = blockIdx.x, tid = threadIdx.x;
    const LinkView lv(src, link);
    if (src.status[lv.lk.a] != RPE_PAIR_OK || src.status[lv.lk.b] != RPE_PAIR_OK) {
        if (tid < 3) stats[link * 3 + tid] = 0.;
        if (tid == 0) { n_shared[link] = 0; code[link] = RPE_LINK_PAIR_FAILED; }
        return;
    }
    if (tid == 0) *s_fill = 0;
    link_join<true>(s_tab, src, lv);
    double Ra[9], ta[3], Rb[9], tb[3];
    pose_load(src.R + lv.lk.a * 9, src.t + lv.lk.a * 3, Ra, ta);
    pose_load(src.R + lv.lk.b * 9, src.t + lv.lk.b * 3, Rb, tb);
    for (int i = tid; i < lv.nb; i += 256) {
        if (!link_usable(src, lv.ob, i)) continue;
        const unsigned e = link_entry(s_tab, src.kcap, lv.key_b[i]);
        if (!link_b_won(e, i)) continue;
        const double da = link_distance(src.points + (lv.oa + (e >> 16)) * 3, Ra, ta, lv.a2);
        const double db = link_distance(src.points + (lv.ob + i) * 3, Rb, tb, lv.b2);
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

// the last run's d_status / d_m_n / d_R / d_t, its match indices and the structure buffers -> link.stats / n / code of
// the L links in link.links
void rpe_launch_scale_links(rpe_handle *h, int L, int min_shared)
{
    const RpeLinkSrc src = rpe_link_src(h);
    const size_t lds = ScaleLinksLds(src.max_matches, src.kcap).total;
    hipLaunchKernelGGL(scale_links_kernel, dim3(L), dim3(256), lds, h->stream, src, min_shared, h->link.stats, h->link.n, h->link.code);
}

// ------------------------------------------------------------ link poses
// rpe_link_poses (NOT in the reference; include/rpe_amd.h states the rule): the pose of pair b's other frame C against the
// points pair a triangulated, by P3P RANSAC over the keypoints of the shared frame S, on pair a's scale.  One 256-thread
// workgroup per link, f64 throughout, no contraction.
//   join     link_join's packed table (high half: lowest usable match of a, low half: lowest match of b; here every match
//            of b takes part).  The winners of b are then compacted in match order by ordered_slot (ballot / popcount):
//            correspondence c = the c-th winner, so no atomic decides an order.
//   list     per correspondence X (3 f64, link_point: in S's frame), q (2 f64) and b's match index (u16).  X and q live in
//            LDS up to LP_LDS_MATCHES matches (40 B each: 20 KB at the default 500) and in lp.corr above it; both forms
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
// Dynamic LDS (all of the kernel's LDS, base 16-byte aligned; LinkPoseLds states it for kernel and launcher):
//   [A] max(kcap u32 table, LP_ROUND * 4 poses of 12 f64 = 96 KB): the table is dead once the list is built, the poses
//       once the election is over (the winner's inlier flags then live there)
//   [s_red 4 * 28 f64][X, q: 40 B * max_matches when in LDS][dense list 1024 u16][match indices max_matches u16][32 ints]
// 120 KB at the defaults (one workgroup per CU), 141 KB at the cut, 115 KB for uncapped SIFT (8064 matches in lp.corr).
#define LP_ROUND 256
#define LP_POSE_DOUBLES 12
#define LP_MODEL_BYTES (sizeof(double) * LP_ROUND * 4 * LP_POSE_DOUBLES)   // a round's candidates: up to four poses per sample
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

// The kernel's dynamic LDS (the list of the header), for the kernel's carve-up and the launcher's size: region A at 0, the
// byte offsets of what follows it, the size.  corr_in_lds: X and q are staged here, else they are in lp.corr
struct LinkPoseLds {
    bool corr_in_lds = false;
    size_t red = 0, corr = 0, list = 0, idx = 0, ints = 0, total = 0;
    __host__ __device__ constexpr LinkPoseLds(int max_matches, int kcap)
    {
        const size_t bytesT = sizeof(unsigned) * (size_t)kcap;
        corr_in_lds = max_matches <= LP_LDS_MATCHES;
        red = ((bytesT > LP_MODEL_BYTES ? bytesT : LP_MODEL_BYTES) + 15) & ~(size_t)15;                   // [4 * LP_NSUM] f64
        corr = red + sizeof(double) * 4 * LP_NSUM;                                                    // [5 * max_matches] f64 when corr_in_lds
        list = corr + (corr_in_lds ? sizeof(double) * RPE_LINK_POSE_CORR_DOUBLES * (size_t)max_matches : 0);                   // [LP_ROUND * 4] u16
        idx = list + sizeof(unsigned short) * LP_ROUND * 4;                                           // [max_matches rounded up to 8] u16
        ints = idx + sizeof(unsigned short) * (size_t)((max_matches + 7) & ~7);                       // [32] ints
        total = ints + sizeof(int) * 32;
    }
};
// the most: the cut, or the largest max_matches (the size grows with max_matches on either side of the cut, and no table
// adds to it)
constexpr size_t LINK_POSE_LDS_MAX = LinkPoseLds(LP_LDS_MATCHES, 0).total > LinkPoseLds(RPE_MAX_MATCHES_LIMIT, 0).total
                                         ? LinkPoseLds(LP_LDS_MATCHES, 0).total : LinkPoseLds(RPE_MAX_MATCHES_LIMIT, 0).total;
static_assert(LINK_POSE_LDS_MAX <= RPE_CU_LDS_BYTES, "the layout at the cut and at the largest max_matches fits a CU's LDS");
static_assert(sizeof(unsigned) * RPE_MAX_KCAP <= LP_MODEL_BYTES, "no table is larger than the candidates it shares region A with");

template <bool CAM>
__global__ __launch_bounds__(256) void link_pose_kernel(const RpeLinkSrc src, const unsigned short *__restrict__ subsets,
                                                         const double *__restrict__ K, const RpeCamSrc cam, double threshold_px,
                                                         int iters, int max_iters, int min_shared, int refine_iters,
                                                         double *__restrict__ corr, double *__restrict__ Rout,
                                                         double *__restrict__ tout, uint8_t *__restrict__ mask,
                                                         int *__restrict__ counts, int *__restrict__ info, double *__restrict__ rms)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lp[];
    const int max_matches = src.max_matches;
    const LinkPoseLds lay(max_matches, src.kcap);
    unsigned *s_tab = (unsigned *)s_lp;                                      // [kcap], until the list is built
    double *s_model = (double *)s_lp;                                        // [LP_ROUND * 4][12], during the rounds
    uint8_t *s_in = (uint8_t *)s_lp;                                         // [n] the winner's inlier flags, after the election
    double *s_red = (double *)(s_lp + lay.red), *s_corr = (double *)(s_lp + lay.corr);
    unsigned short *s_list = (unsigned short *)(s_lp + lay.list), *s_idx = (unsigned short *)(s_lp + lay.idx);
    int *s_int = (int *)(s_lp + lay.ints);                                   // [4] wave counts, [8] bests, [4] counts
    int *s_wc = s_int, *s_best = s_int + 4, *s_cnt = s_int + 12;
    const int link = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const LinkView lv(src, link);
    const long long om = (long long)link * max_matches;
    int code = src.status[lv.lk.a] == RPE_PAIR_OK ? RPE_LINKPOSE_OK : RPE_LINKPOSE_PAIR_FAILED;
    int n = 0;
    double *cX = lay.corr_in_lds ? s_corr : corr + (long long)link * RPE_LINK_POSE_CORR_DOUBLES * max_matches, *cq = cX + 3 * (size_t)max_matches;
    if (code == RPE_LINKPOSE_OK) {                                           // workgroup-uniform
        // ---- join and ordered list
        const double2 *obs = (lv.b2 ? src.n1 : src.n2) + lv.ob;                // b's point on C, its frame that is not shared
        link_join<false>(s_tab, src, lv);
        double Ra[9], ta[3];
        pose_load(src.R + lv.lk.a * 9, src.t + lv.lk.a * 3, Ra, ta);
        for (int i0 = 0; i0 < lv.nb; i0 += 256) {
            const int i = i0 + tid;
            const unsigned e = i < lv.nb ? link_entry(s_tab, src.kcap, lv.key_b[i]) : 0xFFFFFFFFu;
            const bool f = link_b_won(e, i);
            const int pos = ordered_slot(f, s_wc, n);
            if (f) {
                double x, y, z;
                link_point(src.points + (lv.oa + (e >> 16)) * 3, Ra, ta, lv.a2, x, y, z);
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
        scale = rpe_pair_focal<CAM>(K, cam, lv.lk.b);
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
            bm_view<true>(R, t, scale, cX + 3 * c, cq[2 * c], cq[2 * c + 1], rx, ry, Jx, Jy);
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
            bm_view<false>(Rn, tn, scale, cX + 3 * c, cq[2 * c], cq[2 * c + 1], rx, ry, nullptr, nullptr);
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
        for (int e = 0; e < 9; ++e) R[e] = Rt[e];                            // the pose returned: the polished one, or the winner
#pragma unroll
        for (int e = 0; e < 3; ++e) t[e] = Rt[9 + e];
        rigid_convention(lv.b2, R, t, Ro, to);
        pose_store(Rout + link * 9, tout + link * 3, Ro, to);
        counts[link * 2] = n; counts[link * 2 + 1] = win_cnt;
        info[link * 4] = RPE_LINKPOSE_OK; info[link * 4 + 1] = win_it; info[link * 4 + 2] = win_root; info[link * 4 + 3] = polish;
        const double before = m > 0 ? sqrt(cost0 / m) : 0.;
        rms[link * 2] = before;
        rms[link * 2 + 1] = polish > 0 ? sqrt(cost / m) : before;
    }
}

// the correspondence lists of this handle fit the kernel's LDS (else rpe_link_poses creates lp.corr)
bool rpe_link_poses_in_lds(const rpe_handle *h) { return LinkPoseLds(h->cfg.max_matches, h->lay.kcap).corr_in_lds; }

// the links in link.links over the last run r (its d_status / d_m_n / d_R / d_t, match indices, d_n1 / d_n2 and the structure
// buffers) -> lp.*.  Above LP_LDS_MATCHES the lists go to lp.corr, which the caller has allocated.
void rpe_launch_link_poses(rpe_handle *h, const RpeRun &r, int L, int iters, double threshold_px, int min_shared, int refine_iters)
{
    const RpeLinkSrc src = rpe_link_src(h);
    const LinkPoseLds lay(src.max_matches, src.kcap);
    assert(lay.total <= LINK_POSE_LDS_MAX);
    launch_cam(r, link_pose_kernel<true>, link_pose_kernel<false>, dim3(L), dim3(256), lay.total, h->stream, src,
               (const unsigned short *)h->d_subsets, (const double *)h->d_K, r.cam, threshold_px, iters, h->cfg.ransac_max_iters,
               min_shared, refine_iters, lay.corr_in_lds ? (double *)nullptr : h->lp.corr,
               h->lp.R, h->lp.t, h->lp.mask, h->lp.counts, h->lp.info, h->lp.rms);
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
//            and in ba.state above it, walked through the same pointers in the same order; the observations are read
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
    bm_view<true>(RA, tA, fa, X, q[2], q[3], p.e[2], p.e[3], Jx, Jy);
#pragma unroll
    for (int k = 0; k < 3; ++k) { p.JA[0][k] = Jx[k]; p.JA[1][k] = Jy[k]; }
    bm_point_rows(Jx, Jy, RA, p.JX[2], p.JX[3]);
    p.JA[0][3] = (Jx[3] * b1[0] + Jx[4] * b1[1]) + Jx[5] * b1[2]; p.JA[0][4] = (Jx[3] * b2[0] + Jx[4] * b2[1]) + Jx[5] * b2[2];
    p.JA[1][3] = (Jy[3] * b1[0] + Jy[4] * b1[1]) + Jy[5] * b1[2]; p.JA[1][4] = (Jy[3] * b2[0] + Jy[4] * b2[1]) + Jy[5] * b2[2];
    if (hc) {
        bm_view<true>(RC, tC, fc, X, q[4], q[5], p.e[4], p.e[5], p.JC[0], p.JC[1]);
        bm_point_rows(p.JC[0], p.JC[1], RC, p.JX[4], p.JX[5]);
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
// 22; bm_block_row over the six rows in ascending order), g_p = Jp'r and W = Jc'Jp (rows 0..4: A, 5..10: C).  False when V
// is singular.  The inverse stands before W: behind it, bundle_kernel took 113 more vector instructions and 4 % more time.
__device__ __forceinline__ bool ba_block(const BaPoint &p, double lambda, double (&Vi)[6], double (&gp)[3], double (&W)[11][3])
{
    double v[6] = {0., 0., 0., 0., 0., 0.};
    gp[0] = 0.; gp[1] = 0.; gp[2] = 0.;
#pragma unroll
    for (int r = 0; r < 6; ++r) bm_block_row(p.JX[r], p.e[r], v, gp);
    const bool regular = bm_damped_inverse(v, lambda, Vi);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 5; ++k) W[k][i] = p.JA[0][k] * p.JX[2][i] + p.JA[1][k] * p.JX[3][i];
#pragma unroll
        for (int k = 0; k < 6; ++k) W[5 + k][i] = p.JC[0][k] * p.JX[4][i] + p.JC[1][k] * p.JX[5][i];
    }
    return regular;
}

template <bool CAM>
__global__ __launch_bounds__(256) void bundle_gather_kernel(const RpeLinkSrc src, const double *__restrict__ K, const RpeCamSrc cam,
                                                             const double *__restrict__ Rb_in, const double *__restrict__ tb_in,
                                                             double threshold_px, uint8_t *__restrict__ views,
                                                             double *__restrict__ obs, double *__restrict__ X0,
                                                             double *__restrict__ pose0, double *__restrict__ focal,
                                                             int *__restrict__ pre, int *__restrict__ n_in)
{
    extern __shared__ unsigned s_ba_tab[];
    const int link = blockIdx.x, tid = threadIdx.x, max_matches = src.max_matches;
    const LinkView lv(src, link);
    const long long om = (long long)link * max_matches;
    double Rb[9], tb[3];
    pose_load(Rb_in + link * 9, tb_in + link * 3, Rb, tb);
    bool zero = true;
#pragma unroll
    for (int e = 0; e < 9; ++e) zero = zero && Rb[e] == 0.;
    const int code = src.status[lv.lk.a] != RPE_PAIR_OK ? RPE_BUNDLE_PAIR_FAILED : (zero ? RPE_BUNDLE_SKIPPED : RPE_BUNDLE_OK);
    if (code == RPE_BUNDLE_PAIR_FAILED) {                                    // workgroup-uniform
        for (int i = tid; i < max_matches; i += 256) {
            views[om + i] = 0;
            X0[(om + i) * 3] = 0.; X0[(om + i) * 3 + 1] = 0.; X0[(om + i) * 3 + 2] = 0.;
        }
        if (tid < RPE_BUNDLE_POSE_DOUBLES) pose0[link * RPE_BUNDLE_POSE_DOUBLES + tid] = 0.;
        if (tid < 2) focal[link * 2 + tid] = 0.;
        if (tid == 0) { pre[link] = code; n_in[link] = 0; }
        return;
    }
    link_join<false>(s_ba_tab, src, lv);
    double Ra[9], ta[3], RC[9], tC[3], RtC[LP_POSE_DOUBLES];
    pose_load(src.R + lv.lk.a * 9, src.t + lv.lk.a * 3, Ra, ta);
    rigid_convention(lv.b2, Rb, tb, RC, tC);                                 // the solved form of C: S -> C
    pose_store(RtC, RtC + 9, RC, tC);
    const double fa = rpe_pair_focal<CAM>(K, cam, lv.lk.a), fc = rpe_pair_focal<CAM>(K, cam, lv.lk.b);
    const double thr = threshold_px / fc, thr2 = thr * thr;
    const double2 *oS = (lv.a2 ? src.n2 : src.n1) + lv.oa, *oA = (lv.a2 ? src.n1 : src.n2) + lv.oa, *oC = (lv.b2 ? src.n1 : src.n2) + lv.ob;
    for (int i = tid; i < max_matches; i += 256) {
        int v = 0;
        double X[3] = {0., 0., 0.};
        if (i < lv.na && link_usable(src, lv.oa, i)) {
            const unsigned e = link_entry(s_ba_tab, src.kcap, lv.key_a[i]);
            if (link_a_won(e, i)) {
                v = 1;
                link_point(src.points + (lv.oa + i) * 3, Ra, ta, lv.a2, X[0], X[1], X[2]);
                double *o = obs + (om + i) * RPE_BUNDLE_OBS_DOUBLES;
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
        double RA[9], tA[3];
        rigid_convention(lv.a2, Ra, ta, RA, tA);                             // the solved form of A: S -> A
        double *o = pose0 + link * RPE_BUNDLE_POSE_DOUBLES;
        pose_store(o, o + 9, RA, tA);
        pose_store(o + 12, o + 21, RC, tC);
        focal[link * 2] = fa; focal[link * 2 + 1] = fc;
        pre[link] = code; n_in[link] = lv.na;
    }
}

// The kernel's dynamic LDS, for the kernel's carve-up and the launcher's size: the point state (X and the trial X, 6 f64 per
// point) at 0 when state_in_lds, else it is in ba.state; the byte offset of the index list [max_matches rounded up to 8]
// u16; the size
struct BundleLds {
    bool state_in_lds = false;
    size_t idx = 0, total = 0;
    __host__ __device__ constexpr BundleLds(int max_matches)
    {
        state_in_lds = max_matches <= BA_LDS_MATCHES;
        idx = state_in_lds ? sizeof(double) * RPE_BUNDLE_STATE_DOUBLES * (size_t)max_matches : 0;
        total = idx + sizeof(unsigned short) * (size_t)((max_matches + 7) & ~7);
    }
};
static_assert(BundleLds(BA_LDS_MATCHES).total <= RPE_LDS_DEFAULT_BYTES && BundleLds(RPE_MAX_MATCHES_LIMIT).total <= RPE_LDS_DEFAULT_BYTES,
              "the layout at the cut and at the largest max_matches fits the default dynamic LDS");

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
    const BundleLds lay(max_matches);
    double *sX = state ? state + om * RPE_BUNDLE_STATE_DOUBLES : (double *)s_ba, *sXn = sX + 3 * (size_t)max_matches;     // [n][3] each
    unsigned short *s_idx = (unsigned short *)(s_ba + lay.idx);
    const int M = min(max(n_in[prob], 0), max_matches);
    uint8_t *vw = views + om;
    double *pts = points + om * 3;
    const double *ob = obs + om * RPE_BUNDLE_OBS_DOUBLES;
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
    const double *p0 = pose0 + prob * RPE_BUNDLE_POSE_DOUBLES;                                    // the start poses: S -> A, S -> C
    // not two pose_load: with the two poses loaded one after the other instead of element by element, this kernel (500 of
    // 512 VGPRs) spilled 80 of them in the loop below (profiles/r14_kernel_resources.md)
#pragma unroll
    for (int e = 0; e < 9; ++e) { RA[e] = pose0[prob * RPE_BUNDLE_POSE_DOUBLES + e]; RC[e] = pose0[prob * RPE_BUNDLE_POSE_DOUBLES + 12 + e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) { tA[e] = pose0[prob * RPE_BUNDLE_POSE_DOUBLES + 9 + e]; tC[e] = pose0[prob * RPE_BUNDLE_POSE_DOUBLES + 21 + e]; }
    const double fa = focal[prob * 2], fc = focal[prob * 2 + 1];
    double lam = 0.;                                                         // the damping solve() met last: trial() builds the same blocks
    auto point = [&](int j, BaPoint &p) {
        const int i = s_idx[j];
        ba_point(RA, tA, b1, b2, RC, tC, fa, fc, sX + 3 * j, ob + RPE_BUNDLE_OBS_DOUBLES * i, vw[i] == 3, p);
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
                const double Y[3] = {bm_sym_row(Vi, 0, W[k]), bm_sym_row(Vi, 1, W[k]), bm_sym_row(Vi, 2, W[k])};
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
            for (int i = 0; i < 3; ++i) { Xn[i] = sX[3 * j + i] - bm_sym_row(Vi, i, u); sXn[3 * j + i] = Xn[i]; }
            const double *q = ob + RPE_BUNDLE_OBS_DOUBLES * s_idx[j];
            double e[6];
            e[0] = fa * (Xn[0] / Xn[2] - q[0]); e[1] = fa * (Xn[1] / Xn[2] - q[1]);
            bm_view<false>(RAn, tAn, fa, Xn, q[2], q[3], e[2], e[3], nullptr, nullptr);
            e[4] = 0.; e[5] = 0.;
            if (vw[s_idx[j]] == 3) bm_view<false>(RCn, tCn, fc, Xn, q[4], q[5], e[4], e[5], nullptr, nullptr);
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
        double Ro[9], to[3];
        if (take || !links) {
            if (!take) { pose_load(p0, p0 + 9, RA, tA); pose_load(p0 + 12, p0 + 21, RC, tC); }
            rigid_convention(sa != 0, RA, tA, Ro, to);
            pose_store(Ra_out + prob * 9, ta_out + prob * 3, Ro, to);
            rigid_convention(sb != 0, RC, tC, Ro, to);
            pose_store(Rb_out + prob * 9, tb_out + prob * 3, Ro, to);
        } else {
            pose_load(Rall + pa * 9, tall + pa * 3, Ro, to);
            pose_store(Ra_out + prob * 9, ta_out + prob * 3, Ro, to);
            pose_load(Rb_in + prob * 9, tb_in + prob * 3, Ro, to);
            pose_store(Rb_out + prob * 9, tb_out + prob * 3, Ro, to);
        }
        counts[prob * 2] = n; counts[prob * 2 + 1] = n3;
        info[prob * 4] = take ? RPE_BUNDLE_OK : RPE_BUNDLE_REJECTED; info[prob * 4 + 1] = iters; info[prob * 4 + 2] = acc; info[prob * 4 + 3] = 0;
        const double before = sqrt(cost0 / nobs);
        rms[prob * 2] = before;
        rms[prob * 2 + 1] = take ? sqrt(cost / nobs) : before;
    }
}

// the point state of this handle fits the kernel's LDS (else the callers create ba.state)
bool rpe_bundles_in_lds(const rpe_handle *h) { return BundleLds(h->cfg.max_matches).state_in_lds; }

// n problems whose arrays are in ba.* (the stage form uploaded them, or the gather below wrote them) -> ba.* results
void rpe_launch_bundle(rpe_handle *h, int n, int min_shared, int max_iters, bool links)
{
    const RpeLinkSrc src = rpe_link_src(h);
    const BundleLds lay(src.max_matches);
    hipLaunchKernelGGL(bundle_kernel, dim3(n), dim3(256), lay.total, h->stream, (const int *)h->ba.n, (const int *)h->ba.pre,
                       h->ba.views, (const double *)h->ba.obs, h->ba.points, (const double *)h->ba.pose0, (const double *)h->ba.focal,
                       min_shared, max_iters, src.max_matches, lay.state_in_lds ? (double *)nullptr : h->ba.state,
                       links ? src.links : (const RpeLink *)nullptr, src.points, src.R, src.t,
                       (const double *)h->ba.Rin, (const double *)h->ba.tin,
                       h->ba.Ra, h->ba.ta, h->ba.Rb, h->ba.tb, h->ba.counts, h->ba.info, h->ba.rms);
}

// the links in link.links over the last run r, the callers' poses of pair b in ba.Rin / ba.tin -> the problems' arrays
void rpe_launch_bundle_gather(rpe_handle *h, const RpeRun &r, int L, double threshold_px)
{
    const RpeLinkSrc src = rpe_link_src(h);
    // the table is all of the kernel's LDS: the largest (RPE_MAX_KCAP = 16384 entries) is exactly the default dynamic LDS
    static_assert(sizeof(unsigned) * RPE_MAX_KCAP <= RPE_LDS_DEFAULT_BYTES, "the largest table needs no raised limit");
    const size_t lds = sizeof(unsigned) * (size_t)src.kcap;
    launch_cam(r, bundle_gather_kernel<true>, bundle_gather_kernel<false>, dim3(L), dim3(256), lds, h->stream, src,
               (const double *)h->d_K, r.cam, (const double *)h->ba.Rin, (const double *)h->ba.tin, threshold_px,
               h->ba.views, h->ba.obs, h->ba.points, h->ba.pose0, h->ba.focal, h->ba.pre, h->ba.n);
}

// The kernels of this file that launch above the default dynamic LDS.  bundle_gather_kernel and bundle_kernel stay at or
// below it (the static_asserts at the launcher and at BundleLds).
std::vector<RpeLdsCeiling> rpe_link_lds_ceilings()
{
    return {{(const void *)scale_links_kernel, "scale_links_kernel", SCALE_LINKS_LDS_MAX},
            {(const void *)link_pose_kernel<true>, "link_pose_kernel<true>", LINK_POSE_LDS_MAX},
            {(const void *)link_pose_kernel<false>, "link_pose_kernel<false>", LINK_POSE_LDS_MAX}};
}
