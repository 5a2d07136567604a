// Host harness for the workgroup form of relative_pose_estimation_amd/csrc/retain_best_emul.h
// (tests/test_retain_block_cpu.py, tests/test_gpu_orb_retain_block.py): rb::block_pair_swap_model -- the per-wave-slice
// arithmetic of the device routine -- against the sequential scans, the whole workgroup procedure against the REAL
// std::nth_element + std::partition of this container, and the sequential rb::retain_best on the two element kinds of
// the selection kernels as the reference of the GPU test.  With -DRBK_MAIN the same checks run as a stand-alone program
// over a case file (the sanitizer build).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../relative_pose_estimation_amd/csrc/retain_best_emul.h"

namespace {
// kind 0: u32 FAST entries (score << 24 | y << 12 | x), compared on the score; kind 1: u64 Harris entries
// (f32 response bits << 32 | y << 16 | x), compared as floats -- the comparators of orb_kernels.hip
struct FastGT { bool operator()(uint32_t a, uint32_t b) const { return (a >> 24) > (b >> 24); } };
struct FastGE { bool operator()(uint32_t a, uint32_t b) const { return (a >> 24) >= (b >> 24); } };
inline float resp_of(uint64_t e) { const uint32_t u = (uint32_t)(e >> 32); float f; std::memcpy(&f, &u, 4); return f; }
struct HarrisGT { bool operator()(uint64_t a, uint64_t b) const { return resp_of(a) > resp_of(b); } };
struct HarrisGE { bool operator()(uint64_t a, uint64_t b) const { return resp_of(a) >= resp_of(b); } };

template <class E, class GT, class GE> int retain_real(std::vector<E> &a, int n_points, GT gt, GE ge)
{
    // cv::KeyPointsFilter::retainBest on the real library (libstdc++ here)
    if (n_points >= 0 && a.size() > (size_t)n_points) {
        if (n_points == 0) a.clear();
        else {
            std::nth_element(a.begin(), a.begin() + n_points - 1, a.end(), gt);
            const E amb = a[(size_t)n_points - 1];
            a.resize((size_t)(std::partition(a.begin() + n_points, a.end(), [&](const E &k) { return ge(k, amb); }) - a.begin()));
        }
    }
    return (int)a.size();
}

// sequential libstdc++ procedure with a depth limit (0: heap_select from the start)
template <class E, class GT, class GE> int retain_seq_depth(E *a, int n, int n_points, int depth, GT gt, GE ge)
{
    if (!(n_points >= 0 && n > n_points)) return n;
    if (n_points == 0) return 0;
    rb::gnu_nth_element(a, n, n_points - 1, gt, depth);
    const E amb = a[n_points - 1];
    return rb::partition_pred(a, n_points, n, [&](const E &x) { return ge(x, amb); });
}

template <class E, class GT, class GE> int check(const E *src, int n, int op, int a1, int a2, int nwaves, GT gt, GE ge)
{
    std::vector<E> a(src, src + n), b;
    int r1, r2;
    if (op == 0) {                                // one introselect round on [0, n): median to first, unguarded partition of [1, n)
        if (n < 4) return -1;                     // libstdc++ runs it on more than three elements only (no sentinels below)
        rb::gnu_move_median_to_first(a.data(), 0, 1, n / 2, n - 1, gt);
        b = a;
        r1 = rb::gnu_unguarded_partition(a.data(), 1, n, 0, gt);
        const E pv = b[0];
        rb::block_pair_swap_model(b.data(), 1, n, [&](const E &e) { return !gt(e, pv); }, [&](const E &e) { return !gt(pv, e); }, nwaves, &r2);
    } else if (op == 1) {                         // std::partition(a + a1, a + n, e >= amb) with amb = a[a1 - 1]
        if (a1 < 1 || a1 > n) return -1;
        b = a;
        const E amb = a[(size_t)a1 - 1];
        r1 = rb::partition_pred(a.data(), a1, n, [&](const E &x) { return ge(x, amb); });
        int cut, n_rs = 0;
        rb::block_pair_swap_model(b.data(), a1, n, [&](const E &e) { return !ge(e, amb); }, [&](const E &e) { return ge(e, amb); }, nwaves, &cut, &n_rs);
        r2 = a1 + n_rs;
    } else if (op == 2) {                         // retainBest(a1): the workgroup procedure against the real library (depth limit a2 >= 0: against the sequential restatement)
        b = a;
        if (a2 < 0) r1 = retain_real(a, a1, gt, ge);
        else { r1 = retain_seq_depth(a.data(), n, a1, a2, gt, ge); }
        r2 = rb::block_retain_best_gnu_model(b.data(), n, a1, gt, ge, nwaves, a2);
        if (r1 != r2) return 0;
        for (int i = 0; i < r1; ++i) if (a[(size_t)i] != b[(size_t)i]) return 0;
        return 1;
    } else
        return -1;
    if (r1 != r2) return 0;
    for (int i = 0; i < n; ++i) if (a[(size_t)i] != b[(size_t)i]) return 0;
    return 1;
}
}   // namespace

// 1: equal, 0: different, -1: not a case
extern "C" int rbk_check(int kind, const void *elems, int n, int op, int a1, int a2, int nwaves)
{
    return kind ? check((const uint64_t *)elems, n, op, a1, a2, nwaves, HarrisGT(), HarrisGE())
                : check((const uint32_t *)elems, n, op, a1, a2, nwaves, FastGT(), FastGE());
}

// the sequential rb::retain_best in place; returns the new size
extern "C" int rbk_retain(int kind, void *elems, int n, int n_points, int runtime)
{
    return kind ? rb::retain_best((uint64_t *)elems, n, n_points, runtime, HarrisGT(), HarrisGE())
                : rb::retain_best((uint32_t *)elems, n, n_points, runtime, FastGT(), FastGE());
}

#ifdef RBK_MAIN
// case file: records of three int32 (kind, n, checks), then per check five int32 (op, a1, a2, nwaves, want), then the n
// elements; op 3 = rbk_retain with runtime a2 (only run, for the sanitizers).  Exit status 0 when every check returns
// what the file expects.
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    long cases = 0, bad = 0;
    while (std::fread(hdr, sizeof(hdr), 1, f) == 1) {
        const int kind = hdr[0], n = hdr[1];
        std::vector<int32_t> ops((size_t)hdr[2] * 5);
        std::vector<uint64_t> buf((size_t)n + 1), work;
        if (std::fread(ops.data(), 20, (size_t)hdr[2], f) != (size_t)hdr[2]) { std::fclose(f); return 2; }
        if (n && std::fread(buf.data(), kind ? 8 : 4, (size_t)n, f) != (size_t)n) { std::fclose(f); return 2; }
        for (int k = 0; k < hdr[2]; ++k, ++cases) {
            const int32_t *o = &ops[(size_t)k * 5];
            int got = o[4];
            if (o[0] == 3) { work = buf; rbk_retain(kind, work.data(), n, o[1], o[2]); }
            else got = rbk_check(kind, buf.data(), n, o[0], o[1], o[2], o[3]);
            if (got != o[4]) { ++bad; std::fprintf(stderr, "kind %d n %d op %d a1 %d a2 %d nwaves %d -> %d\n", kind, n, o[0], o[1], o[2], o[3], got); }
        }
    }
    std::fclose(f);
    std::printf("%ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
