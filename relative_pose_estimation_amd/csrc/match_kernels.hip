// match_kernels.hip -- brute-force Hamming matcher with OpenCV crossCheck semantics.
//
// Replaces cv2.BFMatcher(NORM_HAMMING, crossCheck=True).match(desc1, desc2)
// + sorted(key=distance) + [:max_matches]   (reference src/core/pose_estimator.py:131,:144-151)
// and the point gather of :518-519 (fused epilogue).
//
// Every configuration has one kernel path.  crossCheck (Hamming and L2) runs on the matrix cores, one workgroup per
// image pair or per tile of one (match_hamming_mfma_kernel, match_l2_mfma_kernel, and the guided kernels next to them).
// Selection follows core/batch_distance.cpp (crosscheck=true) of OpenCV >= 4.5.x, two elections: every train elects its
// nearest query (strict '<', ascending query => lowest index on ties) and every query keeps its best elector as a packed
// (dist<<18 | trainIdx) word under atomicMin (lowest train on ties); every query also finds its OWN nearest train (same
// key, lowest train on ties) and the match survives only if that train elected the query -- the two keys are
// equal exactly then.  The matrix-core kernels take both elections from one pass over the product tiles.  (Rounds 1-2
// ran the first election only, the rule of older OpenCV: a superset.  The reference's result rows single out the
// two-election rule: tests/test_reference_rows_cpu.py.)
// The stable sort by distance is a bitonic sort of (dist<<16 | queryIdx) keys in LDS.
//
// The Lowe-ratio mode is the opt-in extension named by the project brief and absent from the reference (which uses
// crossCheck, pose_estimator.py:131): cv2's knnMatch(k=2) + Lowe's ratio test.  It runs on the vector ALU, and these
// are the only vector-ALU matchers (match_hamming_ratio_kernel: 8 x (v_xor_b32 + v_bcnt_u32_b32) per distance;
// match_l2_ratio_kernel): a lane owns a QUERY descriptor, the TRAIN descriptors stream through LDS; the lane keeps its
// best (distance, lowest train index) and second-best distance and emits the match iff  best < ratio * second
// (compared in f64, as Python compares m.distance < ratio * n.distance); queries with fewer than two candidates emit
// nothing.
//
// What the file shares.  Every matcher -- the ratio kernels, the fused matrix-core and guided kernels, the Hamming and
// the L2 select kernels -- ends in ONE tail, select_sort_emit<NT, Key>: keys from the election words, their count, the
// bitonic sort, the first max_matches ranks with the point gather (MatchOut), m_n.  A caller states only which query
// survives (the ratio flag, best == row, the raw row key's conversion, nn_q[nn_t[i]] == i) and where its train index is.
// The two matrix-core Hamming kernels (crossCheck, guided) share popc256, fill_qpop and load_owner but keep their own tile
// loops (the lesson at rpe_pair_slots), and ONE launch plan, rpe_hamming_plan: the LDS regions, the split over workgroups
// and whether the election words live in LDS (fused kernel) or in HBM (tile kernel + match_hamming_select_kernel) are decided
// there, for both launchers (launch_hamming_plan) and for the allocation of the HBM words (rpe_api.hip).
#include "rpe_internal.h"
#include "hamming_tiles.h"
#include <algorithm>

#define QTILE 1024

__device__ __forceinline__ int ham256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y); d += __popc(a0.z ^ b0.z); d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x); d += __popc(a1.y ^ b1.y); d += __popc(a1.z ^ b1.z); d += __popc(a1.w ^ b1.w);
    return d;
}

// ---------------------------------------------------------------- the tail of every matcher
// Where the matches of one pair go: its max_matches output rows and the keypoints of its two images
template <typename Dist>
struct MatchOut {
    int *q, *t;
    Dist *d;
    float2 *p1, *p2;
    const float2 *kp1, *kp2;
    __device__ MatchOut(int pair, int max_matches, int img1, int img2, int kcap, const float2 *kp_pt,
                        int *m_q, int *m_t, Dist *m_d, float2 *pts1, float2 *pts2)
    {
        const long long o = (long long)pair * max_matches;
        q = m_q + o; t = m_t + o; d = m_d + o; p1 = pts1 + o; p2 = pts2 + o;
        kp1 = kp_pt + (long long)img1 * kcap; kp2 = kp_pt + (long long)img2 * kcap;
    }
    __device__ void put(int r, int i, int j, Dist dist) const
    {
        q[r] = i; t[r] = j; d[r] = dist;
        p1[r] = kp1[i]; p2[r] = kp2[j];
    }
};

// One workgroup of NT threads: the sort key of every query i < n1 from key_of(i) -- (distance << 16 | i), or all ones for
// "no match", which sorts to the end -- a bitonic sort of the next power of two (>= 64) of keys in s_key (ascending: the
// stable sort by distance, the query index breaks ties), then emit(r, i, key) for the first min(valid, max_matches) ranks
// and their number to *n_out.  It opens with a barrier: what the workgroup wrote before the call is visible to key_of, and
// s_key may alias LDS that was read until then -- but nothing that key_of itself reads.
template <int NT, typename Key, typename KeyOf, typename Emit>
__device__ __forceinline__ void select_sort_emit(Key *s_key, int n1, int max_matches, int *n_out, KeyOf key_of, Emit emit)
{
    __shared__ int s_valid;
    constexpr Key NONE = ~(Key)0;
    const int tid = threadIdx.x;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    int sortP = 64;
    while (sortP < n1) sortP <<= 1;
    int myvalid = 0;
    for (int i = tid; i < sortP; i += NT) {
        Key key = NONE;
        if (i < n1) { key = key_of(i); if (key != NONE) ++myvalid; }
        s_key[i] = key;
    }
    if (myvalid) atomicAdd(&s_valid, myvalid);
    __syncthreads();
    for (int k = 2; k <= sortP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (sortP >> 1); t += NT) {
                int i = 2 * j * (t / j) + (t % j);
                int ixj = i + j;
                bool asc = (i & k) == 0;
                Key a = s_key[i], b = s_key[ixj];
                if ((a > b) == asc) { s_key[i] = b; s_key[ixj] = a; }
            }
            __syncthreads();
        }
    }
    const int nm = min(s_valid, max_matches);
    for (int r = tid; r < nm; r += NT) {
        const Key key = s_key[r];
        emit(r, (int)(key & 0xFFFF), key);
    }
    if (tid == 0) *n_out = nm;
}

// The Hamming matchers' sort key of query i from its election word b = (dist << 18 | trainIdx)
__device__ __forceinline__ unsigned ham_sort_key(unsigned b, int i) { return ((b >> 18) << 16) | (unsigned)i; }

// The Lowe-ratio Hamming matcher: one workgroup (256 lanes) per pair, a lane owns one QUERY descriptor (8 dwords in
// registers), the train descriptors stream through LDS in QTILE-row tiles and are read back as wave-uniform ds_read_b128.
template <bool TAB>
__global__ __launch_bounds__(256) void match_hamming_ratio_kernel(const uint8_t *__restrict__ desc, const int *__restrict__ kp_count,
                                                                   const float2 *__restrict__ kp_pt, int img2_base, const int2 *__restrict__ pair_tab, int kcap,
                                                                   int max_matches, double ratio,
                                                                   int *__restrict__ m_q, int *__restrict__ m_t, int *__restrict__ m_d,
                                                                   int *__restrict__ m_n, float2 *__restrict__ pts1, float2 *__restrict__ pts2)
{
    extern __shared__ uint4 s_dyn[];
    uint4 *s_t = s_dyn;                                   // QTILE*2 uint4 = 32 KB (later: sort keys)
    unsigned *s_best = (unsigned *)(s_dyn + QTILE * 2);   // kcap entries: (dist << 18 | trainIdx) where the ratio test passed
    const int tid = threadIdx.x, pair = blockIdx.x;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int n1 = min(kp_count[img1], kcap), n2 = min(kp_count[img2], kcap);
    for (int i = tid; i < n1; i += 256) s_best[i] = 0xFFFFFFFFu;
    const uint4 *d1 = (const uint4 *)(desc + (long long)img1 * kcap * 32);
    const uint4 *d2 = (const uint4 *)(desc + (long long)img2 * kcap * 32);
    for (int qc = 0; qc < n1; qc += 256) {
        const int i = qc + tid;
        const bool valid = i < n1;
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        if (valid) { q0 = d1[2 * i]; q1 = d1[2 * i + 1]; }
        int bestd = 0x7FFFFFFF, bestj = 0, second = 0x7FFFFFFF;
        for (int tt = 0; tt < n2; tt += QTILE) {
            const int nt = min(QTILE, n2 - tt);
            __syncthreads();
            for (int idx = tid; idx < nt * 2; idx += 256) s_t[idx] = d2[2 * tt + idx];
            __syncthreads();
            for (int j = 0; j < nt; ++j) {
                const int da = ham256(s_t[2 * j], s_t[2 * j + 1], q0, q1);
                if (da < bestd) { second = bestd; bestd = da; bestj = tt + j; }
                else if (da < second) second = da;
            }
        }
        if (valid && n2 >= 2 && (double)bestd < ratio * (double)second) s_best[i] = ((unsigned)bestd << 18) | (unsigned)bestj;
    }
    // the staging tile becomes the key array
    const MatchOut<int> out(pair, max_matches, img1, img2, kcap, kp_pt, m_q, m_t, m_d, pts1, pts2);
    select_sort_emit<256>((unsigned *)s_t, n1, max_matches, m_n + pair,
        [&](int i) { const unsigned b = s_best[i]; return b != 0xFFFFFFFFu ? ham_sort_key(b, i) : 0xFFFFFFFFu; },
        [&](int r, int i, unsigned key) { out.put(r, i, s_best[i] & 0x3FFFF, (int)(key >> 16)); });
}

// ---------------------------------------------------------------- crossCheck on the matrix cores
// The measured bound of a vector-ALU crossCheck kernel (the ratio kernel's loop without the second best, shipped until
// the matrix-core kernel replaced it) is vector-instruction issue: 19 instructions per 64 distances
// (8 v_xor + 8 v_bcnt + compare / select) at the 4-cycle integer issue cadence = 0.75 ms for 1024 pairs of
// 1000 x 1000 descriptors, 91 % of the measured issue roof (profiles/r02_counters.json, r02_calibration.json).
// Hamming distance is a dot product in disguise: d(q, t) = |q| + |t| - 2 q.t with the 256 bits as 0/1 bytes, so the
// O(N^2) part goes to v_mfma_i32_32x32x32_i8 (exact integers): 8 MFMAs = one 32 x 32 tile of q.t over K = 256.
// What is left for the vector ALU per tile is the O(N) bit -> byte expansion and a 2-instruction epilogue per
// accumulator: key = ((|q| + 512) << 16 | queryIdx) - (q.t << 17) (one v_mad_i32_i24), running v_min_u32 per train
// column -- the minimum of (distance, queryIdx) keys IS batchDistance's "strict <, ascending query" election.  The second
// crossCheck side (the query's own nearest train) reads the SAME accumulators: q.t is symmetric, so the tile that elects
// along its columns elects along its rows too.  Row key = ((|t| + 512) << 16 | trainIdx) - (q.t << 17), one v_add on the
// product already formed for the column key; its minimum over a row's 32 columns is a transpose reduction across the lanes
// (row_min32: 39 vector instructions per tile), joined over the 8 waves and the rounds by one atomicMin per row into s_row.
// (Until round 5 a second pass ran the same loop with the descriptor sets swapped: 16 MFMAs and 128 vector instructions
// per tile pair where this form has 8 and 106; 0.52 -> 0.37 ms per 1024 pairs)  s_row holds the raw key; it
// is converted to the election words' (dist << 18 | trainIdx) once per query, before the two are compared.
// Workgroup = one pair, 8 waves; wave w owns train tile 8 p + w of round p (its 32 descriptors expanded once into
// 32 VGPRs: the B operand of all 8 K-steps), the query tiles stream through LDS, expanded by all 512 threads
// (16 bits -> 16 bytes: nibble * 0x00204081 & 0x01010101), double buffered: one barrier per query tile.
// The tile helpers (expand16, fill_qpop, load_owner, row_min32 -- its transpose reduction is told there) and the staging
// constants are in hamming_tiles.h, shared with similar_kernels.hip.

// SPLIT = true: small batches (the drop-in's estimate() is a batch of ONE pair: a single workgroup walked 2 x 127 x 127 tiles
// alone, 2.3 ms of a 2.9 ms call).  The rounds of 8 owner tiles are dealt over gridDim.y workgroups per pair, the election
// words live in HBM (integer atomicMin: order independent), and match_hamming_select_kernel sorts and emits afterwards.
template <bool SPLIT, bool TAB>
__global__ __launch_bounds__(MM_NT) void match_hamming_mfma_kernel(const uint8_t *__restrict__ desc, const int *__restrict__ kp_count,
                                                                    const float2 *__restrict__ kp_pt, int img2_base, const int2 *__restrict__ pair_tab, int kcap,
                                                                    int max_matches, int region0,
                                                                    unsigned *__restrict__ g_best, unsigned *__restrict__ g_row,
                                                                    int *__restrict__ m_q, int *__restrict__ m_t, int *__restrict__ m_d,
                                                                    int *__restrict__ m_n, float2 *__restrict__ pts1, float2 *__restrict__ pts2)
{
    extern __shared__ uint4 s_dyn[];
    // [0, region0 x 16 B): two expanded scanned tiles (2 x 8 K-steps x 64 lanes x 16 B = 16 KB) + their packed (|x| + 512, index)
    // words + the popcounts; reused as the sort-key array afterwards.  Then kcap election words and kcap own-nearest words.
    v4i_t *s_a = (v4i_t *)s_dyn;                               // [2][8][64]
    unsigned *s_qpk = (unsigned *)(s_dyn + 2 * 8 * 64);        // [2][32]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, pair = blockIdx.x;
    unsigned *s_best = SPLIT ? g_best + (long long)pair * kcap : (unsigned *)(s_dyn + region0);          // kcap entries
    unsigned *s_row = SPLIT ? g_row + (long long)pair * kcap : s_best + kcap;     // kcap entries: the query's own nearest train, as the raw row key
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int n1 = min(kp_count[img1], kcap), n2 = min(kp_count[img2], kcap);
    if (!SPLIT) for (int i = tid; i < n1; i += MM_NT) { s_best[i] = 0xFFFFFFFFu; s_row[i] = 0xFFFFFFFEu; }      // SPLIT: the host memsets them
    // |q| + 512 of every query, once (the rounds over the query tiles all need them, and so does the row key's conversion);
    // kept in the free part of the first 32 KB (kcap <= 8064 entries)
    unsigned short *s_qpop = (unsigned short *)(s_dyn + MM_STAGE);
    const int h = lane >> 5, col = lane & 31;
    // this thread's share of a scanned tile's expansion: item = tid: K-step s = tid >> 6, lane slot l = tid & 63
    // (row = l & 31, half = l >> 5): the 16 bits [32 s + 16 half, +16) of scanned descriptor (tile * 32 + row)
    const int xs = tid >> 6, xl = tid & 63, xrow = xl & 31, xh = xl >> 5;
    // the TRAINS own the MFMA columns and elect their nearest query (the queries are scanned through LDS): a minimum down
    // each column, carried in best_key over the query tiles.  The same accumulators elect every query's own nearest train: a
    // minimum along each row (row_min32), joined over the 8 waves and the rounds by an atomicMin on s_row.
    const int n_own = n2, n_scan = n1;
    const unsigned *q32 = (const unsigned *)(desc + (long long)img1 * kcap * 32);      // scanned: 8 dwords per descriptor
    const uint4 *d2 = (const uint4 *)(desc + (long long)img2 * kcap * 32);             // owners
    fill_qpop(s_qpop, (const uint4 *)q32, n_scan);
    const bool c3 = (lane & 8) != 0, c2 = (lane & 4) != 0, c1 = (lane & 2) != 0;
    const int rrow = ((col >> 1) & 3) + 8 * (col >> 3) + 4 * h;      // the row whose minimum row_min32 leaves in this lane
    const int ntq = (n_scan + 31) >> 5, ntt = (n_own + 31) >> 5;
    for (int tt0 = SPLIT ? 8 * (int)blockIdx.y : 0; tt0 < ntt && n_scan > 0; tt0 += SPLIT ? 8 * (int)gridDim.y : 8) {
        const int tt = tt0 + wv;                               // wave-uniform
        const int j = tt * 32 + col;
        const bool valid_t = tt < ntt && j < n_own;
        v4i_t bop[8];
        const int tpop = load_owner(bop, d2, j, valid_t, h);
        unsigned best_key = 0xFFFFFFFFu;
        // row key of this lane's column: (|t| + 512 - 2 q.t) << 16 | trainIdx; its minimum over the trains is the query's nearest
        // train, lowest index on ties (|q| is the same along a row).  Columns past the end: a key no real distance can beat.
        const unsigned tpk = ((valid_t ? (unsigned)tpop + 512u : 0x7000u) << 16) | (unsigned)j;
        // The raw scanned words are fetched MM_PF tiles ahead into a register ring: with a one-tile lookahead every step of
        // the loop waited for an L2 round trip (diagnostic build: the loop without its MFMAs took 0.17 of the kernel's
        // 0.35 ms -- 128 steps of 1.3 us).  The loop is unrolled by MM_PF so that the ring is indexed statically.
        unsigned ring[MM_PF];
        auto fetch = [&](int qt) -> unsigned {
            const int q = qt * 32 + xrow;
            return (qt < ntq && q < n_scan) ? q32[(long long)q * 8 + xs] : 0u;
        };
        auto stage = [&](int qt, int buf, unsigned raw) {
            s_a[(buf * 8 + xs) * 64 + xl] = expand16((raw >> (16 * xh)) & 0xFFFFu);
            if (tid < 32) {
                const int qq = qt * 32 + tid;
                const unsigned pk = qq < n_scan ? (unsigned)s_qpop[qq] : 0x7000u;      // rows past the end: a key no real distance can beat
                s_qpk[buf * 32 + tid] = (pk << 16) | (unsigned)qq;
            }
        };
        __syncthreads();                                       // the previous round has finished reading both buffers (and s_qpop is complete)
#pragma unroll
        for (int u = 0; u < MM_PF; ++u) ring[u] = fetch(u);    // tiles 0 .. MM_PF - 1 in flight
        stage(0, 0, ring[0]);
        ring[0] = fetch(MM_PF);
        __syncthreads();
        for (int qt0 = 0; qt0 < ntq; qt0 += MM_PF) {
#pragma unroll
            for (int u = 0; u < MM_PF; ++u) {
                const int qt = qt0 + u;
                if (qt < ntq) {                                // workgroup-uniform
                    const int buf = qt & 1;
                    if (tt < ntt) {
                        v16i_t acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                        for (int sK = 0; sK < 8; ++sK)
                            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(s_a[(buf * 8 + sK) * 64 + lane], bop[sK], acc, 0, 0, 0);
                        // C layout (dtype independent): column = lane & 31, row of register r = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                        unsigned rk[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned qpk = s_qpk[buf * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
                            const unsigned prod = (unsigned)__mul24(acc[r], -131072);
                            best_key = min(best_key, prod + qpk);                                   // (|q| + 512 - 2 q.t) << 16 | queryIdx
                            rk[r] = prod + tpk;
                        }
                        const unsigned rmin = row_min32(rk, c3, c2, c1);
                        const int q = qt * 32 + rrow;
                        if (!(col & 1) && q < n_scan) atomicMin(&s_row[q], rmin);                  // rows past the end write nothing
                    }
                    if (qt + 1 < ntq) {
                        // tile qt + 1 sits in ring slot (u + 1) % MM_PF (tile 0 of this round was staged in the prologue)
                        stage(qt + 1, buf ^ 1, ring[(u + 1) % MM_PF]);
                        ring[(u + 1) % MM_PF] = fetch(qt + 1 + MM_PF);
                    }
                    __syncthreads();
                }
            }
        }
        best_key = min(best_key, (unsigned)__shfl_xor((int)best_key, 32));
        if (valid_t && h == 0) {
            const unsigned d = (best_key >> 16) - 512u + (unsigned)tpop, i = best_key & 0xFFFFu;
            atomicMin(&s_best[i], (d << 18) | (unsigned)j);                     // train j elects query i
        }
    }
    __syncthreads();
    if (SPLIT) return;
    // the row keys in the election words' format, (dist << 18) | trainIdx: dist = (key >> 16) - 512 + |q|.  The initial value
    // (no train at all) keeps a train index that no election word holds.
    for (int i = tid; i < n1; i += MM_NT) {
        const unsigned k = s_row[i];
        s_row[i] = (((k >> 16) - 1024u + (unsigned)s_qpop[i]) << 18) | (k & 0xFFFFu);
    }
    // the key array takes the place of the staging region (and of s_qpop: converted above, not in key_of)
    const MatchOut<int> out(pair, max_matches, img1, img2, kcap, kp_pt, m_q, m_t, m_d, pts1, pts2);
    select_sort_emit<MM_NT>((unsigned *)s_dyn, n1, max_matches, m_n + pair,
        [&](int i) { const unsigned b = s_best[i]; return b != 0xFFFFFFFFu && b == s_row[i] ? ham_sort_key(b, i) : 0xFFFFFFFFu; },
        [&](int r, int i, unsigned key) { out.put(r, i, s_best[i] & 0x3FFFF, (int)(key >> 16)); });
}


// sort + top-max_matches + point gather of a SPLIT run (one workgroup per pair; the same steps as the fused epilogue).
// raw_desc != nullptr: g_row holds match_hamming_mfma_kernel's raw row keys, converted here with |q| counted from the
// descriptors; nullptr: it holds (dist << 18) | trainIdx words already (the guided matcher).
template <bool TAB>
__global__ __launch_bounds__(MM_NT) void match_hamming_select_kernel(const unsigned *__restrict__ g_best, const unsigned *__restrict__ g_row,
                                                                      const uint8_t *__restrict__ raw_desc,
                                                                      const int *__restrict__ kp_count, const float2 *__restrict__ kp_pt,
                                                                      int img2_base, const int2 *__restrict__ pair_tab, int kcap, int max_matches,
                                                                      int *__restrict__ m_q, int *__restrict__ m_t, int *__restrict__ m_d,
                                                                      int *__restrict__ m_n, float2 *__restrict__ pts1, float2 *__restrict__ pts2)
{
    extern __shared__ uint4 s_dyn[];
    const int pair = blockIdx.x;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int n1 = min(kp_count[img1], kcap);
    const unsigned *s_best = g_best + (long long)pair * kcap, *s_row = g_row + (long long)pair * kcap;
    const MatchOut<int> out(pair, max_matches, img1, img2, kcap, kp_pt, m_q, m_t, m_d, pts1, pts2);
    select_sort_emit<MM_NT>((unsigned *)s_dyn, n1, max_matches, m_n + pair,
        [&](int i) {
            const unsigned b = s_best[i];
            unsigned row = s_row[i];
            if (raw_desc) {
                const uint4 *q = (const uint4 *)(raw_desc + ((long long)img1 * kcap + i) * 32);
                row = (((row >> 16) - 512u + popc256(q[0], q[1])) << 18) | (row & 0xFFFFu);
            }
            return b != 0xFFFFFFFFu && b == row ? ham_sort_key(b, i) : 0xFFFFFFFFu;
        },
        [&](int r, int i, unsigned key) { out.put(r, i, s_best[i] & 0x3FFFF, (int)(key >> 16)); });
}

// Launches the pair-table instance of a kernel when the feature source carries a table (a pair list), the rule instance
// otherwise (batch, stream, stage API): the two instances share one signature
template <typename Kernel, typename... Args>
static void launch_tab(bool tab, Kernel with_table, Kernel with_rule, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args)
{
    hipLaunchKernelGGL(tab ? with_table : with_rule, grid, block, lds, stream, args...);
}

// The launch plan of the matrix-core Hamming matchers for B pairs of capacity kcap; extra_uint4: what the matcher keeps in the
// first LDS region besides the crossCheck staging (the guided matcher's records).  The ONE statement of the rule: both
// launchers follow it and alloc_workspace sizes the HBM election words from it.
//   region0: max(staging + 2 B per scanned descriptor (|q| + 512), 4 B x sort size) -- the key array reuses it;
//   fused:   region0 + 8 B of election / own-nearest words per keypoint, while that fits 64 KB of LDS per workgroup
//            (kcap <= 4096);
//   hbm:     the words live in HBM and match_hamming_select_kernel sorts and emits -- batches of up to RPE_MATCH_SPLIT_PAIRS
//            pairs whose rounds of 8 owner tiles are dealt over `split` > 1 workgroups (256 in flight at most), and every
//            batch once the fused form does not fit.
RpeHammingPlan rpe_hamming_plan(int kcap, int B, int extra_uint4)
{
    RpeHammingPlan p;
    p.sortP = 64;
    while (p.sortP < kcap) p.sortP <<= 1;
    p.region0 = (int)((std::max((size_t)(MM_STAGE + extra_uint4) * 16 + (size_t)kcap * 2, (size_t)p.sortP * 4) + 15) / 16);
    const int rounds = ((kcap + 31) / 32 + 7) / 8;
    p.split = B <= RPE_MATCH_SPLIT_PAIRS ? std::min(rounds, std::max(1, 256 / B)) : 1;
    const size_t fused = (size_t)p.region0 * 16 + (size_t)kcap * 8;
    p.hbm = p.split > 1 || fused > RPE_LDS_DEFAULT_BYTES;
    p.lds_tile = p.hbm ? (size_t)p.region0 * 16 : fused;
    p.lds_select = (size_t)p.sortP * 4;
    return p;
}

// Where a matcher's launch sequence leaves its matches
struct MatchBufs { int *q, *t, *d, *n; float2 *p1, *p2; };

// The launches of a plan: the fused tile kernel, or the two memsets of the HBM words, the SPLIT tile kernel and the select
// kernel.  k_* : the tile kernel's instances <SPLIT, TAB>; mid: its arguments between max_matches and the HBM words;
// raw_desc: see match_hamming_select_kernel.
template <typename Kernel, typename... Mid>
static void launch_hamming_plan(rpe_handle *h, const RpeRun &r, const RpeHammingPlan &p, Kernel k_hbm_tab, Kernel k_hbm, Kernel k_fused_tab, Kernel k_fused,
                                const uint8_t *raw_desc, const MatchBufs &o, Mid... mid)
{
    const int kcap = h->lay.kcap, B = r.pairs, mm = h->cfg.max_matches;
    const RpeFeatSrc &f = r.feat;                             // the workspace (batch / stream rule) or the frame store (pair table)
    if (!p.hbm) {
        launch_tab(f.tab, k_fused_tab, k_fused, dim3(B), dim3(MM_NT), p.lds_tile, h->stream,
                           f.desc, f.count, f.pt, f.img2_base, f.tab, kcap, mm, mid...,
                           (unsigned *)nullptr, (unsigned *)nullptr, o.q, o.t, o.d, o.n, o.p1, o.p2);
        return;
    }
    hipMemsetAsync(h->d_hm_best, 0xFF, sizeof(unsigned) * (size_t)B * kcap, h->stream);
    hipMemsetAsync(h->d_hm_row, 0xFE, sizeof(unsigned) * (size_t)B * kcap, h->stream);     // above every row key; its train index is no one's
    launch_tab(f.tab, k_hbm_tab, k_hbm, dim3(B, p.split), dim3(MM_NT), p.lds_tile, h->stream,
                       f.desc, f.count, f.pt, f.img2_base, f.tab, kcap, mm, mid...,
                       h->d_hm_best, h->d_hm_row, o.q, o.t, o.d, o.n, o.p1, o.p2);
    launch_tab(f.tab, match_hamming_select_kernel<true>, match_hamming_select_kernel<false>, dim3(B), dim3(MM_NT), p.lds_select, h->stream,
                       (const unsigned *)h->d_hm_best, (const unsigned *)h->d_hm_row, raw_desc, f.count, f.pt,
                       f.img2_base, f.tab, kcap, mm, o.q, o.t, o.d, o.n, o.p1, o.p2);
}

void rpe_launch_match(rpe_handle *h, const RpeRun &r)
{
    const int kcap = h->lay.kcap, B = r.pairs;
    const RpeFeatSrc &f = r.feat;
    if (h->cfg.match_mode == RPE_MATCH_RATIO)                 // staging / sort keys + 4 bytes of election word per keypoint (<= 64 KB at 8064)
        launch_tab(f.tab, match_hamming_ratio_kernel<true>, match_hamming_ratio_kernel<false>, dim3(B), dim3(256), (size_t)QTILE * 32 + (size_t)kcap * 4, h->stream,
                           f.desc, f.count, f.pt, f.img2_base, f.tab, kcap, h->cfg.max_matches, h->cfg.match_ratio,
                           h->d_m_q, h->d_m_t, h->d_m_d, h->d_m_n, h->d_pts1, h->d_pts2);
    else {
        const RpeHammingPlan p = rpe_hamming_plan(kcap, B, 0);
        launch_hamming_plan(h, r, p, match_hamming_mfma_kernel<true, true>, match_hamming_mfma_kernel<true, false>,
                            match_hamming_mfma_kernel<false, true>, match_hamming_mfma_kernel<false, false>, f.desc,
                            MatchBufs{h->d_m_q, h->d_m_t, h->d_m_d, h->d_m_n, h->d_pts1, h->d_pts2}, p.region0);
    }
}

// ---------------------------------------------------------------- guided matching (rpe_guided_matches; NOT in the reference)
// The crossCheck election again, but only among keypoint pairs (i, j) that pass the Sampson test of a given pose (the rule is
// spelled out in include/rpe_amd.h).  A kernel family of its own next to match_hamming_mfma_kernel, whose instances stay the
// code they are (the 1 % lesson at rpe_pair_slots).
//
// Everything of the gate that depends on one keypoint only is computed once per pair by guided_records_kernel, O(N), and
// kept in HBM as one 32-byte record per keypoint:
//   query i (image 1): (l_0, l_1, l_2, s1) -- its epipolar line E x1 in image 2 and l_0^2 + l_1^2
//   train j (image 2): (x2, y2, s2, 0)     -- its normalised point and the squared norm of the first two rows of E^T x2
// The cameras, the focal scale and the pose enter there and nowhere else: the tile kernel has no CAM switch.  thr2 of the
// pair goes to g_thr2; NaN marks a pair that is not to be matched (status not OK under the run's own poses).
template <bool TAB, bool CAM>
__global__ __launch_bounds__(256) void guided_records_kernel(const int *__restrict__ kp_count, const float2 *__restrict__ kp_pt, int img2_base,
                                                              const int2 *__restrict__ pair_tab, int kcap, const double *__restrict__ K,
                                                              const RpeCamSrc cam, const double *__restrict__ R, const double *__restrict__ t,
                                                              const int *__restrict__ status, double gate_px,
                                                              double4 *__restrict__ rec, double *__restrict__ g_thr2)
{
    const int pair = blockIdx.z, side = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int img = side ? img2 : img1;
    if (side == 0 && k == 0) {
        const double thr = gate_px / rpe_pair_focal<CAM>(K, cam, pair);
        g_thr2[pair] = (status && status[pair] != RPE_PAIR_OK) ? __builtin_nan("") : thr * thr;
    }
    if (k >= min(kp_count[img], kcap)) return;
    // E = [t]x R, row by row
    const double *Rp = R + 9 * pair, *tp = t + 3 * pair;
    double E[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) E[r][c] = tp[(r + 1) % 3] * Rp[((r + 2) % 3) * 3 + c] - tp[(r + 2) % 3] * Rp[((r + 1) % 3) * 3 + c];
    const float2 p = kp_pt[(long long)img * kcap + k];
    double x, y;
    if (CAM) {
        const rpe_camera *c1, *c2;
        rpe_pair_cameras(cam, pair, c1, c2);
        const rpe_camera *c = side ? c2 : c1;
        const double2 q = rpe_camera_normalise(c, rpe_camera_has_lens(c), p);
        x = q.x; y = q.y;
    } else {
        const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
        x = ((double)p.x - cx) / fx; y = ((double)p.y - cy) / fy;
    }
    double4 o;
    if (side == 0) {
        const double l0 = (E[0][0] * x + E[0][1] * y) + E[0][2], l1 = (E[1][0] * x + E[1][1] * y) + E[1][2], l2 = (E[2][0] * x + E[2][1] * y) + E[2][2];
        o = make_double4(l0, l1, l2, l0 * l0 + l1 * l1);
    } else {
        const double m0 = (E[0][0] * x + E[1][0] * y) + E[2][0], m1 = (E[0][1] * x + E[1][1] * y) + E[2][1];
        o = make_double4(x, y, m0 * m0 + m1 * m1, 0.);
    }
    rec[((long long)pair * RPE_GUIDED_SIDES + side) * kcap + k] = o;
}

// The tile loop of match_hamming_mfma_kernel (same MFMA tile, key packing and SPLIT form; still one pass per crossCheck
// side, the second with the descriptor sets swapped, writing (dist << 18 | index) row words) with the gate in the
// epilogue.  The records of the 32 scanned rows of a tile travel with the tile: fetched MM_PF tiles ahead by wave 1 (64
// 16-byte pieces), staged in LDS beside s_qpk; the owner lane keeps its own record in registers.  An accumulator entry is
// gated only when its key would lower the column's running minimum -- min over the admissible keys either way, and the
// f64 arithmetic (7 operations) runs for the few entries per column that are records so far.  Rows past the end and lanes
// without an owner carry NaN records: never admissible, so a column without an admissible entry keeps 0xFFFFFFFF and
// elects nobody.  max_distance is applied to the elected key: the nearest admissible neighbour is beyond it exactly when
// every admissible one is.
template <bool SPLIT, bool TAB>
__global__ __launch_bounds__(MM_NT) void match_guided_mfma_kernel(const uint8_t *__restrict__ desc, const int *__restrict__ kp_count,
                                                                   const float2 *__restrict__ kp_pt, int img2_base, const int2 *__restrict__ pair_tab, int kcap,
                                                                   int max_matches, int max_distance, int region0,
                                                                   const double4 *__restrict__ g_rec, const double *__restrict__ g_thr2,
                                                                   unsigned *__restrict__ g_best, unsigned *__restrict__ g_row,
                                                                   int *__restrict__ m_q, int *__restrict__ m_t, int *__restrict__ m_d,
                                                                   int *__restrict__ m_n, float2 *__restrict__ pts1, float2 *__restrict__ pts2)
{
    extern __shared__ uint4 s_dyn[];
    // [0, region0 x 16 B): the crossCheck kernel's staging (16 KB of expanded tiles, 256 B of packed words), 2 KB of scanned
    // records, the popcounts; reused as the sort-key array afterwards.  Then kcap election words and kcap own-nearest words.
    v4i_t *s_a = (v4i_t *)s_dyn;                               // [2][8][64]
    unsigned *s_qpk = (unsigned *)(s_dyn + 2 * 8 * 64);        // [2][32]
    double2 *s_rec = (double2 *)(s_dyn + MM_STAGE);            // [2][32][2]: RPE_GUIDED_LDS_UINT4
    unsigned short *s_qpop = (unsigned short *)(s_dyn + MM_STAGE + RPE_GUIDED_LDS_UINT4);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, pair = blockIdx.x;
    unsigned *s_best = SPLIT ? g_best + (long long)pair * kcap : (unsigned *)(s_dyn + region0);
    unsigned *s_row = SPLIT ? g_row + (long long)pair * kcap : s_best + kcap;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const double thr2 = g_thr2[pair];
    const bool run = thr2 == thr2;                             // NaN: the pair is not matched
    const int n1 = run ? min(kp_count[img1], kcap) : 0, n2 = run ? min(kp_count[img2], kcap) : 0;
    if (!SPLIT) for (int i = tid; i < n1; i += MM_NT) { s_best[i] = 0xFFFFFFFFu; s_row[i] = 0xFFFFFFFEu; }      // SPLIT: the host memsets them
    const int h = lane >> 5, col = lane & 31;
    const int xs = tid >> 6, xl = tid & 63, xrow = xl & 31, xh = xl >> 5;
    const bool rec_loader = wv == 1;                           // piece (row lane >> 1, half lane & 1) of a tile's 32 records
    const double qnan = __builtin_nan("");
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
    const int n_own = pass ? n1 : n2, n_scan = pass ? n2 : n1;
    const unsigned *q32 = (const unsigned *)(desc + (long long)(pass ? img2 : img1) * kcap * 32);      // scanned: 8 dwords per descriptor
    const uint4 *d2 = (const uint4 *)(desc + (long long)(pass ? img1 : img2) * kcap * 32);             // owners
    const double2 *rec_scan = (const double2 *)(g_rec + ((long long)pair * RPE_GUIDED_SIDES + (pass ? 1 : 0)) * kcap);
    const double4 *rec_own = g_rec + ((long long)pair * RPE_GUIDED_SIDES + (pass ? 0 : 1)) * kcap;
    __syncthreads();                                           // the previous pass is done with s_qpop
    fill_qpop(s_qpop, (const uint4 *)q32, n_scan);
    const int ntq = (n_scan + 31) >> 5, ntt = (n_own + 31) >> 5;
    for (int tt0 = SPLIT ? 8 * (int)blockIdx.y : 0; tt0 < ntt && n_scan > 0; tt0 += SPLIT ? 8 * (int)gridDim.y : 8) {
        const int tt = tt0 + wv;                               // wave-uniform
        const int j = tt * 32 + col;
        const bool valid_t = tt < ntt && j < n_own;
        v4i_t bop[8];
        const int tpop = load_owner(bop, d2, j, valid_t, h);
        // the owner's record: pass 0 a train (x2, y2, s2, 0), pass 1 a query (l_0, l_1, l_2, s1)
        const double4 own = valid_t ? rec_own[j] : make_double4(qnan, qnan, qnan, qnan);
        unsigned best_key = 0xFFFFFFFFu;
        unsigned ring[MM_PF];
        double2 ring_rec[MM_PF];
        auto fetch = [&](int qt) -> unsigned {
            const int q = qt * 32 + xrow;
            return (qt < ntq && q < n_scan) ? q32[(long long)q * 8 + xs] : 0u;
        };
        auto fetch_rec = [&](int qt) -> double2 {
            const int q = qt * 32 + (lane >> 1);
            return (rec_loader && qt < ntq && q < n_scan) ? rec_scan[(long long)q * 2 + (lane & 1)] : make_double2(qnan, qnan);
        };
        auto stage = [&](int qt, int buf, unsigned raw, const double2 &rr) {
            s_a[(buf * 8 + xs) * 64 + xl] = expand16((raw >> (16 * xh)) & 0xFFFFu);
            if (tid < 32) {
                const int qq = qt * 32 + tid;
                const unsigned pk = qq < n_scan ? (unsigned)s_qpop[qq] : 0x7000u;
                s_qpk[buf * 32 + tid] = (pk << 16) | (unsigned)qq;
            }
            if (rec_loader) s_rec[buf * 64 + lane] = rr;
        };
        __syncthreads();                                       // the previous round has finished reading both buffers (and s_qpop is complete)
#pragma unroll
        for (int u = 0; u < MM_PF; ++u) { ring[u] = fetch(u); ring_rec[u] = fetch_rec(u); }
        stage(0, 0, ring[0], ring_rec[0]);
        ring[0] = fetch(MM_PF); ring_rec[0] = fetch_rec(MM_PF);
        __syncthreads();
        for (int qt0 = 0; qt0 < ntq; qt0 += MM_PF) {
#pragma unroll
            for (int u = 0; u < MM_PF; ++u) {
                const int qt = qt0 + u;
                if (qt < ntq) {                                // workgroup-uniform
                    const int buf = qt & 1;
                    if (tt < ntt) {
                        v16i_t acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                        for (int sK = 0; sK < 8; ++sK)
                            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(s_a[(buf * 8 + sK) * 64 + lane], bop[sK], acc, 0, 0, 0);
                        // C layout (dtype independent): column = lane & 31, row of register r = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = buf * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            const unsigned key = (unsigned)__mul24(acc[r], -131072) + s_qpk[row];
                            if (key < best_key) {
                                const double2 ra = s_rec[2 * row], rb = s_rec[2 * row + 1];
                                // v from the query's line in both passes; s1 + s2 in that order
                                double v, ss;
                                if (pass == 0) { v = (ra.x * own.x + ra.y * own.y) + rb.x; ss = rb.y + own.z; }
                                else           { v = (own.x * ra.x + own.y * ra.y) + own.z; ss = own.w + rb.x; }
                                if (v * v <= thr2 * ss) best_key = key;
                            }
                        }
                    }
                    if (qt + 1 < ntq) {
                        stage(qt + 1, buf ^ 1, ring[(u + 1) % MM_PF], ring_rec[(u + 1) % MM_PF]);
                        ring[(u + 1) % MM_PF] = fetch(qt + 1 + MM_PF); ring_rec[(u + 1) % MM_PF] = fetch_rec(qt + 1 + MM_PF);
                    }
                    __syncthreads();
                }
            }
        }
        best_key = min(best_key, (unsigned)__shfl_xor((int)best_key, 32));
        if (valid_t && h == 0 && best_key != 0xFFFFFFFFu) {
            const unsigned d = (best_key >> 16) - 512u + (unsigned)tpop, i = best_key & 0xFFFFu;
            if ((int)d <= max_distance) {
                if (pass == 0) atomicMin(&s_best[i], (d << 18) | (unsigned)j);      // train j elects query i
                else s_row[j] = (d << 18) | i;                                      // query j's own nearest admissible train i
            }
        }
    }
    }
    if (SPLIT) return;                                         // match_hamming_select_kernel sorts and emits
    const MatchOut<int> out(pair, max_matches, img1, img2, kcap, kp_pt, m_q, m_t, m_d, pts1, pts2);
    select_sort_emit<MM_NT>((unsigned *)s_dyn, n1, max_matches, m_n + pair,
        [&](int i) { const unsigned b = s_best[i]; return b != 0xFFFFFFFFu && b == s_row[i] ? ham_sort_key(b, i) : 0xFFFFFFFFu; },
        [&](int r, int i, unsigned key) { out.put(r, i, s_best[i] & 0x3FFFF, (int)(key >> 16)); });
}

// What both norms' guided launchers open with: the gm.* lists cleared and the records of the run under the poses
static void launch_guided_records(rpe_handle *h, const RpeRun &r, const double *d_R, const double *d_t, const int *d_status, double gate_px)
{
    const int kcap = h->lay.kcap, B = r.pairs, mm = h->cfg.max_matches;
    const RpeFeatSrc &f = r.feat;
    // -1 / zero past n_matches (an L2 distance of all-ones bits)
    hipMemsetAsync(h->gm.q, 0xFF, sizeof(int) * (size_t)B * mm, h->stream);
    hipMemsetAsync(h->gm.t, 0xFF, sizeof(int) * (size_t)B * mm, h->stream);
    hipMemsetAsync(h->gm.d, 0xFF, sizeof(int) * (size_t)B * mm, h->stream);
    hipMemsetAsync(h->gm.pts1, 0, sizeof(float2) * (size_t)B * mm, h->stream);
    hipMemsetAsync(h->gm.pts2, 0, sizeof(float2) * (size_t)B * mm, h->stream);
    const bool cam = r.cam.cams != nullptr;
    auto records = f.tab ? (cam ? guided_records_kernel<true, true> : guided_records_kernel<true, false>)
                         : (cam ? guided_records_kernel<false, true> : guided_records_kernel<false, false>);
    hipLaunchKernelGGL(records, dim3((kcap + 255) / 256, 2, B), dim3(256), 0, h->stream,
                       f.count, f.pt, f.img2_base, f.tab, kcap, (const double *)h->d_K, r.cam, d_R, d_t, d_status, gate_px,
                       h->gm.rec, h->gm.thr2);
}

// Guided matches of run r under the poses d_R / d_t (d_status: the run's own poses, pairs that are not OK are skipped; nullptr:
// every pair) into the gm.* buffers.  The election words of the HBM form are the crossCheck matcher's d_hm_*, scratch of one
// launch sequence there as here.
void rpe_launch_guided(rpe_handle *h, const RpeRun &r, const double *d_R, const double *d_t, const int *d_status, double gate_px, int max_distance)
{
    const int kcap = h->lay.kcap, B = r.pairs;
    launch_guided_records(h, r, d_R, d_t, d_status, gate_px);
    // the crossCheck matcher's plan with 2 KB of scanned records in the first LDS region; the row words are final: no raw_desc
    const RpeHammingPlan p = rpe_hamming_plan(kcap, B, RPE_GUIDED_LDS_UINT4);
    launch_hamming_plan(h, r, p, match_guided_mfma_kernel<true, true>, match_guided_mfma_kernel<true, false>,
                        match_guided_mfma_kernel<false, true>, match_guided_mfma_kernel<false, false>, (const uint8_t *)nullptr,
                        MatchBufs{h->gm.q, h->gm.t, h->gm.d, h->gm.n, h->gm.pts1, h->gm.pts2},
                        max_distance, p.region0, (const double4 *)h->gm.rec, (const double *)h->gm.thr2);
}

// ===================================================================== L2 (SIFT)
// cv2.BFMatcher(NORM_L2, crossCheck=True) on SIFT descriptors (pose_estimator.py:94,:127-131).
// SIFT descriptors are integer-valued 0..255 (saturate_cast<uchar> in calcSIFTDescriptor), so
// they are kept as u8[128] in HBM and the squared distance is EXACT in integers:
// |a-b|^2 = |a|^2 + |b|^2 - 2 a.b.  The reported / compared distance is the f32 sqrt of that integer, exactly what
// cv2 computes in f32 (sum < 2^24).  Keys are 64-bit because the sort key is the f32 distance (distinct integers
// can collide after sqrt -> tie broken by index).
//
// crossCheck, as batchDistance runs it (two passes): NNt(i) = the query's nearest train (lowest train on ties),
// NNq(j) = the train's nearest query (lowest query on ties); (i, NNt(i)) is a match iff NNq(NNt(i)) == i.  Both passes
// are the same "every OWNED descriptor finds its nearest SCANNED one" loop with the two images swapped; each writes
// one packed (f32 distance bits << 18 | scanned index) word per owned descriptor, the select kernel joins them.
//
// The O(N^2) part runs on the matrix cores (match_l2_mfma_kernel): with a' = a - 128 (a XOR 0x80 per byte: u8 -> i8),
// |a-b|^2 = |a'|^2 + |b'|^2 - 2 a'.b' and a'.b' is v_mfma_i32_32x32x32_i8 over K = 128 (4 MFMAs per 32 x 32 tile; exact
// integers).  The Lowe-ratio extension, which also needs the second-best distance, has a vector-ALU kernel of its own
// (match_l2_ratio_kernel: 32 x v_dot4_u32_u8 per distance); it serves that mode and nothing else.
#define L2_QTILE 256

// NQ = descriptor bytes / 16: 8 for SIFT (128 B), 2 for ORB descriptors matched with NORM_L2 (32 B; cv2 builds this
// combination too, pose_estimator.py:115-131 -- batchDistance on CV_8U rows gives sqrt((float)sum of squared byte
// differences), the same exact-integer form)
template <int NQ>
__device__ __forceinline__ unsigned dot_u8(const uint4 *q, const uint4 (&t)[NQ])
{
    unsigned acc = 0;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const uint4 a = q[k];
        acc = __builtin_amdgcn_udot4(a.x, t[k].x, acc, false);
        acc = __builtin_amdgcn_udot4(a.y, t[k].y, acc, false);
        acc = __builtin_amdgcn_udot4(a.z, t[k].z, acc, false);
        acc = __builtin_amdgcn_udot4(a.w, t[k].w, acc, false);
    }
    return acc;
}

// The Lowe-ratio L2 matcher, on the vector ALU.  Workgroup = (256 queries, pair), a lane owns one query descriptor; the
// train descriptors stream through LDS.  best[] gets a word only where the ratio test passed.
template <int NQ, bool TAB>
__global__ __launch_bounds__(256) void match_l2_ratio_kernel(const uint8_t *__restrict__ desc, const int *__restrict__ kp_count,
                                                              int img2_base, const int2 *__restrict__ pair_tab, int kcap, double ratio,
                                                              unsigned long long *__restrict__ best)
{
    constexpr int DIM = NQ * 16;
    __shared__ uint4 s_t[L2_QTILE * NQ];                                        // 32 KB (SIFT) / 8 KB (ORB)
    __shared__ unsigned s_tn[L2_QTILE];                                         // |t|^2 of the tile
    const int tid = threadIdx.x, pair = blockIdx.y, qc = blockIdx.x * 256;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int n1 = min(kp_count[img1], kcap), n2 = min(kp_count[img2], kcap);
    if (qc >= n1 || n2 <= 0) return;
    const uint4 *d1 = (const uint4 *)(desc + (long long)img1 * kcap * DIM);
    const uint4 *d2 = (const uint4 *)(desc + (long long)img2 * kcap * DIM);
    const int i = qc + tid;
    const bool valid = i < n1;
    uint4 q[NQ];
    unsigned qn = 0;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        q[k] = valid ? d1[NQ * i + k] : make_uint4(0, 0, 0, 0);
        qn = __builtin_amdgcn_udot4(q[k].x, q[k].x, qn, false); qn = __builtin_amdgcn_udot4(q[k].y, q[k].y, qn, false);
        qn = __builtin_amdgcn_udot4(q[k].z, q[k].z, qn, false); qn = __builtin_amdgcn_udot4(q[k].w, q[k].w, qn, false);
    }
    float bestd = __builtin_inff(), second = __builtin_inff();
    int bestj = -1;
    for (int tt = 0; tt < n2; tt += L2_QTILE) {
        const int nt = min(L2_QTILE, n2 - tt);
        __syncthreads();
        {
            uint4 stage[NQ];
#pragma unroll
            for (int c = 0; c < NQ; ++c) { const int idx = tid + 256 * c; stage[c] = idx < nt * NQ ? d2[NQ * tt + idx] : make_uint4(0, 0, 0, 0); }
#pragma unroll
            for (int c = 0; c < NQ; ++c) s_t[tid + 256 * c] = stage[c];
        }
        __syncthreads();
        if (tid < nt) {
            unsigned tn = 0;
            for (int k = 0; k < NQ; ++k) {
                const uint4 a = s_t[NQ * tid + k];
                tn = __builtin_amdgcn_udot4(a.x, a.x, tn, false); tn = __builtin_amdgcn_udot4(a.y, a.y, tn, false);
                tn = __builtin_amdgcn_udot4(a.z, a.z, tn, false); tn = __builtin_amdgcn_udot4(a.w, a.w, tn, false);
            }
            s_tn[tid] = tn;
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const unsigned ab = dot_u8<NQ>(s_t + NQ * j, q);
            const float d = sqrtf((float)(s_tn[j] + qn - 2u * ab));
            if (d < bestd) { second = bestd; bestd = d; bestj = tt + j; }
            else if (d < second) second = d;
        }
    }
    if (valid && n2 >= 2 && (double)bestd < ratio * (double)second)
        best[(long long)pair * kcap + i] = ((unsigned long long)__float_as_uint(bestd) << 18) | (unsigned long long)bestj;
}

// Per descriptor a (u = a - 128 per byte): { |u|^2, |u|^2 + 2 sum(u) } -- the owner's and the scanned row's terms of the MFMA kernel
template <int NQ>
__global__ __launch_bounds__(256) void match_l2_norms_kernel(const uint8_t *__restrict__ desc, const int *__restrict__ kp_count, int kcap,
                                                              int2 *__restrict__ norms)
{
    const int img = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= min(kp_count[img], kcap)) return;
    const uint4 *d = (const uint4 *)(desc + ((long long)img * kcap + k) * (NQ * 16));
    int acc = 0, sum = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint4 a = d[q];
        const int x = (int)(a.x ^ 0x80808080u), y = (int)(a.y ^ 0x80808080u), z = (int)(a.z ^ 0x80808080u), w = (int)(a.w ^ 0x80808080u);
        acc = __builtin_amdgcn_sdot4(x, x, acc, false); acc = __builtin_amdgcn_sdot4(y, y, acc, false);
        acc = __builtin_amdgcn_sdot4(z, z, acc, false); acc = __builtin_amdgcn_sdot4(w, w, acc, false);
        sum = __builtin_amdgcn_sdot4(x, 0x01010101, sum, false); sum = __builtin_amdgcn_sdot4(y, 0x01010101, sum, false);
        sum = __builtin_amdgcn_sdot4(z, 0x01010101, sum, false); sum = __builtin_amdgcn_sdot4(w, 0x01010101, sum, false);
    }
    norms[(long long)img * kcap + k] = make_int2(acc, acc + 2 * sum);
}

// Matrix-core form of one crossCheck pass.  Workgroup = 4 waves; wave w owns 32 descriptors (tile 4 blockIdx.x + w): the
// B operand (MFMA columns) of all KS K-steps, in registers.  The scanned descriptors stream through LDS as A-operand
// tiles of 32 rows (lane l of K-step s holds bytes [32 s + 16 (l >> 5), +16) of row l & 31: a plain 16-byte piece of
// the descriptor), double buffered, fetched PF tiles ahead.  blockIdx.y deals the scanned tiles over gridDim.y
// workgroups (small batches: one pair of 12 k x 12 k descriptors fills the chip), blockIdx.z = 2 pair + pass.
// The owner operand is the one's complement w = -v - 1 = b XOR 0x7F of v = b - 128 (its negative would not fit int8), so
// u.v = -u.w - sum(u) and |a-b|^2 = |v|^2 + e with e = (|u|^2 + 2 sum(u)) + 2 u.w: one v_lshl_add_u32 per accumulator,
// the row term comes from the norms kernel, the owner's |v|^2 is a per-lane constant and stays out of the comparison.  cv2 compares f32 distances: sqrtf is monotone, so a row can only win if its e is no larger than
// the running best's -- or larger by at most 2, when two integers share one f32 square root (only beyond 2^22) and the
// row has the lower index.  That test runs on the tile minimum; the exact (f32 distance, index) comparison of the
// 16 rows runs only in a wave where some lane passes it.
#define L2M_PF 3
template <int KS, bool TAB>
__global__ __launch_bounds__(256) void match_l2_mfma_kernel(const uint8_t *__restrict__ desc, const int2 *__restrict__ norms,
                                                             const int *__restrict__ kp_count, int img2_base, const int2 *__restrict__ pair_tab, int kcap,
                                                             unsigned long long *__restrict__ nn_t, unsigned long long *__restrict__ nn_q)
{
    constexpr int DIM = KS * 32;
    __shared__ v4i_t s_a[2][KS][64];
    __shared__ __attribute__((aligned(16))) int s_qn[2][32];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, col = lane & 31;
    const int pair = blockIdx.z >> 1, pass = blockIdx.z & 1;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int n1 = min(kp_count[img1], kcap), n2 = min(kp_count[img2], kcap);
    // pass 0: the queries own the columns and find their nearest train (NNt); pass 1: the trains find their nearest query
    const int img_own = pass ? img2 : img1, img_scan = pass ? img1 : img2;
    const int n_own = pass ? n2 : n1, n_scan = pass ? n1 : n2;
    if (blockIdx.x * 128 >= n_own || n_scan <= 0) return;
    const int ntq = (n_scan + 31) >> 5;
    const int per = (ntq + (int)gridDim.y - 1) / (int)gridDim.y;
    const int qt_lo = (int)blockIdx.y * per, qt_hi = min(ntq, qt_lo + per);
    if (qt_lo >= qt_hi) return;
    const uint4 *d_own = (const uint4 *)(desc + (long long)img_own * kcap * DIM);
    const uint4 *d_scan = (const uint4 *)(desc + (long long)img_scan * kcap * DIM);
    const int2 *nrm_scan = norms + (long long)img_scan * kcap;
    const int j = (blockIdx.x * 4 + wv) * 32 + col;
    const bool valid_own = j < n_own;
    v4i_t bop[KS];
#pragma unroll
    for (int sK = 0; sK < KS; ++sK) {
        uint4 t = make_uint4(0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu);
        if (valid_own) t = d_own[(long long)j * (DIM / 16) + 2 * sK + h];
        bop[sK].x = (int)(t.x ^ 0x7F7F7F7Fu); bop[sK].y = (int)(t.y ^ 0x7F7F7F7Fu); bop[sK].z = (int)(t.z ^ 0x7F7F7F7Fu); bop[sK].w = (int)(t.w ^ 0x7F7F7F7Fu);
    }
    const int tn = valid_own ? norms[(long long)img_own * kcap + j].x : 0;
    // loader: thread (s = tid >> 6, l = tid & 63) brings piece (row l & 31, bytes [32 s + 16 (l >> 5), +16)) of a tile
    const int xs = tid >> 6, xrow = lane & 31, xh = lane >> 5;
    const bool loader = xs < KS;
    auto fetch = [&](int qt) -> uint4 {
        const int q = qt * 32 + xrow;
        return (loader && qt < qt_hi && q < n_scan) ? d_scan[(long long)q * (DIM / 16) + 2 * xs + xh] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
    };
    auto fetch_n = [&](int qt) -> int {
        const int q = qt * 32 + tid;
        return (tid < 32 && qt < qt_hi && q < n_scan) ? nrm_scan[q].y : 0x3FFFFFFF;     // rows past the end never win
    };
    auto stage = [&](int buf, const uint4 &raw, int qn) {
        if (loader) {
            v4i_t v; v.x = (int)(raw.x ^ 0x80808080u); v.y = (int)(raw.y ^ 0x80808080u); v.z = (int)(raw.z ^ 0x80808080u); v.w = (int)(raw.w ^ 0x80808080u);
            s_a[buf][xs][lane] = v;
        }
        if (tid < 32) s_qn[buf][tid] = qn;
    };
    uint4 ring[L2M_PF]; int ring_n[L2M_PF];
#pragma unroll
    for (int u = 0; u < L2M_PF; ++u) { ring[u] = fetch(qt_lo + u); ring_n[u] = fetch_n(qt_lo + u); }
    stage(0, ring[0], ring_n[0]);
    ring[0] = fetch(qt_lo + L2M_PF); ring_n[0] = fetch_n(qt_lo + L2M_PF);
    __syncthreads();
    int best_e = 0x3FFFFFF0, best_idx = 0x7FFFFFFF;
    float best_g = __builtin_inff();
    for (int qt0 = qt_lo; qt0 < qt_hi; qt0 += L2M_PF) {
#pragma unroll
        for (int u = 0; u < L2M_PF; ++u) {
            const int qt = qt0 + u;
            if (qt < qt_hi) {                                  // workgroup-uniform
                const int buf = (qt - qt_lo) & 1;
                v16i_t acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int sK = 0; sK < KS; ++sK)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(s_a[buf][sK][lane], bop[sK], acc, 0, 0, 0);
                // C layout: column = lane & 31, row of register r = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                int e[16];
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const v4i_t qn4 = *(const v4i_t *)&s_qn[buf][8 * g4 + 4 * h];
                    e[4 * g4 + 0] = (acc[4 * g4 + 0] << 1) + qn4.x; e[4 * g4 + 1] = (acc[4 * g4 + 1] << 1) + qn4.y;
                    e[4 * g4 + 2] = (acc[4 * g4 + 2] << 1) + qn4.z; e[4 * g4 + 3] = (acc[4 * g4 + 3] << 1) + qn4.w;
                }
                int tmin = e[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) tmin = min(tmin, e[r]);
                if (__any(tmin <= best_e + 2)) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (e[r] <= best_e + 2) {
                            const float g = sqrtf((float)(e[r] + tn));
                            const int idx = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            if (g < best_g || (g == best_g && idx < best_idx)) { best_g = g; best_idx = idx; best_e = e[r]; }
                        }
                    }
                }
                if (qt + 1 < qt_hi) {
                    stage(buf ^ 1, ring[(u + 1) % L2M_PF], ring_n[(u + 1) % L2M_PF]);
                    ring[(u + 1) % L2M_PF] = fetch(qt + 1 + L2M_PF); ring_n[(u + 1) % L2M_PF] = fetch_n(qt + 1 + L2M_PF);
                }
                __syncthreads();
            }
        }
    }
    // the two half-waves hold the same columns (different rows)
    {
        const float og = __shfl_xor(best_g, 32); const int oi = __shfl_xor(best_idx, 32);
        if (og < best_g || (og == best_g && oi < best_idx)) { best_g = og; best_idx = oi; }
    }
    if (valid_own && h == 0 && best_idx != 0x7FFFFFFF) {
        unsigned long long *out = (pass ? nn_q : nn_t) + (long long)pair * kcap + j;
        atomicMin(out, ((unsigned long long)__float_as_uint(best_g) << 18) | (unsigned long long)best_idx);
    }
}

// The tile loop of match_l2_mfma_kernel (same grid, B operand, A tiles, ring and e = (acc << 1) + qn epilogue) with the gate of
// guided matching (include/rpe_amd.h, rpe_guided_matches_l2) in the exact branch: a kernel family of its own, as
// match_guided_mfma_kernel is beside the Hamming tile kernel.  The records are guided_records_kernel's.  The owner lane
// keeps its 32-byte record in registers; the 32 records of a scanned tile travel with the tile: 64 16-byte pieces fetched
// L2M_PF tiles ahead by wave 3, staged in 2 KB of LDS beside s_qn and read only by an entry that reaches the gate.  An
// entry reaches it when it passes e <= best_e + 2 and beats (best_g, best_idx) in the f32 (distance, index) order; best_e,
// best_g and best_idx move on admissible entries only, so the + 2 allowance is relative to the best admissible entry so
// far and the result is the minimum over the admissible entries whatever the order of the tiles.  Rows past the end carry
// NaN records and an e above every allowance; a lane without an owner starts from a best_e below every e and never enters
// the branch.  A pair whose thr2 is NaN is not matched.  max_distance is applied to the column's elected key: the
// nearest admissible neighbour is beyond it exactly when every admissible one is.
template <int KS, bool TAB>
__global__ __launch_bounds__(256) void match_l2_guided_mfma_kernel(const uint8_t *__restrict__ desc, const int2 *__restrict__ norms,
                                                                    const int *__restrict__ kp_count, int img2_base, const int2 *__restrict__ pair_tab, int kcap,
                                                                    const double4 *__restrict__ g_rec, const double *__restrict__ g_thr2, double max_distance,
                                                                    unsigned long long *__restrict__ nn_t, unsigned long long *__restrict__ nn_q)
{
    constexpr int DIM = KS * 32;
    __shared__ v4i_t s_a[2][KS][64];
    __shared__ __attribute__((aligned(16))) int s_qn[2][32];
    __shared__ double2 s_rec[2][64];                          // [buf][2 row + half]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, col = lane & 31;
    const int pair = blockIdx.z >> 1, pass = blockIdx.z & 1;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const double thr2 = g_thr2[pair];
    if (thr2 != thr2) return;                                  // NaN: the pair is not matched
    const int n1 = min(kp_count[img1], kcap), n2 = min(kp_count[img2], kcap);
    // pass 0: the queries own the columns and find their nearest admissible train (NNt); pass 1: the trains find their query
    const int img_own = pass ? img2 : img1, img_scan = pass ? img1 : img2;
    const int n_own = pass ? n2 : n1, n_scan = pass ? n1 : n2;
    if (blockIdx.x * 128 >= n_own || n_scan <= 0) return;
    const int ntq = (n_scan + 31) >> 5;
    const int per = (ntq + (int)gridDim.y - 1) / (int)gridDim.y;
    const int qt_lo = (int)blockIdx.y * per, qt_hi = min(ntq, qt_lo + per);
    if (qt_lo >= qt_hi) return;
    const uint4 *d_own = (const uint4 *)(desc + (long long)img_own * kcap * DIM);
    const uint4 *d_scan = (const uint4 *)(desc + (long long)img_scan * kcap * DIM);
    const int2 *nrm_scan = norms + (long long)img_scan * kcap;
    // records: side 0 the queries' (l_0, l_1, l_2, s1), side 1 the trains' (x2, y2, s2, 0)
    const double4 *rec_own = g_rec + ((long long)pair * RPE_GUIDED_SIDES + pass) * kcap;
    const double2 *rec_scan = (const double2 *)(g_rec + ((long long)pair * RPE_GUIDED_SIDES + (pass ^ 1)) * kcap);
    const int j = (blockIdx.x * 4 + wv) * 32 + col;
    const bool valid_own = j < n_own;
    v4i_t bop[KS];
#pragma unroll
    for (int sK = 0; sK < KS; ++sK) {
        uint4 t = make_uint4(0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu);
        if (valid_own) t = d_own[(long long)j * (DIM / 16) + 2 * sK + h];
        bop[sK].x = (int)(t.x ^ 0x7F7F7F7Fu); bop[sK].y = (int)(t.y ^ 0x7F7F7F7Fu); bop[sK].z = (int)(t.z ^ 0x7F7F7F7Fu); bop[sK].w = (int)(t.w ^ 0x7F7F7F7Fu);
    }
    const int tn = valid_own ? norms[(long long)img_own * kcap + j].x : 0;
    const double qnan = __builtin_nan("");
    const double4 own = valid_own ? rec_own[j] : make_double4(qnan, qnan, qnan, qnan);
    const int xs = tid >> 6, xrow = lane & 31, xh = lane >> 5;
    const bool loader = xs < KS;
    const bool rec_loader = wv == 3;                           // piece (row lane >> 1, half lane & 1) of a tile's 32 records
    auto fetch = [&](int qt) -> uint4 {
        const int q = qt * 32 + xrow;
        return (loader && qt < qt_hi && q < n_scan) ? d_scan[(long long)q * (DIM / 16) + 2 * xs + xh] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
    };
    auto fetch_n = [&](int qt) -> int {
        const int q = qt * 32 + tid;
        return (tid < 32 && qt < qt_hi && q < n_scan) ? nrm_scan[q].y : 0x3FFFFFFF;     // rows past the end never win
    };
    auto fetch_rec = [&](int qt) -> double2 {
        const int q = qt * 32 + (lane >> 1);
        return (rec_loader && qt < qt_hi && q < n_scan) ? rec_scan[(long long)q * 2 + (lane & 1)] : make_double2(qnan, qnan);
    };
    auto stage = [&](int buf, const uint4 &raw, int qn, const double2 &rr) {
        if (loader) {
            v4i_t v; v.x = (int)(raw.x ^ 0x80808080u); v.y = (int)(raw.y ^ 0x80808080u); v.z = (int)(raw.z ^ 0x80808080u); v.w = (int)(raw.w ^ 0x80808080u);
            s_a[buf][xs][lane] = v;
        }
        if (tid < 32) s_qn[buf][tid] = qn;
        if (rec_loader) s_rec[buf][lane] = rr;
    };
    uint4 ring[L2M_PF]; int ring_n[L2M_PF]; double2 ring_rec[L2M_PF];
#pragma unroll
    for (int u = 0; u < L2M_PF; ++u) { ring[u] = fetch(qt_lo + u); ring_n[u] = fetch_n(qt_lo + u); ring_rec[u] = fetch_rec(qt_lo + u); }
    stage(0, ring[0], ring_n[0], ring_rec[0]);
    ring[0] = fetch(qt_lo + L2M_PF); ring_n[0] = fetch_n(qt_lo + L2M_PF); ring_rec[0] = fetch_rec(qt_lo + L2M_PF);
    __syncthreads();
    int best_e = valid_own ? 0x3FFFFFF0 : -0x40000000, best_idx = 0x7FFFFFFF;
    float best_g = __builtin_inff();
    for (int qt0 = qt_lo; qt0 < qt_hi; qt0 += L2M_PF) {
#pragma unroll
        for (int u = 0; u < L2M_PF; ++u) {
            const int qt = qt0 + u;
            if (qt < qt_hi) {                                  // workgroup-uniform
                const int buf = (qt - qt_lo) & 1;
                v16i_t acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int sK = 0; sK < KS; ++sK)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(s_a[buf][sK][lane], bop[sK], acc, 0, 0, 0);
                // C layout: column = lane & 31, row of register r = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                int e[16];
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const v4i_t qn4 = *(const v4i_t *)&s_qn[buf][8 * g4 + 4 * h];
                    e[4 * g4 + 0] = (acc[4 * g4 + 0] << 1) + qn4.x; e[4 * g4 + 1] = (acc[4 * g4 + 1] << 1) + qn4.y;
                    e[4 * g4 + 2] = (acc[4 * g4 + 2] << 1) + qn4.z; e[4 * g4 + 3] = (acc[4 * g4 + 3] << 1) + qn4.w;
                }
                int tmin = e[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) tmin = min(tmin, e[r]);
                if (__any(tmin <= best_e + 2)) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (e[r] <= best_e + 2) {
                            const float g = sqrtf((float)(e[r] + tn));
                            const int row = (r & 3) + 8 * (r >> 2) + 4 * h, idx = qt * 32 + row;
                            if (g < best_g || (g == best_g && idx < best_idx)) {
                                const double2 ra = s_rec[buf][2 * row], rb = s_rec[buf][2 * row + 1];
                                // v from the query's line in both passes; s1 + s2 in that order
                                double v, ss;
                                if (pass == 0) { v = (own.x * ra.x + own.y * ra.y) + own.z; ss = own.w + rb.x; }
                                else           { v = (ra.x * own.x + ra.y * own.y) + rb.x; ss = rb.y + own.z; }
                                if (v * v <= thr2 * ss) { best_g = g; best_idx = idx; best_e = e[r]; }
                            }
                        }
                    }
                }
                if (qt + 1 < qt_hi) {
                    stage(buf ^ 1, ring[(u + 1) % L2M_PF], ring_n[(u + 1) % L2M_PF], ring_rec[(u + 1) % L2M_PF]);
                    ring[(u + 1) % L2M_PF] = fetch(qt + 1 + L2M_PF); ring_n[(u + 1) % L2M_PF] = fetch_n(qt + 1 + L2M_PF);
                    ring_rec[(u + 1) % L2M_PF] = fetch_rec(qt + 1 + L2M_PF);
                }
                __syncthreads();
            }
        }
    }
    // the two half-waves hold the same columns (different rows)
    {
        const float og = __shfl_xor(best_g, 32); const int oi = __shfl_xor(best_idx, 32);
        if (og < best_g || (og == best_g && oi < best_idx)) { best_g = og; best_idx = oi; }
    }
    // a column without an admissible entry within max_distance publishes nothing
    if (valid_own && h == 0 && best_idx != 0x7FFFFFFF && (double)best_g <= max_distance) {
        unsigned long long *out = (pass ? nn_q : nn_t) + (long long)pair * kcap + j;
        atomicMin(out, ((unsigned long long)__float_as_uint(best_g) << 18) | (unsigned long long)best_idx);
    }
}

// Kernel 2: workgroup = pair: stable sort of the (distance, queryIdx) keys of the surviving matches, first max_matches,
// point gather.  nn_t[i] = query i's nearest train; nn_q (crossCheck only, nullptr for the ratio mode) = train j's
// nearest query: the match survives iff nn_q[nn_t[i]] names i
template <bool TAB>
__global__ __launch_bounds__(256) void match_l2_select_kernel(const unsigned long long *__restrict__ nn_t, const unsigned long long *__restrict__ nn_q,
                                                               const int *__restrict__ kp_count,
                                                               const float2 *__restrict__ kp_pt, int img2_base, const int2 *__restrict__ pair_tab, int kcap, int max_matches,
                                                               int *__restrict__ m_q, int *__restrict__ m_t, float *__restrict__ m_d,
                                                               int *__restrict__ m_n, float2 *__restrict__ pts1, float2 *__restrict__ pts2)
{
    extern __shared__ unsigned long long s_key[];          // sortP <= 16384 keys (128 KB)
    const int pair = blockIdx.x;
    int img1, img2;
    rpe_pair_slots<TAB>(pair_tab, img2_base, pair, img1, img2);
    const int n1 = min(kp_count[img1], kcap);
    const unsigned long long *bp = nn_t + (long long)pair * kcap;
    const unsigned long long *nq = nn_q ? nn_q + (long long)pair * kcap : nullptr;
    const MatchOut<float> out(pair, max_matches, img1, img2, kcap, kp_pt, m_q, m_t, m_d, pts1, pts2);
    select_sort_emit<256>(s_key, n1, max_matches, m_n + pair,
        [&](int i) {
            const unsigned long long b = bp[i];
            return b != ~0ull && (!nq || (int)(nq[b & 0x3FFFF] & 0x3FFFF) == i) ? ((b >> 18) << 16) | (unsigned long long)i : ~0ull;
        },
        [&](int r, int i, unsigned long long key) { out.put(r, i, (int)(bp[i] & 0x3FFFF), __uint_as_float((unsigned)(key >> 16))); });
}

// match_l2_select_kernel's dynamic LDS: one 64-bit key per element of the sort size, the power of two >= max(kcap, 64).
// More than 8128 keypoints per image pass the default; the most is uncapped SIFT's 16384 keys, 128 KB of the CU's 160
constexpr size_t l2_select_lds_bytes(int kcap)
{
    int sortP = 64;
    while (sortP < kcap) sortP <<= 1;
    return sizeof(unsigned long long) * (size_t)sortP;
}
static_assert(l2_select_lds_bytes(RPE_MAX_KCAP) <= RPE_CU_LDS_BYTES, "the largest handle's sort keys fit a CU's LDS");

// The launch of match_l2_select_kernel over the words in d_m_best2 (and nn_q, see there) into the lists o (o.d holds f32)
static void launch_l2_select(rpe_handle *h, const RpeRun &r, const unsigned long long *nn_q, const MatchBufs &o)
{
    const int kcap = h->lay.kcap;
    const RpeFeatSrc &f = r.feat;
    launch_tab(f.tab, match_l2_select_kernel<true>, match_l2_select_kernel<false>, dim3(r.pairs), dim3(256), l2_select_lds_bytes(kcap), h->stream,
                       (const unsigned long long *)h->d_m_best2, nn_q, f.count, f.pt, f.img2_base, f.tab, kcap, h->cfg.max_matches,
                       o.q, o.t, (float *)o.d, o.n, o.p1, o.p2);
}

// The kernels of this file that launch above the default dynamic LDS.  The Hamming matchers serve ORB handles only
// (kcap <= RPE_ORB_MAX_FEATURES + 64 = 8064) and stay at or below it: the fused tile kernel by rpe_hamming_plan's rule, the
// HBM form's tile and select kernels with 35 KB and 32 KB, the ratio kernel with QTILE * 32 + kcap * 4 = 63.5 KB.
std::vector<RpeLdsCeiling> rpe_match_lds_ceilings()
{
    constexpr size_t kcap = RPE_ORB_MAX_FEATURES + 64;
    static_assert((size_t)QTILE * 32 + kcap * 4 <= RPE_LDS_DEFAULT_BYTES, "the ratio kernel needs no raised limit");
    static_assert((MM_STAGE + RPE_GUIDED_LDS_UINT4) * 16 + kcap * 2 + 15 <= RPE_LDS_DEFAULT_BYTES && l2_select_lds_bytes(kcap) / 2 <= RPE_LDS_DEFAULT_BYTES,
                  "region0 of the HBM form (staging + scanned words, or the 4-byte sort keys) and the select kernel's keys need none");
    return {{(const void *)match_l2_select_kernel<true>, "match_l2_select_kernel<true>", l2_select_lds_bytes(RPE_MAX_KCAP)},
            {(const void *)match_l2_select_kernel<false>, "match_l2_select_kernel<false>", l2_select_lds_bytes(RPE_MAX_KCAP)}};
}

// The split of the matrix-core L2 tile kernels for B pairs: owner chunks of 128, the scanned tiles dealt over gridDim.y
// workgroups until ~1024 workgroups are in flight (a single pair included), blockIdx.z = 2 pair + pass
static dim3 l2_mfma_grid(int kcap, int B)
{
    const int chunks = (kcap + 127) / 128;
    int split = (1024 + chunks * 2 * B - 1) / (chunks * 2 * B);
    split = split < 1 ? 1 : split > 8 ? 8 : split;
    return dim3(chunks, split, 2 * B);
}

// { |u|^2, |u|^2 + 2 sum(u) } of the descriptors of workspace images [0, n_img): once per batch / stream, and once per
// rpe_frames_put* (the frame store keeps the words next to the descriptors; a pair list never recomputes them)
void rpe_launch_l2_norms(rpe_handle *h, int n_img)
{
    const int kcap = h->lay.kcap;
    const dim3 gn((kcap + 255) / 256, n_img);
    if (h->desc_bytes == 128) hipLaunchKernelGGL(match_l2_norms_kernel<8>, gn, dim3(256), 0, h->stream, h->d_desc, h->d_kp_count, kcap, (int2 *)h->d_m_norm);
    else                      hipLaunchKernelGGL(match_l2_norms_kernel<2>, gn, dim3(256), 0, h->stream, h->d_desc, h->d_kp_count, kcap, (int2 *)h->d_m_norm);
}

void rpe_launch_match_l2(rpe_handle *h, const RpeRun &r)
{
    const int kcap = h->lay.kcap, B = r.pairs;
    const RpeFeatSrc &f = r.feat;                             // the workspace (batch / stream rule) or the frame store (pair table)
    const int img2_base = f.img2_base;
    // d_m_best2 = NNt (per query; the ratio mode's only list), d_m_best = NNq (per train)
    hipMemsetAsync(h->d_m_best2, 0xFF, sizeof(unsigned long long) * (size_t)B * kcap, h->stream);
    const bool rt = h->cfg.match_mode == RPE_MATCH_RATIO;
    if (!rt) hipMemsetAsync(h->d_m_best, 0xFF, sizeof(unsigned long long) * (size_t)B * kcap, h->stream);
    const bool sift = h->desc_bytes == 128;
    if (rt) {
        const dim3 grid((kcap + 255) / 256, B);
        if (sift) launch_tab(f.tab, match_l2_ratio_kernel<8, true>, match_l2_ratio_kernel<8, false>, grid, dim3(256), 0, h->stream, f.desc, f.count, img2_base, f.tab, kcap, h->cfg.match_ratio, h->d_m_best2);
        else      launch_tab(f.tab, match_l2_ratio_kernel<2, true>, match_l2_ratio_kernel<2, false>, grid, dim3(256), 0, h->stream, f.desc, f.count, img2_base, f.tab, kcap, h->cfg.match_ratio, h->d_m_best2);
    } else {
        // images [0, B) and [img2_base, img2_base + B) (a stream: B + 1 frames); the frame store holds its slots' words already
        if (!f.tab) rpe_launch_l2_norms(h, img2_base + B);
        const dim3 grid = l2_mfma_grid(kcap, B);
        if (sift) launch_tab(f.tab, match_l2_mfma_kernel<4, true>, match_l2_mfma_kernel<4, false>, grid, dim3(256), 0, h->stream, f.desc, f.norm, f.count, img2_base, f.tab, kcap, h->d_m_best2, h->d_m_best);
        else      launch_tab(f.tab, match_l2_mfma_kernel<1, true>, match_l2_mfma_kernel<1, false>, grid, dim3(256), 0, h->stream, f.desc, f.norm, f.count, img2_base, f.tab, kcap, h->d_m_best2, h->d_m_best);
    }
    launch_l2_select(h, r, rt ? (const unsigned long long *)nullptr : (const unsigned long long *)h->d_m_best,
                     MatchBufs{h->d_m_q, h->d_m_t, h->d_m_d, h->d_m_n, h->d_pts1, h->d_pts2});
}

// Guided matches of run r for an L2 handle, into the gm.* buffers (gm.d read as f32); poses and d_status as in
// rpe_launch_guided.  Served for both match modes: the guided rule is the mutual one, and the matrix-core form needs the norm
// words, which a ratio-mode run of the workspace never wrote (the kernel is idempotent and O(N); the frame
// store of every NORM_L2 handle, ratio mode included, holds its slots' words from the put).  d_m_best2 / d_m_best are scratch of one matcher launch sequence -- nothing reads
// them after rpe_launch_match_l2's select -- and serve as the guided NNt / NNq words here.
void rpe_launch_guided_l2(rpe_handle *h, const RpeRun &r, const double *d_R, const double *d_t, const int *d_status, double gate_px, double max_distance)
{
    const int kcap = h->lay.kcap, B = r.pairs;
    const RpeFeatSrc &f = r.feat;
    launch_guided_records(h, r, d_R, d_t, d_status, gate_px);
    if (!f.tab) rpe_launch_l2_norms(h, f.img2_base + B);
    hipMemsetAsync(h->d_m_best2, 0xFF, sizeof(unsigned long long) * (size_t)B * kcap, h->stream);
    hipMemsetAsync(h->d_m_best, 0xFF, sizeof(unsigned long long) * (size_t)B * kcap, h->stream);
    const dim3 grid = l2_mfma_grid(kcap, B);
    if (h->desc_bytes == 128)
        launch_tab(f.tab, match_l2_guided_mfma_kernel<4, true>, match_l2_guided_mfma_kernel<4, false>, grid, dim3(256), 0, h->stream,
                   f.desc, f.norm, f.count, f.img2_base, f.tab, kcap, (const double4 *)h->gm.rec, (const double *)h->gm.thr2, max_distance, h->d_m_best2, h->d_m_best);
    else
        launch_tab(f.tab, match_l2_guided_mfma_kernel<1, true>, match_l2_guided_mfma_kernel<1, false>, grid, dim3(256), 0, h->stream,
                   f.desc, f.norm, f.count, f.img2_base, f.tab, kcap, (const double4 *)h->gm.rec, (const double *)h->gm.thr2, max_distance, h->d_m_best2, h->d_m_best);
    launch_l2_select(h, r, (const unsigned long long *)h->d_m_best, MatchBufs{h->gm.q, h->gm.t, h->gm.d, h->gm.n, h->gm.pts1, h->gm.pts2});
}
