// similar_kernels.hip -- pair proposals (rpe_frames_similar / rpe_similarity_hamming; NOT in the reference): an exact
// similarity score between frames and a top-k candidate selection.
//
// The score of (query frame, target frame) is the NUMBER of crossCheck matches between their sampled descriptors whose
// distance is <= max_distance (the definition: include/rpe_amd.h, "pair proposals").  That is the main loop of
// match_hamming_mfma_kernel and a count: no sort, no point gather.  similar_hamming_kernel keeps that loop -- the target's
// sampled descriptors are the MFMA B operands, 32 per wave in 32 VGPRs, the query's tiles stream through the double-buffered
// LDS stage, v_mfma_i32_32x32x32_i8 on 0/1 bytes, the column minima in a register, the row minima through row_min32 and an
// LDS atomicMin -- and differs around it:
//   * a workgroup serves one target and a CHUNK of query positions, one after the other.  A target sample of 8 tiles or
//     fewer (M <= 256) is loaded and expanded once and its owner registers are kept over the whole chunk: with a stride
//     the samples are small, and the owner load would otherwise be a large part of a pair;
//   * the stride is address arithmetic on the loads (sample k is descriptor k * step): no packing pass;
//   * the epilogue of a pair converts the row keys, counts the queries whose election word equals their row word within
//     max_distance (ballot + popcount, one LDS add per wave) and writes one int.  The election words are set again for
//     every pair;
//   * identical lists (the host compares them) run the triangle r <= c and write scores[r][c] and scores[c][r]: the
//     mutual set of (a, b) is the transpose of that of (b, a).
// similar_select_kernel picks the candidates of a query row: k rounds of a maximum over (score, ~column) keys among the
// eligible columns, each round below the key of the round before.  Plain vector code: nt words per round from L2.
#include "rpe_internal.h"
#include "hamming_tiles.h"

// LDS of similar_hamming_kernel for samples of up to mcap descriptors: the staging, then per sampled query its election word,
// its own-nearest word and |q| + 512
static constexpr size_t similar_lds_bytes(int mcap) { return (size_t)MM_STAGE * 16 + (size_t)mcap * 10 + 16; }
static_assert(similar_lds_bytes(RPE_ORB_MAX_FEATURES + 64) <= RPE_CU_LDS_BYTES, "an ORB handle's full sample fits one workgroup's LDS");

__global__ __launch_bounds__(MM_NT, 4) void similar_hamming_kernel(const uint8_t *__restrict__ desc, const int *__restrict__ kp_count, int kcap,
                                                                 const int *__restrict__ q_slots, const int *__restrict__ t_slots, int nq, int nt,
                                                                 int chunk, int same, int step, int max_distance, int mcap,
                                                                 int *__restrict__ scores)
{
    extern __shared__ uint4 s_dyn[];
    __shared__ int s_cnt;
    v4i_t *s_a = (v4i_t *)s_dyn;                               // [2][8][64]
    unsigned *s_qpk = (unsigned *)(s_dyn + 2 * 8 * 64);        // [2][32]
    unsigned *s_best = (unsigned *)(s_dyn + MM_STAGE);         // mcap election words (dist << 18 | target sample index)
    unsigned *s_row = s_best + mcap;                           // mcap own-nearest words, as the raw row key
    unsigned short *s_qpop = (unsigned short *)(s_row + mcap); // mcap: |q| + 512
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // workgroup = (target position c, chunk of query positions [r0, r_end)); the triangle of identical lists ends at r = c
    const int c = (int)(blockIdx.x % (unsigned)nt), r0 = (int)(blockIdx.x / (unsigned)nt) * chunk;
    const int r_end = min(r0 + chunk, same ? c + 1 : nq);
    if (r0 >= r_end) return;
    const int h = lane >> 5, col = lane & 31;
    const int xs = tid >> 6, xl = tid & 63, xrow = xl & 31, xh = xl >> 5;
    const bool c3 = (lane & 8) != 0, c2 = (lane & 4) != 0, c1 = (lane & 2) != 0;
    const int rrow = ((col >> 1) & 3) + 8 * (col >> 3) + 4 * h;      // the row whose minimum row_min32 leaves in this lane
    // the target: the owner of the MFMA columns.  Sample index j is its descriptor j * step
    const int t_slot = t_slots[c];
    const int m_own = (min(kp_count[t_slot], kcap) + step - 1) / step, ntt = (m_own + 31) >> 5;
    const uint4 *d2 = (const uint4 *)(desc + (long long)t_slot * kcap * 32);
    // What a lane keeps of its owner: the B operands and the row key of its column, (|t| + 512) << 16 | j (see
    // match_hamming_mfma_kernel); columns past the end: a key no real distance can beat.  The rest is derived again where it
    // is needed, once per round: the registers are what decides the workgroups per CU
    v4i_t bop[8];
    unsigned tpk = 0;
    auto own = [&](int tt0) {
        const int j = (tt0 + wv) * 32 + col;
        const bool valid_t = j < m_own;
        const int tpop = load_owner(bop, d2, j * step, valid_t, h);
        tpk = ((valid_t ? (unsigned)tpop + 512u : 0x7000u) << 16) | (unsigned)j;
    };
    const bool keep = ntt <= 8;                                // one round: the owner registers serve every query of the chunk
    if (keep) own(0);
    for (int r = r0; r < r_end; ++r) {
        const int q_slot = q_slots[r];
        const int m_scan = (min(kp_count[q_slot], kcap) + step - 1) / step, ntq = (m_scan + 31) >> 5;
        const unsigned *q32 = (const unsigned *)(desc + (long long)q_slot * kcap * 32);      // scanned: 8 dwords per descriptor
        // (the pair before is behind the barrier in front of its score: nothing of it reads the words set here)
        for (int i = tid; i < m_scan; i += MM_NT) {
            const uint4 *d = (const uint4 *)q32 + 2 * (long long)(i * step);
            s_best[i] = 0xFFFFFFFFu; s_row[i] = 0xFFFFFFFEu;
            s_qpop[i] = (unsigned short)(512u + popc256(d[0], d[1]));
        }
        if (tid == 0) s_cnt = 0;
        for (int tt0 = 0; tt0 < ntt && m_scan > 0; tt0 += 8) {
            if (!keep) own(tt0);
            const int tt = tt0 + wv;
            unsigned best_key = 0xFFFFFFFFu;
            unsigned ring[MM_PF];
            auto fetch = [&](int qt) -> unsigned {
                const int q = qt * 32 + xrow;
                return q < m_scan ? q32[(long long)(q * step) * 8 + xs] : 0u;
            };
            auto stage = [&](int qt, int buf, unsigned raw) {
                s_a[(buf * 8 + xs) * 64 + xl] = expand16((raw >> (16 * xh)) & 0xFFFFu);
                if (tid < 32) {
                    const int qq = qt * 32 + tid;
                    const unsigned pk = qq < m_scan ? (unsigned)s_qpop[qq] : 0x7000u;      // rows past the end: a key no real distance can beat
                    s_qpk[buf * 32 + tid] = (pk << 16) | (unsigned)qq;
                }
            };
            __syncthreads();                                   // the round before has finished reading both buffers (and the words and s_qpop are set)
#pragma unroll
            for (int u = 0; u < MM_PF; ++u) ring[u] = fetch(u);
            stage(0, 0, ring[0]);
            ring[0] = fetch(MM_PF);
            __syncthreads();
            for (int qt0 = 0; qt0 < ntq; qt0 += MM_PF) {
#pragma unroll
                for (int u = 0; u < MM_PF; ++u) {
                    const int qt = qt0 + u;
                    if (qt < ntq) {                            // workgroup-uniform
                        const int buf = qt & 1;
                        if (tt < ntt) {
                            v16i_t acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                            for (int sK = 0; sK < 8; ++sK)
                                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(s_a[(buf * 8 + sK) * 64 + lane], bop[sK], acc, 0, 0, 0);
                            unsigned rk[16];
#pragma unroll
                            for (int rr = 0; rr < 16; ++rr) {
                                const unsigned qpk = s_qpk[buf * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * h];
                                const unsigned prod = (unsigned)__mul24(acc[rr], -131072);
                                best_key = min(best_key, prod + qpk);                               // (|q| + 512 - 2 q.t) << 16 | query sample index
                                rk[rr] = prod + tpk;
                            }
                            const unsigned rmin = row_min32(rk, c3, c2, c1);
                            const int q = qt * 32 + rrow;
                            if (!(col & 1) && q < m_scan) atomicMin(&s_row[q], rmin);              // rows past the end write nothing
                        }
                        if (qt + 1 < ntq) {
                            stage(qt + 1, buf ^ 1, ring[(u + 1) % MM_PF]);
                            ring[(u + 1) % MM_PF] = fetch(qt + 1 + MM_PF);
                        }
                        __syncthreads();
                    }
                }
            }
            best_key = min(best_key, (unsigned)__shfl_xor((int)best_key, 32));
            if ((int)(tpk & 0xFFFFu) < m_own && h == 0) {      // the lane has an owner
                const unsigned d = (best_key >> 16) - 1024u + (tpk >> 16), i = best_key & 0xFFFFu;      // |q| + 512 - 2 q.t, then - 512 + |t|
                atomicMin(&s_best[i], (d << 18) | (tpk & 0xFFFFu));             // target sample j elects query sample i
            }
        }
        __syncthreads();
        // a query counts when the target it is nearest to elected it: its row key, in the election words' format, equals its
        // election word (0xFFFFFFFF: nobody elected it), and the distance is within the bound
        int cnt = 0;
        for (int i0 = 0; i0 < m_scan; i0 += MM_NT) {           // wave-uniform trip count: the ballot sees all 64 lanes
            const int i = i0 + tid;
            bool hit = false;
            if (i < m_scan) {
                const unsigned b = s_best[i], k = s_row[i];
                const unsigned row = (((k >> 16) - 1024u + (unsigned)s_qpop[i]) << 18) | (k & 0xFFFFu);
                hit = b != 0xFFFFFFFFu && b == row && (int)(b >> 18) <= max_distance;
            }
            cnt += __popcll(__ballot(hit));
        }
        if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) {
            const int s = s_cnt;
            scores[(long long)r * nt + c] = s;
            if (same && r != c) scores[(long long)c * nt + r] = s;
        }
    }
}

// One workgroup per query row r.  Round m takes the largest key (score + 1) << 32 | ~column among the eligible columns whose
// key is below round m - 1's winner: score descending, column position ascending, every column once.  0 = no column left.
__global__ __launch_bounds__(256) void similar_select_kernel(const int *__restrict__ scores, int nt, const int *__restrict__ q_slots,
                                                              const int *__restrict__ t_slots, const int *__restrict__ q_time,
                                                              const int *__restrict__ t_time, int exclude, int min_score, int k,
                                                              int *__restrict__ cand, int *__restrict__ cand_score, int *__restrict__ n_cand)
{
    __shared__ unsigned long long s_w[4];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int *row = scores + (long long)r * nt;
    const int q_slot = q_slots[r];
    const long long qt = q_time[r];
    unsigned long long below = ~0ull;
    int n = 0;
    for (int m = 0; m < k; ++m) {
        unsigned long long best = 0;
        for (int c = tid; c < nt; c += 256) {
            const int s = row[c];
            const long long dt = qt - (long long)t_time[c];
            const bool ok = t_slots[c] != q_slot && (exclude < 0 || (dt < 0 ? -dt : dt) > (long long)exclude) && s >= min_score;
            const unsigned long long key = ((unsigned long long)(unsigned)(s + 1) << 32) | (unsigned)~c;
            if (ok && key < below && key > best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if ((tid & 63) == 0) s_w[tid >> 6] = best;
        __syncthreads();
        best = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
        __syncthreads();                                       // read before the next round writes
        if (best == 0) break;                                  // workgroup-uniform
        if (tid == 0) { cand[(long long)r * k + m] = (int)~(unsigned)best; cand_score[(long long)r * k + m] = (int)(best >> 32) - 1; }
        below = best;
        ++n;
    }
    if (tid == 0) {
        for (int m = n; m < k; ++m) { cand[(long long)r * k + m] = -1; cand_score[(long long)r * k + m] = -1; }
        n_cand[r] = n;
    }
}

// Query positions per workgroup.  A workgroup's pairs run one after the other, so the chunk stays small: one pair while
// the pairs do not fill the chip four workgroups per CU, then up to 4 (the last workgroups of a launch then last 4 pairs,
// not more, and a kept owner is loaded a quarter as often)
static int similar_chunk(long long pairs) { return (int)std::min<long long>(4, std::max<long long>(1, (pairs + 1023) / 1024)); }

void rpe_launch_similar(rpe_handle *h, const RpeSimilarJob &job)
{
    const int kcap = h->lay.kcap, mcap = (kcap + job.step - 1) / job.step;
    const long long pairs = job.same ? (long long)job.nq * (job.nq + 1) / 2 : (long long)job.nq * job.nt;
    const int chunk = similar_chunk(pairs);
    const long long groups = (long long)job.nt * ((job.nq + chunk - 1) / chunk);
    hipLaunchKernelGGL(similar_hamming_kernel, dim3((unsigned)groups), dim3(MM_NT), similar_lds_bytes(mcap), h->stream,
                       job.desc, job.count, kcap, job.q, job.t, job.nq, job.nt, chunk, job.same ? 1 : 0, job.step, job.max_distance, mcap,
                       job.scores);
    if (job.cand)
        hipLaunchKernelGGL(similar_select_kernel, dim3(job.nq), dim3(256), 0, h->stream,
                           (const int *)job.scores, job.nt, job.q, job.t, job.q_time, job.t_time, job.exclude, job.min_score, job.k,
                           job.cand, job.cand_score, job.n_cand);
}

// similar_hamming_kernel launches above the default dynamic LDS when an ORB handle's full sample (step 1) is larger than
// 4800 descriptors; its ceiling is the largest ORB capacity's
std::vector<RpeLdsCeiling> rpe_similar_lds_ceilings()
{
    return {{(const void *)similar_hamming_kernel, "similar_hamming_kernel", similar_lds_bytes(RPE_ORB_MAX_FEATURES + 64)}};
}
