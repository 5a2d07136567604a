// hamming_tiles.h -- the tile helpers of the matrix-core Hamming kernels, shared by match_kernels.hip (crossCheck and
// guided matchers) and similar_kernels.hip (frame similarity): the staging layout, the bit -> byte expansion, the owner
// operand, the scanned popcounts and the row election.  The kernels keep their own tile loops (the lesson at
// rpe_pair_slots); what the pieces are for is told at match_hamming_mfma_kernel.
#pragma once
#include "rpe_internal.h"

__device__ __forceinline__ unsigned popc256(const uint4 &a, const uint4 &b)
{
    return __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
}

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));
#define MM_NT 512
#define MM_PF 4                      // query tiles fetched ahead of the one being multiplied
#define MM_STAGE (2 * 8 * 64 + 16)   // uint4 at the head of LDS: two expanded scanned tiles [2][8][64] + their packed words [2][32]

__device__ __forceinline__ v4i_t expand16(unsigned b)
{
    v4i_t r;
    r.x = (int)(__umul24(b & 15u, 0x00204081u) & 0x01010101u);
    r.y = (int)(__umul24((b >> 4) & 15u, 0x00204081u) & 0x01010101u);
    r.z = (int)(__umul24((b >> 8) & 15u, 0x00204081u) & 0x01010101u);
    r.w = (int)(__umul24((b >> 12) & 15u, 0x00204081u) & 0x01010101u);
    return r;
}

// |q| + 512 of the n scanned descriptors d, for the packed (|q| + 512, index) words of the staged tiles
__device__ __forceinline__ void fill_qpop(unsigned short *s_qpop, const uint4 *d, int n)
{
    for (int i = threadIdx.x; i < n; i += MM_NT) s_qpop[i] = (unsigned short)(512u + popc256(d[2 * i], d[2 * i + 1]));
}

// B operand of the 8 K-steps: the lane's own descriptor j (zeros without one), bits [32 s + 16 h, +16) of step s; returns |t|
__device__ __forceinline__ int load_owner(v4i_t (&bop)[8], const uint4 *d, int j, bool valid, int h)
{
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0;
    if (valid) { t0 = d[2 * j]; t1 = d[2 * j + 1]; }
    const unsigned tw[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    int tpop = 0;
#pragma unroll
    for (int sK = 0; sK < 8; ++sK) { bop[sK] = expand16((tw[sK] >> (16 * h)) & 0xFFFFu); tpop += __popc(tw[sK]); }
    return tpop;
}

// Row election of one accumulator tile.  k[r] is this lane's key of row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) at column
// lane & 31; the result is the minimum over the 32 columns of row r = (lane & 31) >> 1 (both lanes of a pair hold it).
// A transpose reduction: at each step a lane pair trades half of its live registers and keeps the minima of the other
// half -- the lane whose column bit is set keeps the upper half -- so 16 registers become 8, 4, 2, 1 and the last step
// joins the two lanes of a pair.  Column bit 4 goes through v_permlane16_swap (one swap leaves both operands' partners in
// place: min of the pair), bits 3..0 through DPP row_ror:8, row_half_mirror, quad_perm [2,3,0,1] and [1,0,3,2]; every
// partner differs in the step's bit and agrees in the bits of the steps before it, and the five masks 16, 8, 7, 2, 1
// span the 32 columns.  8 + 8 + 3 (4 + 2 + 1) + 2 = 39 vector instructions, against 80 for five full rounds.
#define MM_DPP_ROR8 0x128
#define MM_DPP_HALF_MIRROR 0x141
#define MM_DPP_XOR2 0x4E
#define MM_DPP_XOR1 0xB1
template <int CTRL>
__device__ __forceinline__ unsigned min_dpp(unsigned x)
{
    return min(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, true));
}

__device__ __forceinline__ unsigned row_min32(unsigned (&k)[16], bool c3, bool c2, bool c1)
{
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const auto sw = __builtin_amdgcn_permlane16_swap(k[r], k[r + 8], false, false);
        k[r] = min((unsigned)sw[0], (unsigned)sw[1]);          // register r + 8 (column bit 4)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { const unsigned a = min_dpp<MM_DPP_ROR8>(k[r]), b = min_dpp<MM_DPP_ROR8>(k[r + 4]); k[r] = c3 ? b : a; }
#pragma unroll
    for (int r = 0; r < 2; ++r) { const unsigned a = min_dpp<MM_DPP_HALF_MIRROR>(k[r]), b = min_dpp<MM_DPP_HALF_MIRROR>(k[r + 2]); k[r] = c2 ? b : a; }
    const unsigned a = min_dpp<MM_DPP_XOR2>(k[0]), b = min_dpp<MM_DPP_XOR2>(k[1]);
    return min_dpp<MM_DPP_XOR1>(c1 ? b : a);
}
