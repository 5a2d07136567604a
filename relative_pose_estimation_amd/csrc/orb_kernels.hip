// orb_kernels.hip -- ORB detectAndCompute as hand-written gfx950 kernels.
//
// Replaces cv2.ORB_create(nfeatures, 1.1, 12, fastThreshold=15, HARRIS_SCORE)
// .detectAndCompute(image, None)  (reference src/core/pose_estimator.py:85-91,:108).
// Kernels (all images of the batch per launch; the stage names are the hipEvent slots of rpe_get_stage_ms):
//   pyramid  : pyr_resize x11: INTER_LINEAR_EXACT chain, 8.8 fixed point, 256x16 tiles of one wave, source window in LDS
//   fast     : fast_nms: FAST-9/16 score + 3x3 NMS + 31-px border filter, fused, 64x64 tiles, per-tile keypoint lists;
//              tiles cover the border-filtered region only ("nms" slot is empty)
//   select   : raster_corners (a level's tile lists -> one list in FAST's raster emission order) + retain_fast:
//              retainBest(2*quota) on the FAST score, replayed as the C++ runtime's nth_element + partition (cv2's ORDER)
//   harris   : 7x7 Harris response per candidate (f32, op order = oracle)
//   keypoints: retain_harris: retainBest(quota) on the Harris response, same replay; compact_keypoints: level-major lists
//   angle    : orient_describe: one keypoint per one-wave workgroup: patch in LDS -> intensity-centroid angle (fastAtan2) ->
//              Gaussian 7x7 on the patch (cv2's sepFilter2D f32 route, fused multiply-adds) -> 256-bit steered BRIEF
//              ("blur" / "describe" slots are empty; the whole-level blur kernel at the end only serves rpe_orb_debug_fetch)
// There is one configuration: the tile shapes are constants (rpe_internal.h for those the host tables share, here for the
// rest) and the static_asserts beside them hold the relations the kernels rely on.
// Everything is integer or mirrored-order f32, so results equal the CPU oracle bit for bit -- and, on the reference's own
// image pairs, cv2's (tests/test_reference_rows_cpu.py, tests/test_gpu_round3.py).
#include "rpe_internal.h"
#include "rpe_devmath.h"
#include "retain_best_emul.h"
#include "fast_entry.h"

__device__ float4 c_pattern_f[256];         // rBRIEF pattern (brief_pattern.inc) as f32 (x0, y0, x1, y1), uploaded at handle creation

// the radius-15 intensity-centroid disc as packed-u8 dot-product weights: item (row v = -15..15, dword j = 0..7) covers
// u = -16 + 4j .. +3; .x = 1 per in-disc byte, .y = (u + 16) per in-disc byte (0 elsewhere).  A 32nd row of zeros lets
// orient_describe_kernel run its four rounds of 64 items without a bound on the last one.
__constant__ uint2 c_discw[32 * 8];

// taps of the descriptor blur: GaussianBlur(7x7, sigma 2) as cv2's sepFilter2D f32 route holds them -- (float)(exp(-x^2 / 8) / sum),
// getGaussianKernel's normalised f64 kernel cast to f32 (computed on the host at handle creation, like the oracle does)
__constant__ float c_gauss[7];

// the kernels' constant tables: disc weights (from the n (u, v) offsets of the disc), rBRIEF pattern, blur taps
void rpe_orb_upload_constants(const signed char *disc, int n)
{
    uint2 wt[32 * 8];
    for (int i = 0; i < 32 * 8; ++i) wt[i] = make_uint2(0u, 0u);
    for (int i = 0; i < n; ++i) {
        const int u = disc[2 * i], v = disc[2 * i + 1];
        const int j = (u + 16) >> 2, b = (u + 16) & 3;
        wt[(v + 15) * 8 + j].x |= 1u << (8 * b);
        wt[(v + 15) * 8 + j].y |= (unsigned)(u + 16) << (8 * b);
    }
    hipMemcpyToSymbol(HIP_SYMBOL(c_discw), wt, sizeof(wt));
    {
        static const signed char pat[256 * 4] = {
#include "brief_pattern.inc"
        };
        std::vector<float> pf(1024);
        for (int i = 0; i < 1024; ++i) pf[i] = (float)pat[i];
        hipMemcpyToSymbol(HIP_SYMBOL(c_pattern_f), pf.data(), sizeof(float) * 1024);
    }
    {
        double v[7], sum = 0.;
        float g[7];
        for (int i = 0; i < 7; ++i) { const double x = (double)(i - 3); v[i] = exp(-0.125 * x * x); sum += v[i]; }
        for (int i = 0; i < 7; ++i) g[i] = (float)(v[i] / sum);
        hipMemcpyToSymbol(HIP_SYMBOL(c_gauss), g, sizeof(g));
    }
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an
// XCD and its L2), so workgroup b takes tile (b % 8) * ceil(n/8) + b / 8: every XCD walks one
// contiguous run of the raster-ordered tile list and neighbouring tiles (shared halo rows and
// shared 128-B lines) hit the same L2.  Only speed depends on this, never correctness.
__device__ __forceinline__ int xcd_tile(int b, int n)
{
    const int per = (n + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}

// Image-granular XCD mapping for the per-keypoint / per-candidate gather kernels: workgroups are dealt round-robin over
// the 8 XCDs (b and b + 8 share one), each XCD has its own 4 MB L2, and a gather kernel whose workgroups of ONE image
// land on all 8 XCDs pulls that image's pyramid into 8 L2s (r02 PMC: 8.75 GB fetched per step by the descriptor kernel
// for 3.3 GB of pyramids).  Linear block b -> XCD group x = b % 8, position idx = b / 8 inside the group; group x owns
// images x, x + 8, ... and walks them one after the other: img = x + 8 (idx / nb), blk = idx % nb.  Speed / traffic only.
__device__ __forceinline__ bool xcd_image_block(int nb, int n_img, int &img, int &blk)
{
    const int b = blockIdx.x, x = b & 7, idx = b >> 3;
    img = x + 8 * (idx / nb);
    blk = idx - (idx / nb) * nb;
    return img < n_img;
}
static inline unsigned xcd_image_grid(int nb, int n_img) { return (unsigned)(8 * ((n_img + 7) / 8) * nb); }

// ---------------------------------------------------------------- pyramid
// Workgroup = one wave = 256 x 16 destination tile of level l (PYR_TW x PYR_TH).  The source footprint in level l-1
// (at most PYR_ROWS = 23 rows x PYR_DW = 84 dwords; origin and row count come from the host's tile record, which
// build_tables checks against the window at create time) is staged in LDS with aligned 16-byte loads, all of them in
// flight before the first LDS store -- 7744 B per workgroup, so the LDS of a CU (160 KB) holds 21 windows.
// One lane = 4 destination columns x the tile's 16 rows, one run.  The bilinear chain is separable in exact integer
// arithmetic: h(src row, dst col) = a0 p[o] + a1 p[o+1] (16 bits), out = (b0 h(top) + b1 h(bottom) + 2^15) >> 16.
// Reading p[o+1] and the row below unclamped is exact: the coefficient tables give weight 0 wherever OpenCV clamps
// (last source column / row).  A source row passes the horizontal filter once: the h of a row's bottom source row stay
// in registers and are the next row's top h wherever the source row advances by one (15 rows of 16 at scale 1.1).
// Everything that is the same in all 64 lanes -- the tile record, the 16 row-table entries, weights, row offsets, the
// re-use mask, the destination row pointer -- lives in scalar registers.  The row loop is described where it stands.
// Cost per tile (static count of the gfx950 code, path of a full tile whose 15 later rows re-use): about 435 vector
// instructions and 34 LDS read instructions; the form before (both source rows filtered per output row, row constants
// built per lane, a division per window load) took 866 and 48.  Measured: 841 -> 444 vector instructions per tile, 1.63 ->
// 1.41 ms per step of 1024 VGA pairs.
// Why this tile.  The kernel lives on how many tile windows a CU keeps in flight (r02 diagnostic builds: loads + LDS alone
// 1.12 ms, rows + stores alone 1.26 ms, together 1.92 ms -- the phases of a workgroup overlap only through OTHER
// workgroups, and FAST run beside it on a second stream gained nothing: wave slots are the contended resource), so
// every instruction taken out of a tile's life shortens its stay in a wave slot.  A lane takes all 16 rows (half the
// waves per window of an 8-row split, the column constants serve 16 rows) and a tile is one wave: 64-row tiles of two
// waves measured 1.89 ms, 128 x 32 of one wave 1.68.  And the longer the contiguous rows the better the mixed read /
// write stream runs: 64-wide 1.82, 128-wide 1.67, 256 x 16 1.64 ms (all three with the row body of that time; partial
// tiles at the right edge idle lanes: 73 % of the lane-pixels of a VGA pyramid are pixels).
constexpr int PYR_THREADS = 64;
constexpr int PYR_LDS_DW = PYR_ROWS * PYR_DW + 4;          // +4: the unclamped p[o+1] of the last row's last column
constexpr int PYR_NQ = PYR_DW / 4;                                 // 16-byte chunks of a window row
constexpr int PYR_LROWS = PYR_THREADS / PYR_NQ;                    // window rows a round of loads covers: lane = (row tid / 21, chunk tid % 21)
constexpr int PYR_LLANES = PYR_LROWS * PYR_NQ;                     // lanes that stage a chunk per round (63)
constexpr int PYR_NLD = (PYR_ROWS + PYR_LROWS - 1) / PYR_LROWS;    // rounds
constexpr int PYR_NLD_FULL = (PYR_TH + 1 + PYR_LROWS - 1) / PYR_LROWS;  // rounds every tile runs: a full tile reads PYR_TH + 1 rows or more
constexpr int PYR_NCHUNK = PYR_ROWS * PYR_NQ;
static_assert(PYR_THREADS == PYR_TW / 4 && PYR_THREADS == 64 && PYR_TH == 16, "one wave per tile; a lane takes 4 columns x the tile's 16 rows");
static_assert(PYR_DW % 4 == 0, "window rows are whole 16-byte chunks");
static_assert(PYR_LROWS == 3 && PYR_LLANES == 63 && PYR_NLD == 8, "63 lanes x 8 rounds of 3 rows cover the 23 x 21 chunks");
static_assert(PYR_NCHUNK * 4 <= PYR_LDS_DW && (PYR_NLD - 1) * PYR_LLANES < PYR_NCHUNK, "only the last round is cut short by the window's end");
static_assert((PYR_ROWS + 1) * PYR_DW * 4 < (1 << PYR_YW_SHIFT), "a window byte offset fits the row field of the y table");
static_assert(PYR_LDS_DW * 4 == 7744, "LDS per tile window");
__global__ __launch_bounds__(PYR_THREADS) void pyr_resize_kernel(uint8_t *pyr, RpeDeviceLayout lay, const int *__restrict__ coef,
                                                                  const RpePyrTile *__restrict__ ptiles, int ntiles, int l)
{
    __shared__ __attribute__((aligned(16))) unsigned s_src[PYR_LDS_DW];
    const RpeLevel &S = lay.lv[l - 1];
    const RpeLevel &D = lay.lv[l];
    const int tid = threadIdx.x;
    const int ti = xcd_tile(blockIdx.x, ntiles);
    if (ti >= ntiles) return;
    // tile origin and source-window origin come from a host table: the two 64-bit divisions that derive the window from
    // the tile (floor(x0 * S.w / D.w), floor(y0 * S.h / D.h)) cost ~250 scalar instructions per wave when done here, and
    // the scalar unit issues at the same 1-per-4-cycles cadence per SIMD as the vector ALU
    // (one 16-byte scalar load: everything in the record is the same in all 64 lanes)
    const RpePyrTile pt = ptiles[ti];
    const int x0 = pt.x0, y0 = pt.y0, a0 = pt.a0, sy0 = pt.sy0, nsrc = pt.nsrc;
    const unsigned reuse = pt.reuse;
    const uint8_t *src = rpe_level_base(pyr, lay, blockIdx.y, l - 1);
    // per destination column: offset | weight << 16; per destination row: window byte offset of the source row (row x 4
    // PYR_DW) | weight << PYR_YW_SHIFT.  The device table pads the x run to a multiple of 128 and the y run to a multiple
    // of 64 entries (last entry replicated) and aligns both to 16 B, so a lane fetches its 4 columns with one 16-B load
    // and the wave its 16 rows with scalar loads (the address is uniform), without clamps
    const int *cxp = coef + D.dcoef_off, *cyp = cxp + ((D.w + 127) & ~127) + y0;
    // lane = column group of 4 pixels
    const int x4 = x0 + 4 * tid;
    // coefficient loads go out first, in the shadow of the window loads
    const int4 cv = *(const int4 *)(cxp + x4);
    unsigned ys[PYR_TH];
#pragma unroll
    for (int r = 0; r < PYR_TH; ++r) ys[r] = (unsigned)cyp[r];
    {   // all window loads (16 B per lane) in flight before the first LDS store (one HBM round trip per tile).  Lane =
        // (window row tid / 21, 16-B column tid % 21) + 3 rows per round q: one division per tile, and the LDS chunk of
        // round q is tid + 63 q.  Only rows 0 .. nsrc - 1 of the window are read by the tile: rows past them load row
        // nsrc - 1 again, and the rounds that lie past the rows every full tile needs (PYR_TH + 1 at any scale >= 1) are
        // skipped when they lie past nsrc (a uniform branch; 21 rows and up: never at scale 1.1).  Lane 63 loads a valid
        // chunk and stores nothing.
        const int lr = tid / PYR_NQ, lc = tid - lr * PYR_NQ;
        const unsigned colb = (unsigned)min(a0 + 16 * lc, S.pitch - 16) + __umul24((unsigned)sy0, (unsigned)S.pitch);   // pitch is a multiple of 16; clamped columns are never read
        const unsigned off0 = colb + __umul24((unsigned)lr, (unsigned)S.pitch), offmax = colb + __umul24((unsigned)(nsrc - 1), (unsigned)S.pitch);
        const unsigned pitch3 = PYR_LROWS * S.pitch;
        uint4 stage[PYR_NLD];
#pragma unroll
        for (int q = 0; q < PYR_NLD; ++q)
            if (q < PYR_NLD_FULL || PYR_LROWS * q < nsrc) stage[q] = *(const uint4 *)(src + min(off0 + q * pitch3, offmax));
        // pin the loads above the guarded stores: left alone the compiler sinks every load into the block of its store
        // (load, s_waitcnt vmcnt(0), ds_write, next load ...: dependent HBM round trips instead of one)
#pragma unroll
        for (int q = 0; q < PYR_NLD; ++q)
            if (q < PYR_NLD_FULL || PYR_LROWS * q < nsrc) asm volatile("" : "+v"(stage[q].x), "+v"(stage[q].y), "+v"(stage[q].z), "+v"(stage[q].w));
        if (tid < PYR_LLANES) {
#pragma unroll
            for (int q = 0; q < PYR_NLD; ++q)
                if ((q < PYR_NLD_FULL || PYR_LROWS * q < nsrc) && (PYR_LLANES * (q + 1) <= PYR_NCHUNK || tid < PYR_NCHUNK - PYR_LLANES * q))
                    ((uint4 *)s_src)[tid + PYR_LLANES * q] = stage[q];
        }
    }
    // per-lane column constants: source offsets o_j (non-decreasing, o_3 - o_0 <= 4) -> byte selectors, packed weights
    typedef unsigned short v2u16_t __attribute__((ext_vector_type(2)));
    unsigned selp[4];              // v_perm selector of column j: bytes (p[o_j], 0, p[o_j + 1], 0) of the 8 window bytes from o_0 on
    v2u16_t apk[4];                // (256 - a1_j, a1_j)
    int bcol;                      // window byte column of o_0
    {
        const int cw[4] = {cv.x, cv.y, cv.z, cv.w};
        const int o0 = cw[0] & 0xFFFF;
        bcol = o0 - a0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned rel = (unsigned)min(max((cw[j] & 0xFFFF) - o0, 0), 4);   // columns past D.w repeat the last entry: rel stays in range
            selp[j] = 0x0c000c00u | rel | ((rel + 1u) << 16);
            const unsigned a1 = (unsigned)cw[j] >> 16;
            apk[j] = __builtin_bit_cast(v2u16_t, (256u - a1) | (a1 << 16));
        }
    }
    // row constants: the table entries are scalars (waited for once, before the row loop, and never behind a vmcnt that
    // would also wait for the previous row's global STORE), so a row's weights and the window offset of its source row
    // come from scalar code; the lane's own term is one register: the LDS byte offset of the dword holding p[o_0] in
    // window row 0, less the window's first row
    const unsigned vbase = ((unsigned)bcol & ~3u) - (unsigned)sy0 * (PYR_DW * 4);
    __syncthreads();
    if (x4 >= D.pitch) return;
    // One source row = three aligned LDS dwords from the one holding p[o_0] (the 4 columns span <= 6 bytes), two v_alignbyte
    // to the lane's byte phase, then per column j a v_perm_b32 -> (p[o_j], p[o_j + 1]) as two u16 and a v_dot2_u32_u16 with
    // (256 - a1_j, a1_j) -> h_j (16 bits): 10 vector instructions and 3 LDS reads.  (Byte-unaligned ds_read_b64 straight at
    // p[o_0] saves the two v_alignbyte and was measured 70 % SLOWER: the LDS serialises misaligned 8-byte lanes.)
    const unsigned sh = (unsigned)bcol & 3u;
    auto fetch = [&](unsigned lds_byte, unsigned (&t)[3]) {
        const unsigned *p = (const unsigned *)((const uint8_t *)s_src + lds_byte);
        t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
    };
    auto hpass = [&](const unsigned (&t)[3], unsigned (&hh)[4]) {
        const unsigned lo = __builtin_amdgcn_alignbyte(t[1], t[0], sh), hi = __builtin_amdgcn_alignbyte(t[2], t[1], sh);
#pragma unroll
        for (int j = 0; j < 4; ++j) hh[j] = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16_t, __builtin_amdgcn_perm(hi, lo, selp[j])), apk[j], 0u, false);
    };
    // the four results of a row are byte 2 of four 24-bit sums; bytes past D.w stay 0: their selector byte picks the constant 0
    const unsigned colmask = x4 + 3 < D.w ? 0xFFFFFFFFu : (x4 >= D.w ? 0u : (0xFFFFFFFFu >> (8 * (x4 + 4 - D.w))));
    const unsigned sel01 = (0x0c0c0602u & colmask) | (0x0c0c0c0cu & ~colmask), sel23 = (0x06020c0cu & colmask) | (0x0c0c0c0cu & ~colmask);
    // One output row = the horizontal pass of its bottom source row + the vertical blend
    //   out_j = (b0 h_top + b1 h_bot + 2^15) >> 16 by two 24-bit mads.
    // The bottom row is the top row + one window row -- where OpenCV clamps it (last source row) its weight is 0 and whatever
    // the window holds there is finite, so the unclamped read is exact.  The top row's h is the previous output row's bottom h
    // wherever the source row advances by exactly one (bit r of the tile's reuse mask, a scalar: 15 rows of 16 at scale 1.1);
    // the first row of a tile and rows after a step of 0 or 2 pass their top row too.  The 16 rows are one unrolled run and
    // the two sets of four h alternate between top and bottom from row to row, so the two paths join without a copy.  Both
    // branches of a row (reuse, rows past D.h in the last tile row) are scalar.
    uint8_t *drow = pyr + (long long)blockIdx.y * lay.stride + D.off + __umul24((unsigned)y0, (unsigned)D.pitch) + x0;
    const int nrows = min(PYR_TH, D.h - y0);
    unsigned vo = 4u * (unsigned)tid, half = 32768u;
    asm("" : "+v"(half));                    // the rounding term stays in one register (it is an operand of a three-operand mad)
    auto rowtop = [&](int r) { return (ys[r] & ((1u << PYR_YW_SHIFT) - 1u)) + vbase; };
    unsigned hs[2][4], nb[3];
    fetch(rowtop(0) + PYR_DW * 4, nb);
#pragma unroll
    for (int r = 0; r < PYR_TH; ++r) {
        if (r == 0 || !((reuse >> r) & 1u)) { unsigned tt[3]; fetch(rowtop(r), tt); hpass(tt, hs[r & 1]); }
        // the next row's bottom source row is on its way from LDS while this row is computed
        const unsigned cb[3] = {nb[0], nb[1], nb[2]};
        if (r + 1 < PYR_TH) fetch(rowtop(r + 1) + PYR_DW * 4, nb);
        hpass(cb, hs[(r + 1) & 1]);
        const unsigned (&ht)[4] = hs[r & 1], (&hb)[4] = hs[(r + 1) & 1];
        const unsigned b1u = ys[r] >> PYR_YW_SHIFT, b0u = 256u - b1u;
        unsigned sm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned t = __umul24(b0u, ht[j]) + half;
            asm("" : "+v"(t));               // two v_mad_u32_u24 per column; left alone the sums are re-associated into mul, mul, add3
            sm[j] = __umul24(b1u, hb[j]) + t;
        }
        asm("" : "+v"(vo));                  // keeps the zero-extension in the row's block: the store takes (scalar row pointer, lane offset)
        // rows past D.h (last tile row of a level) are computed like any other -- the y table repeats its last entry, so they
        // read inside the window -- and only their store is skipped: a branch around the whole row would make every value
        // carried from row to row a merge of two paths, paid for in copies by all rows
        if (r < nrows) *(unsigned *)(drow + vo) = __builtin_amdgcn_perm(sm[1], sm[0], sel01) | __builtin_amdgcn_perm(sm[3], sm[2], sel23);
        drow += D.pitch;
    }
}

void rpe_launch_pyramid(rpe_handle *h, int n_img, int l0, int l1)
{
    for (int l = std::max(l0, 1); l < l1; ++l) {
        const int nt = h->pyr_tile_cnt[l];
        hipLaunchKernelGGL(pyr_resize_kernel, dim3((nt + 7) / 8 * 8, n_img), dim3(PYR_THREADS), 0, h->stream, h->d_pyr, h->lay, h->d_coef,
                           (const RpePyrTile *)(h->d_pyr_tiles + h->pyr_tile_off[l]), nt, l);
    }
}

// ------------------------------------------------------------- FAST + NMS
// Fused FAST-9/16 score + 3x3 non-maximum suppression + border filter.
// Tile = 64x64 output pixels; scores are needed on 66x66, pixels on 72x72 (halo 3+1
// rows, 4 columns => dword aligned).  ~5 KB of loads in flight per workgroup.
//  phase 1: every dword group (4 px) of the 66x72 score area: OpenCV's pair test on the
//           4 compass + 4 diagonal ring pixels, darker and brighter side apart:
//           a 9-arc contains one pixel of every opposite pair, so a darker (brighter) arc needs
//           every pair to hold a pixel below v - thr (above v + thr).  The four pixels stay four
//           bytes of one register: each comparison is the carry of a byte sum against a saturated
//           threshold (v_lerp_u8, bit 7 of every byte), the pair logic runs on whole dwords.
//           Exact for every (r, v, thr): tests/test_fast_bytes_cpu.py.  Survivors are appended
//           to an LDS list with one wave-aggregated LDS atomic per wave: candidates with a darker
//           arc possible from the front, brighter-only ones from the back.
//  phase 2: the list in one contiguous slice per wave: the score of the possible side(s) only,
//           window-9 min/max via min3/max3 on the raw ring values, score - 1 into the LDS score
//           tile; the corners (score > thr) are compacted to the front of the wave's slice.
//  phase 3: strict 3x3 maximum on the LDS score tile over the corners only, 31-px border
//           filter (KeyPointsFilter::runByImageBorder), per-tile keypoint list to HBM.
__device__ __forceinline__ int imax3(int a, int b, int c) { return max(a, max(b, c)); }
// one v_max3_u32 / v_min3_u32 per window of 3: left to itself the compiler shares two-input partial results between
// neighbouring windows (max(r[k+1], r[k+2]) ...) and spends ~48 instructions on a side's windows of 3 and 9 and the
// reduction instead of 16 + 16 + 8
__device__ __forceinline__ int vmax3u(int a, int b, int c) { int d; asm("v_max3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
__device__ __forceinline__ int vmin3u(int a, int b, int c) { int d; asm("v_min3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));
// Bresenham circle of radius 3 (fast.cpp), compile-time offsets
static constexpr int CIRC_DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
static constexpr int CIRC_DY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

constexpr int FS_ROWS = FAST_TH + 2;         // score rows (y0-1 .. y0+FAST_TH)
constexpr int FAST_PROWS = FAST_TH + 8;      // pixel rows (y0-4 .. y0+FAST_TH+3)
constexpr int FAST_THREADS = 256;
constexpr int FAST_NRP = 14;                 // rows of the 18-dword tile row that one pass of the lanes covers
constexpr int FAST_LANES = FAST_NRP * 18;    // the 252 lanes that load pixels and run phase 1
constexpr int FAST_NCAND = FS_ROWS * 72;     // candidate list capacity: one entry per score-area pixel at most
static_assert(FAST_LANES <= FAST_THREADS, "a pass of FAST_NRP tile rows fits the workgroup");
static_assert(FAST_ENTRY_NRP == FAST_NRP && FAST_ENTRY_LANES == FAST_LANES && FAST_ENTRY_PITCH == 72 && FAST_ENTRY_NPASS == 5,
              "fast_entry.h describes this kernel's lane mapping");
static_assert(6 * FAST_NRP >= FAST_PROWS && 5 * FAST_NRP >= FS_ROWS, "6 load passes cover the pixel rows, 5 phase-1 passes the score rows");
static_assert(RPE_FAST_TILE_CAP == (64 / 2) * (FAST_TH / 2), "strict 3x3 maxima of a tile");
static_assert(RPE_FAST_TILE_CAP <= FAST_PROWS * 18, "the tile's keypoint list lives in the dead pixel tile");
static_assert((FAST_PROWS * 18 + FS_ROWS * 18) * 4 + FAST_NCAND * 2 + 8 == 19448, "LDS per workgroup");
// Output: one compact list per tile of the keypoints that survive NMS and the border filter, packed
// score << 24 | y << 12 | x (level coordinates).  A strict 3x3
// maximum cannot have an 8-neighbour that is one too, so a 64x64 tile holds at most 32*32 = 1024 of them:
// RPE_FAST_TILE_CAP is never exceeded and nothing is ever dropped here.  ~0.5 % of the pixels survive, so
// the lists replace a dense NMS map (1.6 MB written + re-read per VGA image) by ~100 bytes per tile; list
// order inside a tile depends on wave timing, which nothing downstream reads (select ranks by (y, x)).
__global__ __launch_bounds__(FAST_THREADS) void fast_nms_kernel(const uint8_t *__restrict__ pyr, unsigned *__restrict__ tile_list,
                                                        int *__restrict__ tile_cnt, RpeDeviceLayout lay,
                                                        const RpeTile *__restrict__ tiles, int ntiles, int t0, int nt)
{
    // 19448 B of LDS per workgroup = 8 workgroups (32 waves) per CU: the pixel tile is dead after phase 2, so the keypoint
    // list of phase 3 lives in its place (4096 <= 5184 bytes); with a list of its own (24.5 KB) only 6 workgroups fitted
    __shared__ __attribute__((aligned(16))) unsigned s_in[FAST_PROWS * 18];        // pixels  y0-4 .. y0+FAST_TH+3, x0-4 .. x0+67
    __shared__ __attribute__((aligned(16))) unsigned s_sc[FS_ROWS * 18];   // scores  y0-1 .. y0+64, x0-4 .. x0+67
    unsigned *s_out = s_in;                                               // phase 3: the tile's keypoint list [1024]
    __shared__ unsigned short s_cand[FAST_NCAND];
    __shared__ int s_ncand, s_nout;
    const int tid = threadIdx.x, lane = tid & 63;
    // this launch's run [t0, t0 + nt) of the tile table (a level group, orb_groups.h, or all of it); the slots keep the
    // table's stride ntiles
    const int tr = xcd_tile(blockIdx.x, nt);
    if (tr >= nt) return;
    const int ti = t0 + tr;
    const RpeTile t = tiles[ti];
    const RpeLevel &L = lay.lv[t.level];
    const int w = L.w, hgt = L.h, pitch = L.pitch, thr = lay.fast_thr;
    const int x0 = t.tx, y0 = t.ty;
    const long long tslot = (long long)blockIdx.y * ntiles + ti;
    // tiles that cannot contain a keypoint after the border filter (the host table lists none): empty list
    const bool live = w > 2 * RPE_EDGE && hgt > 2 * RPE_EDGE && x0 < w - RPE_EDGE && x0 + 64 > RPE_EDGE &&
                      y0 < hgt - RPE_EDGE && y0 + FAST_TH > RPE_EDGE;
    if (!live) {
        if (tid == 0) tile_cnt[tslot] = 0;
        return;
    }
    const uint8_t *src = rpe_level_base(pyr, lay, blockIdx.y, t.level);
    if (tid == 0) { s_ncand = 0; s_nout = 0; }
    {   // all tile loads in flight before the first LDS store.  lane -> fixed dword column (tid % 18) and rows
        // tid / 18 + 14 q: one column clamp and one division per tile instead of one per load.  Only the upper clamps
        // exist (last tile row and column): a FAST tile starts at x0 >= FAST_TILE_X0 = 28 and y0 >= RPE_EDGE = 31
        // (build_tables checks its table against both), so x0 - 4 and y0 - 4 are never negative
        const int lc = tid % 18, lr = tid / 18;
        const int lx = min(x0 - 4 + 4 * lc, pitch - 4);
        unsigned stage[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int r = min(lr + FAST_NRP * q, FAST_PROWS - 1);
            const int y = min(y0 - 4 + r, hgt - 1);
            stage[q] = *(const unsigned *)(src + (__umul24((unsigned)y, (unsigned)pitch) + (unsigned)lx));
        }
        // pin the loads above the guarded stores (the compiler sinks a load into the block of its store: dependent round trips)
#pragma unroll
        for (int q = 0; q < 6; ++q) asm volatile("" : "+v"(stage[q]));
#pragma unroll
        for (int q = 0; q < 6; ++q) { const int r = lr + FAST_NRP * q; if (tid < FAST_LANES && r < FAST_PROWS) s_in[r * 18 + lc] = stage[q]; }
    }
    {   // zero the score tile with 16-B LDS stores
        uint4 *z1 = (uint4 *)s_sc;
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < FS_ROWS * 18 / 4; i += FAST_THREADS) z1[i] = z;
    }
    __syncthreads();
    // ---- phase 1 (byte SWAR: the four pixels of the dword group in one VGPR, two v_lerp_u8 per ring pixel)
    // lane -> fixed dword column c (18 per row) and rows r0, r0+14, ... : the x-validity mask is
    // computed once per tile and the candidate bits of the 5 rows are appended in one go
    const unsigned T0 = (unsigned)thr * 0x01000100u;                      // thr in the high byte of both 16-bit lanes
    const int c = tid % 18, r0 = tid / 18;
    unsigned dark_bits = 0, brt_bits = 0, ndark_bits = 0xFFFFFFFFu;
    if (tid < FAST_LANES) {
        const int cl = max(c - 1, 0), cr = min(c + 1, 17);
        const int pxb = x0 - 4 + 4 * c;
        const int xlo = max(x0 - 1, RPE_EDGE - 1), xhi = min(x0 + 64, w - RPE_EDGE);   // valid px range (inclusive)
        unsigned vmask = 0xFu;
        if (pxb < xlo) vmask &= 0xFu << min(xlo - pxb, 4);
        if (pxb + 3 > xhi) vmask &= 0xFu >> min(pxb + 3 - xhi, 4);
        vmask &= 0xFu;
        // candidate flags of the 5 rows share one dword per side: pixel px of row it -> bit 8 px + it (a row's flags are
        // bit 7 of its four bytes and drop into place by a shift and a v_bfi / v_and_or: 2 instructions per row and side
        // instead of 14 for the compact 4-bit form; the x-validity mask is applied once, spread to bytes).  The darker side
        // is kept inverted ("no darker arc") until the five rows are done
        const unsigned vmask5 = ((vmask * 0x00204081u) & 0x01010101u) * 0x1Fu;
        // The compiler pairs the 11 dwords of a row into four ds_read2_b32 + three ds_read_b32; a pass is 252 dwords and a
        // ds_read2 offset ends at 255, so rows 1-4 pay four address additions each.  Eleven single ds_read_b32 (volatile LDS
        // pointers; their 16-bit byte offset reaches every pass) took the additions out and were not faster: four more
        // LDS instructions a row cost what the four additions did
        const unsigned *pC = s_in + (r0 + 3) * 18 + c, *pL = s_in + (r0 + 3) * 18 + cl, *pR = s_in + (r0 + 3) * 18 + cr;
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int ry = r0 + FAST_NRP * it;
            const int py = y0 - 1 + ry;
            if (vmask == 0 || ry >= FS_ROWS || py < RPE_EDGE - 1 || py >= hgt - RPE_EDGE + 1) continue;
            // input row of this score row = ry + 3; the three column pointers are per-lane constants, the rows compile-time
            // offsets from them (ds_read immediate offsets instead of six address instructions per row)
            const int ro = FAST_NRP * 18 * it;
            const unsigned cdw = pC[ro], ldw = pL[ro], rdw = pR[ro];
            const unsigned upl = pL[ro - 36], upc = pC[ro - 36], upr = pR[ro - 36];
            const unsigned dnl = pL[ro + 36], dnc = pC[ro + 36], dnr = pR[ro + 36];
            const unsigned bot = pC[ro + 54], top = pC[ro - 54];
            // thresholds of the row, per byte, from n = ~v: Yd = min(n + thr, 255), Yb = max(n - thr, 0).  The even bytes
            // (n << 8) and the odd ones (n itself) sit in the HIGH bytes of 16-bit lanes; thr << 8 has an empty low byte, so
            // whatever is in the low bytes neither carries nor borrows, and the clamps (0xFFFF / 0) are 255 / 0 in the high byte
            const unsigned n = ~cdw;
            const ushort2_t ne = __builtin_bit_cast(ushort2_t, n << 8), no = __builtin_bit_cast(ushort2_t, n);
            const ushort2_t T8 = __builtin_bit_cast(ushort2_t, T0);
            const unsigned Yd = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, __builtin_elementwise_add_sat(no, T8)),
                                                      __builtin_bit_cast(unsigned, __builtin_elementwise_add_sat(ne, T8)), 0x07030501u);
            const unsigned Yb = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(no, T8)),
                                                      __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(ne, T8)), 0x07030501u);
            // ring values of the four pixels, one byte each: v_alignbyte_b32 shifts the dword pair {hi:lo} right by sh bytes
            unsigned r[8];
            r[0] = bot;                                         // ( 0, 3)
            r[1] = top;                                         // ( 0,-3)
            r[2] = __builtin_amdgcn_alignbyte(rdw, cdw, 3);     // ( 3, 0)
            r[3] = __builtin_amdgcn_alignbyte(cdw, ldw, 1);     // (-3, 0)
            r[4] = __builtin_amdgcn_alignbyte(dnr, dnc, 2);     // ( 2, 2)
            r[5] = __builtin_amdgcn_alignbyte(upc, upl, 2);     // (-2,-2)
            r[6] = __builtin_amdgcn_alignbyte(upr, upc, 2);     // ( 2,-2)
            r[7] = __builtin_amdgcn_alignbyte(dnc, dnl, 2);     // (-2, 2)
            // v_lerp_u8: per byte (a + b + (c & 1)) >> 1 with a 9-bit sum, so bit 7 is the carry of a + b + (c & 1):
            //   nd: r + Yd + 1 >= 256  <=>  r >= v - thr  (not darker; always when thr >= v: Yd = 255)
            //   br: r + Yb     >= 256  <=>  r >  v + thr  (brighter;   never  when v + thr >= 255: Yb = 0)
            unsigned nd[8], br[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                nd[k] = __builtin_amdgcn_lerp(r[k], Yd, 0xFFFFFFFFu);
                br[k] = __builtin_amdgcn_lerp(r[k], Yb, 0u);
            }
            // opposite pairs (0,1) (2,3) (4,5) (6,7), whole dwords, the flags in bit 7 of each byte:
            //   no darker arc:         some pair with both pixels not darker
            //   brighter arc possible: every pair holds a brighter pixel
            // one three-input instruction per further pair (v_and_or_b32 and its dual, v_bitop3_b32 with the truth table
            // of (a | b) & c): left to itself the compiler balances the chains into five instructions a side instead of four
            unsigned xnd = nd[0] & nd[1], xb = br[0] | br[1];
#pragma unroll
            for (int k = 2; k < 8; k += 2) {
                xnd = __builtin_amdgcn_bitop3_b32(nd[k], nd[k + 1], xnd, 0xEA);     // (a & b) | c
                xb = __builtin_amdgcn_bitop3_b32(br[k], br[k + 1], xb, 0xA8);       // (a | b) & c
            }
            // drop bit 7 of the four bytes into bits 8 px + it (v_bfi_b32); rows that are skipped keep "no darker arc"
            const unsigned rowm = 0x01010101u << it;
            ndark_bits = (ndark_bits & ~rowm) | ((xnd >> (7 - it)) & rowm);
            brt_bits |= (xb >> (7 - it)) & rowm;
        }
        dark_bits = ~ndark_bits & vmask5;
        brt_bits &= vmask5;
    }
    {   // one append per tile: wave prefix sum of the per-lane counts (front | back << 16), one LDS atomic per wave.
        // List entry in lane form (fast_entry.h): (tid << 5) | bit position | side bits, 0x4000 darker arc possible, 0x8000
        // brighter arc possible -- the lane's part with the side bits is one register, so a trip is find-first-set, clear
        // the bit, or, store, advance.  Entries with the darker side go to the front, brighter-only ones to the back, so
        // the lanes of a phase-2 round almost always share one side.  The 0.1 % with both sides possible follow the
        // darker-only ones at the front in a loop of their own, which most waves skip: taking the brighter flag out of
        // brt_bits per bit cost every trip of the darker loop two instructions.  Both lists together hold at most one
        // entry per score-area pixel.
        const unsigned both_bits = brt_bits & dark_bits, do_bits = dark_bits & ~brt_bits, bo_bits = brt_bits & ~dark_bits;
        const int n = __popc(dark_bits) | (__popc(bo_bits) << 16);
        const int inc = wave_inclusive_sum(n);
        const int total = __shfl(inc, 63);
        if (total) {
            int base = 0;
            if (lane == 63) base = atomicAdd(&s_ncand, total);
            const int pre = __shfl(base, 63) + inc - n;
            // one loop per kind of entry: choosing the side per bit inside one loop cost 20 instructions per trip instead
            // of ~10, more than the trips it saves
            unsigned short *wF = s_cand + (pre & 0xFFFF), *wB = s_cand + (FAST_NCAND - 1 - (pre >> 16));
            const unsigned ebase = fast_entry_lane_base((unsigned)tid);
            auto append = [&](unsigned bits, unsigned sides, unsigned short *&w, int step) {
                unsigned e = fast_entry_lane(ebase, 0u, sides);
                asm("" : "+v"(e));           // one register for the loop: left alone the constant is or-ed in again on every trip
                while (bits) {
                    const unsigned bpos = (unsigned)__ffs((int)bits) - 1u;
                    bits &= bits - 1;
                    *w = (unsigned short)(e | bpos);
                    w += step;
                }
            };
            append(do_bits, FAST_ENTRY_DARK, wF, 1);
            append(both_bits, FAST_ENTRY_SIDES, wF, 1);
            append(bo_bits, FAST_ENTRY_BRIGHT, wB, -1);
        }
    }
    __syncthreads();
    // ---- phase 2: virtual list index j in [0, nF + nB) -> s_cand[j] (front), s_cand[j + gap] (back).  Wave wv takes the
    // slice [jb, je) in rounds of 64 and compacts the corners of the slice to s_cand[cb ..] (cb = the slice's first
    // physical index).  A corner's physical write index never passes the read index of the round (the gap between the
    // lists is free), and the slices do not overlap, so no other lane's unread entry is overwritten.
    const int ncand = s_ncand;
    const int nF = ncand & 0xFFFF, nB = ncand >> 16, nc = nF + nB, gap = FAST_NCAND - nc;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = ((nc + FAST_THREADS - 1) / FAST_THREADS) * 64;
    const int jb = min(wv * slice, nc), je = min(jb + slice, nc);
    const int cb = jb < nF ? jb : jb + gap;
    int ncorner = 0;
    const uint8_t *sb = (const uint8_t *)s_in;
    for (int j0 = jb; j0 < je; j0 += 64) {                              // wave-uniform trip count
        const int j = j0 + lane;
        bool corner = false;
        int cc = 0;
        if (j < je) {
            cc = s_cand[j < nF ? j : j + gap];
            // lane form: the byte offset 72 ry + bx of the pixel comes straight from the entry's fields (fast_entry.h)
            const unsigned off = fast_entry_offset((unsigned)cc);
            const uint8_t *p = sb + 3 * 72 + off;
            const int v = p[0];
            int r[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) r[k] = p[CIRC_DY[k] * 72 + CIRC_DX[k]];
            // with d = v - r: the darker score A = max_k min_arc9(k) d = v - min_k max_arc9(k) r, the brighter one
            // -Bm = -min_k max_arc9(k) d = max_k min_arc9(k) r - v; a side that phase 1 ruled out has a score <= thr
            // (necessary condition above), so max(A, -Bm) > thr iff the possible side's score is, and then it is that score
            int s = 0;
            if (cc & 0x4000) {
                int x3[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) x3[k] = vmax3u(r[k], r[(k + 1) & 15], r[(k + 2) & 15]);
                int x9[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) x9[k] = vmax3u(x3[k], x3[(k + 3) & 15], x3[(k + 6) & 15]);
                const int m = min(vmin3u(vmin3u(x9[0], x9[1], x9[2]), vmin3u(x9[3], x9[4], x9[5]), vmin3u(x9[6], x9[7], x9[8])),
                                  vmin3u(vmin3u(x9[9], x9[10], x9[11]), vmin3u(x9[12], x9[13], x9[14]), x9[15]));
                s = v - m;
            }
            if (cc & 0x8000) {
                int m3[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) m3[k] = vmin3u(r[k], r[(k + 1) & 15], r[(k + 2) & 15]);
                int m9[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) m9[k] = vmin3u(m3[k], m3[(k + 3) & 15], m3[(k + 6) & 15]);
                const int m = max(vmax3u(vmax3u(m9[0], m9[1], m9[2]), vmax3u(m9[3], m9[4], m9[5]), vmax3u(m9[6], m9[7], m9[8])),
                                  vmax3u(vmax3u(m9[9], m9[10], m9[11]), vmax3u(m9[12], m9[13], m9[14]), m9[15]));
                s = max(s, m - v);
            }
            if (s > thr) {
                ((uint8_t *)s_sc)[off] = (uint8_t)(s - 1);
                corner = true;
            }
        }
        const unsigned long long km = __ballot(corner);
        // a corner goes back in compact form (ry << 7) | bx | side bits, which is what phase 3 reads
        if (corner) s_cand[cb + ncorner + __popcll(km & ((1ull << lane) - 1ull))] = (unsigned short)fast_entry_to_compact((unsigned)cc);
        ncorner += __popcll(km);
    }
    __syncthreads();
    // ---- phase 3: NMS + border filter over the wave's own corners (only a corner can be a maximum: a pixel without a
    // score holds 0); survivors are appended to the tile's list, one LDS atomic per wave and round.
    // The pixel tile is dead now (the barrier above ended phase 2): its LDS holds the list.
    const uint8_t *sc = (const uint8_t *)s_sc;
    for (int i0 = 0; i0 < ncorner; i0 += 64) {                          // wave-uniform trip count: the ballot sees whole waves
        const int i = i0 + lane;
        bool keep = false;
        unsigned ent = 0;
        if (i < ncorner) {
            const int cc = s_cand[cb + i];
            const int bx = (int)fast_entry_compact_bx((unsigned)cc), ry = (int)fast_entry_compact_ry((unsigned)cc);
            const int px = x0 - 4 + bx, py = y0 - 1 + ry;
            // branch-free: the eight neighbour reads go out together (as a short-circuit chain they were nine dependent LDS
            // round trips with an exec-mask save / restore each); reads of halo corners past the score tile land in
            // other LDS arrays of this kernel and are discarded by `inside`
            const bool inside = (unsigned)(bx - 4) < 64u & (unsigned)(ry - 1) < (unsigned)FAST_TH &                 // halo pixels are not outputs
                                (unsigned)(px - RPE_EDGE) < (unsigned)(w - 2 * RPE_EDGE) & (unsigned)(py - RPE_EDGE) < (unsigned)(hgt - 2 * RPE_EDGE);
            const uint8_t *q = sc + ry * 72 + bx;
            const int v = q[0];
            const int nmax = imax3(imax3(q[-1], q[1], q[-73]), imax3(q[-72], q[-71], q[71]), max((int)q[72], (int)q[73]));
            if (inside & (v > nmax)) {
                keep = true;
                ent = ((unsigned)v << 24) | ((unsigned)py << 12) | (unsigned)px;
            }
        }
        const unsigned long long km = __ballot(keep);
        if (km) {                                              // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_nout, __popcll(km));
            base = __shfl(base, 0);
            if (keep) s_out[base + __popcll(km & ((1ull << lane) - 1ull))] = ent;
        }
    }
    __syncthreads();
    const int nout = s_nout;                                   // <= RPE_FAST_TILE_CAP by the NMS argument above
    unsigned *dst = tile_list + tslot * RPE_FAST_TILE_CAP;
    for (int i = tid; i < nout; i += FAST_THREADS) dst[i] = s_out[i];
    if (tid == 0) tile_cnt[tslot] = nout;
}

void rpe_launch_fast(rpe_handle *h, int n_img, int t0, int nt, hipStream_t stream)
{
    // tiles cover the border-filtered region only
    if (nt == 0) return;
    hipLaunchKernelGGL(fast_nms_kernel, dim3((nt + 7) / 8 * 8, n_img), dim3(FAST_THREADS), 0, stream,
                       h->d_pyr, h->d_tile_list, h->d_tile_cnt, h->lay, h->d_tiles_fast, h->n_tiles_fast, t0, nt);
}

// ----------------------------------------------------------------- select
// cv2's keypoint ORDER (orb.cpp computeKeyPoints): FAST emits a level's corners in raster order, then
// KeyPointsFilter::retainBest(2 * quota) on the FAST score reorders them through std::nth_element + std::partition;
// the Harris responses are computed for the survivors in THAT order and retainBest(quota) reorders them once more.
// The reference's own result rows pin this order (retain_best_emul.h, tests/test_reference_rows_cpu.py), so the
// selection is replayed move for move:
//   raster_corners  one workgroup per (level, image): the level's FAST tile lists -> ONE list in raster order
//                   (counting sort over rows in LDS, rank by x inside a row), the first ccap entries
//   retain_fast     one workgroup per (level, image): retainBest(2 * quota) on the FAST score -> candidates
//   harris          (below)
//   retain_harris   one workgroup per (level, image): retainBest(quota) on the Harris response, in place
//   compact         one workgroup per image: level-major concatenation into the keypoint arrays
// Raster order, pass by pass:
//   pass 1  per-row count of the entries (LDS atomics)                          -> exclusive scan = row starts
//   pass 2  entry -> slot row_start[y] + (arrival order inside the row); rows that start at or beyond the
//           capacity are dropped here (their ranks are >= ccap whatever their x)
//   pass 3  rank inside the row by x (a row holds a handful of entries) -> final position; positions >= ccap
//           are truncated exactly as the oracle truncates (first ccap in raster order) and flagged.
// Arrival order inside a row depends on wave timing; the final position does not.
__global__ __launch_bounds__(256) void raster_corners_kernel(const unsigned *__restrict__ tile_list, const int *__restrict__ tile_cnt,
                                                              unsigned *__restrict__ corner, int *__restrict__ corner_count,
                                                              unsigned *__restrict__ ovf, RpeDeviceLayout lay, int ntiles, int rows_cap, int key_cap, int l0)
{
    extern __shared__ unsigned s_dyn[];
    unsigned *s_rs = s_dyn;                          // [rows_cap + 1] per-row counts, then exclusive row starts
    unsigned *s_fill = s_rs + rows_cap + 1;          // [rows_cap] arrival counters
    unsigned *s_key = s_fill + rows_cap;             // [key_cap] staged entries (score << 24 | y << 12 | x), grouped by row
    unsigned *s_toff = s_key + key_cap;              // [level tiles + 1] exclusive prefix of the tile counts
    __shared__ int s_wave[5];
    __shared__ int s_live;
    const int tid = threadIdx.x, l = l0 + blockIdx.x, img = blockIdx.y;
    const RpeLevel &L = lay.lv[l];
    if (tid == 64) s_live = 0x7FFFFFFF;
    const int nrows = L.h, nt = L.ntile, ccap = L.ccap;
    for (int i = tid; i <= nrows; i += 256) s_rs[i] = 0;
    for (int i = tid; i < nrows; i += 256) s_fill[i] = 0;
    // exclusive prefix of the level's tile counts (<= 16 tiles per lane and round)
    const int *tc = tile_cnt + (long long)img * ntiles + L.tile0;
    const unsigned *tl = tile_list + ((long long)img * ntiles + L.tile0) * RPE_FAST_TILE_CAP;
    int nraw = 0;
    for (int t0 = 0; t0 < nt; t0 += 256) {                 // block-uniform
        const int t = t0 + tid;
        const int c = t < nt ? tc[t] : 0;
        int total;
        const int ex = block_excl_scan(c, s_wave, total);
        if (t < nt) s_toff[t] = (unsigned)(nraw + ex);
        nraw += total;
    }
    if (tid == 0) s_toff[nt] = (unsigned)nraw;
    __syncthreads();
    // entry s of the concatenated lists -> (tile, index) by binary search over the prefix
    auto fetch = [&](int sidx) -> unsigned {
        int lo = 0, hi = nt;                               // s_toff[lo] <= sidx < s_toff[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_toff[mid] <= (unsigned)sidx) lo = mid; else hi = mid; }
        return tl[(long long)lo * RPE_FAST_TILE_CAP + (sidx - (int)s_toff[lo])];
    };
    // both passes over the lists take four entries per lane and round: four independent loads in flight instead of one
    // dependent L2 / HBM round trip per 256 entries
    for (int base = 0; base < nraw; base += 1024) {
        unsigned e4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int sidx = base + tid + 256 * u; e4[u] = sidx < nraw ? fetch(sidx) : 0u; }   // score 0 = no entry
#pragma unroll
        for (int u = 0; u < 4; ++u) if (e4[u] >> 24) atomicAdd(&s_rs[(e4[u] >> 12) & 0xFFFu], 1u);
    }
    __syncthreads();
    // exclusive scan of the row counts, 16 consecutive rows per lane
    int kept = 0;
    for (int r0 = 0; r0 < nrows; r0 += 4096) {             // block-uniform (one round: h <= 4095)
        const int rb = r0 + tid * 16;
        unsigned c[16]; int sum = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { c[k] = (rb + k < nrows) ? s_rs[rb + k] : 0u; sum += (int)c[k]; }
        int total;
        int ex = block_excl_scan(sum, s_wave, total) + kept;
        int first_out = 0x7FFFFFFF;                        // first row start at or beyond the capacity
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (rb + k < nrows) { s_rs[rb + k] = (unsigned)ex; if (ex >= ccap) first_out = min(first_out, ex); }
            ex += (int)c[k];
        }
        if (first_out != 0x7FFFFFFF) atomicMin(&s_live, first_out);
        kept += total;
    }
    if (tid == 0) s_rs[nrows] = (unsigned)kept;
    __syncthreads();
    for (int base = 0; base < nraw; base += 1024) {
        unsigned e4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int sidx = base + tid + 256 * u; e4[u] = sidx < nraw ? fetch(sidx) : 0u; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned e = e4[u];
            if (e >> 24) {
                const unsigned y = (e >> 12) & 0xFFFu, rs = s_rs[y];
                if (rs < (unsigned)ccap) {
                    const unsigned slot = rs + atomicAdd(&s_fill[y], 1u);
                    if (slot < (unsigned)key_cap) s_key[slot] = e;
                }
            }
        }
    }
    __syncthreads();
    unsigned *out = corner + (long long)img * lay.corner_total + L.corner_off;
    // staged slots: every row that starts below ccap is staged whole, so the live slots are [0, first row start >= ccap)
    // (or all `kept` of them); a row holds <= w/2 keypoints, hence nlive <= ccap + w/2 <= key_cap
    const int nlive = min(min(s_live, kept), key_cap);
    for (int slot = tid; slot < nlive; slot += 256) {
        const unsigned key = s_key[slot];
        const unsigned y = (key >> 12) & 0xFFFu, x = key & 0xFFFu;
        const unsigned rs = s_rs[y], re = s_rs[y + 1];
        unsigned rank = 0;
        for (unsigned j = rs; j < re; ++j) rank += ((s_key[j] & 0xFFFu) < x) ? 1u : 0u;
        const unsigned pos = rs + rank;
        if (pos < (unsigned)ccap) out[pos] = key;
    }
    if (tid == 0) {
        corner_count[img * RPE_NLEVELS + l] = min(kept, ccap);
        if (kept > ccap) atomicOr(&ovf[img], (unsigned)RPE_OVF_ORB_CANDIDATES);
    }
}

// retainBest(2 * quota) on the FAST score.  One workgroup of RPE_RETAIN_FAST_WAVES waves per (level, image); the list sits in
// LDS and the workgroup replays the runtime library's nth_element + partition on it (retain_best_emul.h): libstdc++'s
// partition passes have a closed form that the lanes evaluate with ballots and popcounts, every wave on its own slice of
// the range (one lane alone spent 2.5 ms per 2048 images chasing dependent LDS round trips, one wave per list filled 10
// of a CU's 32 wave slots); the few-element steps and MSVC's fat-pivot partition run on one lane.  Two launches share the
// work by list length (lo < n0 <= cap) so that the common short lists do not reserve the LDS of the longest possible one.
#define RPE_RETAIN_FAST_WAVES 2     // measured 1 / 2 / 4: the long lists of retain_fast gain from a second wave,
#define RPE_RETAIN_HARRIS_WAVES 1   // the <= 2 quota + ties candidates of retain_harris lose to the barriers of any more

// retainBest(n_points) on one list in LDS, by the whole workgroup (uniform arguments and result): the routine of
// retain_fast_kernel, retain_harris_kernel and the stage entry rpe_orb_debug_retain.  s_pos: [n + 2] u16, s_ctl: 3 ints per wave.
template <int NW, class E, class GT, class GE>
__device__ __forceinline__ int retain_list(E *s_a, int n, int n_points, int stl, GT gt, GE ge, unsigned short *s_pos, int *s_ctl)
{
    if (stl == rb::RT_LIBSTDCXX)                             // the partition passes as ballot / popcount sweeps of all waves
        return rb::block_retain_best_gnu<NW>(s_a, n, n_points, gt, ge, s_pos, s_ctl);
    if (threadIdx.x == 0) s_ctl[0] = rb::retain_best(s_a, n, n_points, stl, gt, ge);   // MSVC's fat-pivot partition: one lane, move for move
    __syncthreads();
    return s_ctl[0];
}

struct FastScoreGT { __device__ __forceinline__ bool operator()(unsigned a, unsigned b) const { return (a >> 24) > (b >> 24); } };
struct FastScoreGE { __device__ __forceinline__ bool operator()(unsigned a, unsigned b) const { return (a >> 24) >= (b >> 24); } };

__global__ __launch_bounds__(64 * RPE_RETAIN_FAST_WAVES) void retain_fast_kernel(const unsigned *__restrict__ corner, const int *__restrict__ corner_count,
                                                          unsigned *__restrict__ cand_xy, int *__restrict__ cand_count,
                                                          unsigned *__restrict__ ovf, RpeDeviceLayout lay, int lo, int cap, int n_img, int l0)
{
    extern __shared__ unsigned s_a[];                          // [cap] elements, then [cap + 2] u16 stopper positions (block_pair_swap)
    __shared__ int s_ctl[3 * RPE_RETAIN_FAST_WAVES];
    const int tid = threadIdx.x, l = l0 + blockIdx.x;
    const RpeLevel &L = lay.lv[l];
    // the long-list launch runs a small grid whose workgroups walk over the images: on ordinary images it has nothing to do,
    // and 10 000 empty workgroups that each reserve 26 KB of LDS took 64 us
#pragma unroll 1
    for (int img = blockIdx.y; img < n_img; img += gridDim.y) {
    __syncthreads();
    const int n0 = corner_count[img * RPE_NLEVELS + l];
    const int n_points = 2 * L.quota;
    const bool active = n0 > n_points;                       // retainBest does nothing otherwise (the list stays in raster order)
    // the pass-through lists belong to the first launch (lo == 0)
    if (active ? !(n0 > lo && n0 <= cap) : lo != 0) continue;
    const unsigned *in = corner + (long long)img * lay.corner_total + L.corner_off;
    unsigned *out = cand_xy + (long long)img * lay.cand_total + L.cand_off;
    int n1 = n0;
    if (active) {
        for (int i = tid; i < n0; i += 64 * RPE_RETAIN_FAST_WAVES) s_a[i] = in[i];
        __syncthreads();
        n1 = retain_list<RPE_RETAIN_FAST_WAVES>(s_a, n0, n_points, lay.stl, FastScoreGT(), FastScoreGE(), (unsigned short *)(s_a + cap), s_ctl);
    }
    const int nw = min(n1, L.kcap2);
    for (int i = tid; i < nw; i += 64 * RPE_RETAIN_FAST_WAVES) {
        const unsigned e = active ? s_a[i] : in[i];
        out[i] = (((e >> 12) & 0xFFFu) << 16) | (e & 0xFFFu);
    }
    if (tid == 0) {
        cand_count[img * RPE_NLEVELS + l] = nw;
        if (n1 > L.kcap2) atomicOr(&ovf[img], (unsigned)RPE_OVF_ORB_CANDIDATES);
    }
    }
}

#define RPE_RETAIN_TIER 2048         // list length served by the small-LDS launch of the two retain kernels
// The longest lists of the two retain kernels fit the default dynamic LDS: a corner list (ccap), and the candidates of level
// 0, kcap2 = 4 quota + 256 with quota = nfeatures (1 - f) / (1 - f^12) < nfeatures / 7 for orb.cpp's f = 1 / 1.1
constexpr int RETAIN_HARRIS_CAP_MAX = 4 * (RPE_ORB_MAX_FEATURES / 7 + 1) + 256;
static_assert(rpe_retain_lds(0, rpe_corner_cap(RPE_MAX_IMAGE_DIM, RPE_MAX_IMAGE_DIM)) <= RPE_LDS_DEFAULT_BYTES &&
              rpe_retain_lds(1, RETAIN_HARRIS_CAP_MAX) <= RPE_LDS_DEFAULT_BYTES, "the retain kernels need no raised limit");

// raster_corners_kernel's dynamic LDS over a handle's levels: row starts + fill counters + staged entries (raster_key_cap:
// the largest ccap + one full row of keypoints) + tile prefix.  Every term grows with the level's size and level 0 is the
// image itself, so the most is the largest image rpe_create accepts (images beyond ~3000 px pass the default)
constexpr int raster_key_cap(int ccap_max, int wmax) { return ccap_max + wmax / 2 + 64; }
constexpr size_t raster_lds_bytes(int rows_cap, int key_cap, int nt_max) { return sizeof(unsigned) * ((size_t)rows_cap + 1 + rows_cap + key_cap + nt_max + 1); }
constexpr size_t RASTER_LDS_MAX = raster_lds_bytes(RPE_MAX_IMAGE_DIM, raster_key_cap(rpe_corner_cap(RPE_MAX_IMAGE_DIM, RPE_MAX_IMAGE_DIM), RPE_MAX_IMAGE_DIM),
                                                   rpe_fast_tiles(RPE_MAX_IMAGE_DIM, RPE_MAX_IMAGE_DIM));
static_assert(RASTER_LDS_MAX <= RPE_CU_LDS_BYTES, "the largest image's rows, entries and tiles fit a CU's LDS");

// The three launchers of the selection chain take the levels [l0, l1) they run (a level group, orb_groups.h, or all
// twelve) and the stream they run on.  LDS sizes and list tiers stay those of the handle's largest level whatever the
// range, so a level's workgroup is launched the same way in every range; an empty grid is not launched.
void rpe_launch_raster_retain(rpe_handle *h, int n_img, int l0, int l1, hipStream_t stream)
{
    if (l1 <= l0) return;
    int rows_cap = 0, ccap_max = 0, nt_max = 0, wmax = 0, nlev_big = 0;
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        rows_cap = std::max(rows_cap, h->lay.lv[l].h); ccap_max = std::max(ccap_max, h->lay.lv[l].ccap);
        nt_max = std::max(nt_max, h->lay.lv[l].ntile); wmax = std::max(wmax, h->lay.lv[l].w);
        if (h->lay.lv[l].ccap > RPE_RETAIN_TIER) nlev_big = l + 1;       // capacities shrink with the level
    }
    const int key_cap = raster_key_cap(ccap_max, wmax);
    const size_t lds = raster_lds_bytes(rows_cap, key_cap, nt_max);
    assert(lds <= RASTER_LDS_MAX);
    hipLaunchKernelGGL(raster_corners_kernel, dim3(l1 - l0, n_img), dim3(256), lds, stream,
                       (const unsigned *)h->d_tile_list, (const int *)h->d_tile_cnt,
                       h->d_corner, h->d_corner_count, h->d_ovf, h->lay, h->n_tiles_fast, rows_cap, key_cap, l0);
    hipLaunchKernelGGL(retain_fast_kernel, dim3(l1 - l0, n_img), dim3(64 * RPE_RETAIN_FAST_WAVES), rpe_retain_lds(0, std::min(ccap_max, RPE_RETAIN_TIER)), stream,
                       (const unsigned *)h->d_corner, (const int *)h->d_corner_count, h->d_cand_xy, h->d_cand_count, h->d_ovf, h->lay,
                       0, std::min(ccap_max, RPE_RETAIN_TIER), n_img, l0);
    if (std::min(nlev_big, l1) > l0)       // the levels with long lists are [0, nlev_big): those of them in the range
        hipLaunchKernelGGL(retain_fast_kernel, dim3(std::min(nlev_big, l1) - l0, std::min(n_img, 512)), dim3(64 * RPE_RETAIN_FAST_WAVES), rpe_retain_lds(0, ccap_max), stream,
                           (const unsigned *)h->d_corner, (const int *)h->d_corner_count, h->d_cand_xy, h->d_cand_count, h->d_ovf, h->lay,
                           RPE_RETAIN_TIER, ccap_max, n_img, l0);
}

// ----------------------------------------------------------------- harris
// orb.cpp HarrisResponses: 7x7 block of 3x3 Sobel-like derivatives, f32 response.
__global__ __launch_bounds__(256) void harris_kernel(const uint8_t *__restrict__ pyr, const unsigned *__restrict__ cand_xy,
                                                      const int *__restrict__ cand_count, float *__restrict__ cand_resp,
                                                      RpeDeviceLayout lay, int nb, int n_img, int l0, int l1)
{
    // dense lane -> candidate mapping over the per-level counts: the slot arrays are sized 4*quota + 256 per level but
    // hold ~2*quota entries, so slot-indexed lanes were two thirds idle.  The walk covers the launch's levels [l0, l1)
    // and reads no other level's count: retain_fast of another level group may be writing it on another stream
    int img, blk;
    if (!xcd_image_block(nb, n_img, img, blk)) return;
    const int dsel = blk * 256 + threadIdx.x;
    int l = -1, ci = 0, acc = 0;
#pragma unroll
    for (int k = 0; k < RPE_NLEVELS; ++k) {
        if (k < l0 || k >= l1) continue;                     // uniform
        const int n = cand_count[img * RPE_NLEVELS + k];
        if (l < 0 && dsel < acc + n) { l = k; ci = dsel - acc; }
        acc += n;
    }
    if (l < 0) return;
    const RpeLevel &L = lay.lv[l];
    const int c = L.cand_off + ci;
    unsigned xy = cand_xy[(long long)img * lay.cand_total + c];
    const int x0 = xy & 0xFFFF, y0 = xy >> 16, pitch = L.pitch;
    // 9x9 patch (7x7 block of 3x3 derivatives) as 9 rows of THREE ALIGNED DWORDS each (the 9 bytes x0-4 .. x0+4 start at
    // byte (x0 & 3) of the dword run beginning at (x0 - 4) & ~3): 27 dword loads per candidate, all in flight at once,
    // instead of 81 dependent byte loads -- the kernel was bound by the number of memory instructions, not by bytes
    // (0.05 G vector instructions in 0.5 ms).  Reads stay inside the row: x0 >= 31 and x0 + 7 < w - 24 <= pitch.
    const int sh = x0 & 3;
    const uint8_t *p0 = rpe_level_base(pyr, lay, img, l) + (long long)(y0 - 4) * pitch + ((x0 - 4) & ~3);
    unsigned w[9][3];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const unsigned *pr = (const unsigned *)(p0 + r * pitch);
        w[r][0] = pr[0]; w[r][1] = pr[1]; w[r][2] = pr[2];
    }
    int a = 0, b = 0, cc = 0;
    int rowm[9], row0[9], rowp[9];
    auto unpack = [&](int r, int (&out)[9]) {
        const unsigned q0 = __builtin_amdgcn_alignbyte(w[r][1], w[r][0], sh), q1 = __builtin_amdgcn_alignbyte(w[r][2], w[r][1], sh);
        const unsigned q2 = w[r][2] >> (8 * sh);
#pragma unroll
        for (int k = 0; k < 4; ++k) { out[k] = (int)((q0 >> (8 * k)) & 255u); out[4 + k] = (int)((q1 >> (8 * k)) & 255u); }
        out[8] = (int)(q2 & 255u);
    };
    unpack(0, rowm); unpack(1, row0);
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        unpack(r + 2, rowp);
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            int Ix = (row0[k + 1] - row0[k - 1]) * 2 + (rowm[k + 1] - rowm[k - 1]) + (rowp[k + 1] - rowp[k - 1]);
            int Iy = (rowp[k] - rowm[k]) * 2 + (rowp[k - 1] - rowm[k - 1]) + (rowp[k + 1] - rowm[k + 1]);
            a += Ix * Ix; b += Iy * Iy; cc += Ix * Iy;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) { rowm[k] = row0[k]; row0[k] = rowp[k]; }
    }
    const float scale = 1.f / ((1 << 2) * 7 * 255.f);
    const float scale_sq_sq = scale * scale * scale * scale;
    float fa = (float)a, fb = (float)b, fc = (float)cc;
    float t1 = fa * fb, t2 = fc * fc, t3 = t1 - t2;
    float s = fa + fb;
    float t4 = (0.04f * s) * s;
    cand_resp[(long long)img * lay.cand_total + c] = (t3 - t4) * scale_sq_sq;
}

void rpe_launch_harris(rpe_handle *h, int n_img, int l0, int l1, hipStream_t stream)
{
    if (l1 <= l0) return;
    // workgroups per image: the candidate capacity of the range's levels (cand_total when it is all of them)
    const int nb = (h->lay.lv[l1 - 1].cand_off + h->lay.lv[l1 - 1].kcap2 - h->lay.lv[l0].cand_off + 255) / 256;
    hipLaunchKernelGGL(harris_kernel, dim3(xcd_image_grid(nb, n_img)), dim3(256), 0, stream,
                       h->d_pyr, h->d_cand_xy, h->d_cand_count, h->d_cand_resp, h->lay, nb, n_img, l0, l1);
}

// -------------------------------------------------------------- keypoints
// KeyPointsFilter::retainBest(quota) on the Harris response, per level, replayed on the candidates in the order the
// first retainBest left them (see "select" above): element = (f32 response bits << 32 | y << 16 | x), in LDS;
// the survivors go back to the head of the level's candidate run, in order.  compact_keypoints then concatenates the
// levels into the level-major keypoint arrays the descriptor kernel and the matcher read.
struct HarrisGT { __device__ __forceinline__ bool operator()(unsigned long long a, unsigned long long b) const { return __uint_as_float((unsigned)(a >> 32)) > __uint_as_float((unsigned)(b >> 32)); } };
struct HarrisGE { __device__ __forceinline__ bool operator()(unsigned long long a, unsigned long long b) const { return __uint_as_float((unsigned)(a >> 32)) >= __uint_as_float((unsigned)(b >> 32)); } };

__global__ __launch_bounds__(64 * RPE_RETAIN_HARRIS_WAVES) void retain_harris_kernel(unsigned *__restrict__ cand_xy, float *__restrict__ cand_resp,
                                                            const int *__restrict__ cand_count, int *__restrict__ kp_lvl_count,
                                                            RpeDeviceLayout lay, int lo, int cap, int l0)
{
    extern __shared__ unsigned long long s_e[];               // [cap] elements, then [cap + 2] u16 stopper positions
    __shared__ int s_ctl[3 * RPE_RETAIN_HARRIS_WAVES];
    const int tid = threadIdx.x, l = l0 + blockIdx.x, img = blockIdx.y;
    const RpeLevel &L = lay.lv[l];
    const int n1 = cand_count[img * RPE_NLEVELS + l];
    const int q = L.quota;
    const bool active = n1 > q;
    if (active ? !(n1 > lo && n1 <= cap) : lo != 0) return;
    if (!active) { if (tid == 0) kp_lvl_count[img * RPE_NLEVELS + l] = n1; return; }
    unsigned *xy = cand_xy + (long long)img * lay.cand_total + L.cand_off;
    float *resp = cand_resp + (long long)img * lay.cand_total + L.cand_off;
    for (int i = tid; i < n1; i += 64 * RPE_RETAIN_HARRIS_WAVES) s_e[i] = ((unsigned long long)__float_as_uint(resp[i]) << 32) | xy[i];
    __syncthreads();
    const int n2 = retain_list<RPE_RETAIN_HARRIS_WAVES>(s_e, n1, q, lay.stl, HarrisGT(), HarrisGE(), (unsigned short *)(s_e + cap), s_ctl);
    for (int i = tid; i < n2; i += 64 * RPE_RETAIN_HARRIS_WAVES) { const unsigned long long e = s_e[i]; xy[i] = (unsigned)e; resp[i] = __uint_as_float((unsigned)(e >> 32)); }
    if (tid == 0) kp_lvl_count[img * RPE_NLEVELS + l] = n2;
}

// stage entry rpe_orb_debug_retain: retainBest(n_points[i]) on list i of a batch (elements at elems + i * cap, len[i] of
// them), one workgroup per list, through retain_list with the waves of the kind's kernel; every list goes back as it was left, with its new size.
template <int NW, class E, class GT, class GE>
__global__ __launch_bounds__(64 * NW) void retain_debug_kernel(E *__restrict__ elems, const int *__restrict__ len,
                                                                          const int *__restrict__ n_points, int *__restrict__ out_len, int cap, int stl)
{
    extern __shared__ unsigned long long s_dbg[];             // [cap] elements, then [cap + 2] u16 stopper positions
    __shared__ int s_ctl[3 * NW];
    E *s_l = (E *)s_dbg;
    E *list = elems + (long long)blockIdx.x * cap;
    const int tid = threadIdx.x, n = len[blockIdx.x];
    for (int i = tid; i < n; i += 64 * NW) s_l[i] = list[i];
    __syncthreads();
    const int n1 = retain_list<NW>(s_l, n, n_points[blockIdx.x], stl, GT(), GE(), (unsigned short *)(s_l + cap), s_ctl);
    for (int i = tid; i < n; i += 64 * NW) list[i] = s_l[i];
    if (tid == 0) out_len[blockIdx.x] = n1;
}

void rpe_launch_debug_retain(rpe_handle *h, int kind, int stl, void *d_elems, const int *d_len, const int *d_n_points, int *d_out_len, int n_lists, int cap)
{
    const size_t lds = rpe_retain_lds(kind, cap);
    if (kind == 0)
        hipLaunchKernelGGL((retain_debug_kernel<RPE_RETAIN_FAST_WAVES, unsigned, FastScoreGT, FastScoreGE>), dim3(n_lists), dim3(64 * RPE_RETAIN_FAST_WAVES), lds, h->stream,
                           (unsigned *)d_elems, d_len, d_n_points, d_out_len, cap, stl);
    else
        hipLaunchKernelGGL((retain_debug_kernel<RPE_RETAIN_HARRIS_WAVES, unsigned long long, HarrisGT, HarrisGE>), dim3(n_lists), dim3(64 * RPE_RETAIN_HARRIS_WAVES), lds, h->stream,
                           (unsigned long long *)d_elems, d_len, d_n_points, d_out_len, cap, stl);
}

__global__ __launch_bounds__(256) void compact_keypoints_kernel(const unsigned *__restrict__ cand_xy, const float *__restrict__ cand_resp,
                                                                 const int *__restrict__ kp_lvl_count,
                                                                 unsigned *__restrict__ kp_xy, float *__restrict__ kp_resp,
                                                                 float2 *__restrict__ kp_pt, int *__restrict__ kp_count,
                                                                 unsigned *__restrict__ ovf, RpeDeviceLayout lay)
{
    const int img = blockIdx.x, kcap = lay.kcap;
    int offset = 0;
#pragma unroll 1
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        const RpeLevel &L = lay.lv[l];
        const int n = kp_lvl_count[img * RPE_NLEVELS + l];
        const unsigned *xy = cand_xy + (long long)img * lay.cand_total + L.cand_off;
        const float *resp = cand_resp + (long long)img * lay.cand_total + L.cand_off;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int o = offset + i;
            if (o < kcap) {
                const unsigned p = xy[i];
                const int x = p & 0xFFFF, y = p >> 16;
                const long long g = (long long)img * kcap + o;
                kp_xy[g] = (unsigned)x | ((unsigned)y << 12) | ((unsigned)l << 24);
                kp_resp[g] = resp[i];
                kp_pt[g] = make_float2((float)x * L.scale, (float)y * L.scale);
            }
        }
        offset += n;
    }
    if (threadIdx.x == 0) {
        kp_count[img] = min(offset, kcap);
        if (offset > kcap) atomicOr(&ovf[img], (unsigned)RPE_OVF_ORB_KEYPOINTS);
    }
}

void rpe_launch_retain_harris(rpe_handle *h, int n_img, int l0, int l1, hipStream_t stream)
{
    if (l1 <= l0) return;
    int kcap2_max = 0, nlev_big = 0;
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        kcap2_max = std::max(kcap2_max, h->lay.lv[l].kcap2);
        if (h->lay.lv[l].kcap2 > RPE_RETAIN_TIER / 2) nlev_big = l + 1;
    }
    const int tier = std::min(kcap2_max, RPE_RETAIN_TIER / 2);
    assert(kcap2_max <= RETAIN_HARRIS_CAP_MAX);
    hipLaunchKernelGGL(retain_harris_kernel, dim3(l1 - l0, n_img), dim3(64 * RPE_RETAIN_HARRIS_WAVES), rpe_retain_lds(1, tier), stream,
                       h->d_cand_xy, h->d_cand_resp, (const int *)h->d_cand_count, h->d_kp_lvl_count, h->lay, 0, tier, l0);
    if (std::min(nlev_big, l1) > l0)
        hipLaunchKernelGGL(retain_harris_kernel, dim3(std::min(nlev_big, l1) - l0, n_img), dim3(64 * RPE_RETAIN_HARRIS_WAVES), rpe_retain_lds(1, kcap2_max), stream,
                           h->d_cand_xy, h->d_cand_resp, (const int *)h->d_cand_count, h->d_kp_lvl_count, h->lay, RPE_RETAIN_TIER / 2, kcap2_max, l0);
}

// every level's retain_harris has run: the level-major concatenation, on the handle's stream
void rpe_launch_keypoints(rpe_handle *h, int n_img)
{
    hipLaunchKernelGGL(compact_keypoints_kernel, dim3(n_img), dim3(256), 0, h->stream,
                       (const unsigned *)h->d_cand_xy, (const float *)h->d_cand_resp, (const int *)h->d_kp_lvl_count,
                       h->d_kp_xy, h->d_kp_resp, h->d_kp_pt, h->d_kp_count, h->d_ovf, h->lay);
}

// The kernel of this file that launches above the default dynamic LDS.  The retain kernels stay below it (the
// static_assert at RPE_RETAIN_TIER: 48 KB and 47 KB), and rpe_orb_debug_retain refuses a list above it.
std::vector<RpeLdsCeiling> rpe_orb_lds_ceilings()
{
    return {{(const void *)raster_corners_kernel, "raster_corners_kernel", RASTER_LDS_MAX}};
}

// ------------------------------------------------- orientation + descriptor
// Fused per-keypoint kernel (replaces the separate ICAngles, whole-pyramid GaussianBlur
// and rBRIEF launches of the first version): one keypoint per workgroup of one wave, kcap
// workgroups per image.  The 45 x 48-byte raw patch around the keypoint is staged in LDS once and
// feeds (1) the intensity-centroid moments over the radius-15 disc -> fastAtan2 angle,
// (2) the horizontal pass of the f32 7x7 Gaussian on the rows the descriptor can
// touch, (3) the vertical pass evaluated only at the 512 steered sampling points.
// Results are identical to blurring the whole level (the patch never reaches
// the image border: keypoints are >= 31 px inside, the footprint is 22 px).  10016 B of LDS per workgroup.
// Why one keypoint per workgroup.  The phases of a keypoint (patch fetch 0.88 ms, moments + blur 0.36 ms, steered
// sampling 0.65 ms when run alone -- diagnostic builds) overlap only through OTHER waves, and the barriers that tied the
// keypoints of a larger workgroup together cost more than sharing the angle / sincos evaluation between them saved:
// 4 per workgroup 2.25 ms, 2: 2.25, 1: 2.17.  The wave evaluates its own angle on uniform values, no exchange.
#define KP_R 22
#define KP_ROWS 45
#define KP_RAW_DW 12                 // 48 bytes per raw row
#define KP_HCOLS 40                  // horizontally blurred columns: x = x0 - 19 + j (the descriptor reaches |dx| <= 18: columns 1..37)
#define KP_HSTRIDE 49                // f32 per column of the blurred buffer (45 rows + padding; odd, so neighbouring columns start in different banks)
static_assert((KP_ROWS * KP_RAW_DW + 4 + KP_HCOLS * KP_HSTRIDE) * 4 == 10016, "LDS per keypoint");
__global__ __launch_bounds__(64) void orient_describe_kernel(const uint8_t *__restrict__ pyr, const unsigned *__restrict__ kp_xy,
                                                               const float2 *__restrict__ kp_pt, const int *__restrict__ kp_count,
                                                               float *__restrict__ kp_angle, uint8_t *__restrict__ desc,
                                                               RpeDeviceLayout lay, int nb, int n_img)
{
    __shared__ __attribute__((aligned(16))) unsigned raw[KP_ROWS * KP_RAW_DW + 4];   // 16-B aligned rows of 48 B (+ one row pass over-read)
    // horizontally blurred patch, COLUMN-major f32 [column][row]: the 7 vertical taps of a steered sample are contiguous
    __shared__ float hb[KP_HCOLS * KP_HSTRIDE];
    // The workgroup is one wave and the keypoint depends on the workgroup index alone, so everything about the keypoint is
    // wave-uniform.  The record is read through readfirstlane so that the compiler keeps it, the level's layout fields and
    // the patch's base address in scalar registers: the patch loads take a scalar base and one 32-bit offset per lane.
    // (The kernel used to index keypoint and LDS arrays by threadIdx.x >> 6, which hid the uniformity: the level's
    // fields came through vector loads and every address was 64-bit vector arithmetic.)  Measured on its own, together with
    // the row-paired blur pass below: 14 % fewer vector instructions executed and the same kernel time (2.91 -> 2.89 ms) --
    // with 4 waves per SIMD the kernel waits on its memory round trips, which is why the loads below leave early
    // (round 6 in DESIGN section 4).
    const int lane = threadIdx.x;
    int img, blk;
    if (!xcd_image_block(nb, n_img, img, blk)) return;
    // the count and the record leave together (the record of a slot past the count is inside the array and is not used)
    const long long g = (long long)img * lay.kcap + blk;
    const int nkp = kp_count[img];
    const unsigned p = (unsigned)__builtin_amdgcn_readfirstlane((int)kp_xy[g]);
    if (blk >= nkp) return;                                           // the grid is sized for the keypoint capacity
    const int x0 = p & 0xFFF, y0 = (p >> 12) & 0xFFF, l = p >> 24;
    const RpeLevel &L = lay.lv[l];
    const int pitch = L.pitch;
    const int xal = (x0 - KP_R) & ~3, off0 = (x0 - KP_R) - xal;     // off0 in 0..3
    // The kernel runs 4 waves per SIMD (LDS) and its phases are dependent chains, so it pays for every memory round trip it
    // does not overlap: the loads of the two constant tables go out right behind the patch loads instead of where their
    // values are used (24 VGPRs held meanwhile; the kernel has 128 to spend).
    uint2 wt[4];
    float4 pf[4];
    {
        const uint8_t *src = rpe_level_base(pyr, lay, img, l) + (long long)(y0 - KP_R) * pitch + xal;
        // lane -> fixed dword column (lane % 12) and rows lane / 12 + 5 q (60 lanes x 9 loads = 45 x 12 dwords), all loads in
        // flight before the first LDS store.  Byte offsets inside the patch (< 45 pitch) are 32-bit.
        const int lc = lane % KP_RAW_DW, lr = lane / KP_RAW_DW;
        unsigned stage[9];
        if (lane < 60) {
            const unsigned vo = 4u * (unsigned)lc + (unsigned)lr * (unsigned)pitch, p5 = 5u * (unsigned)pitch;
#pragma unroll
            for (int q = 0; q < 9; ++q) stage[q] = *(const unsigned *)(src + (vo + (unsigned)q * p5));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) wt[q] = c_discw[lane + 64 * q];
#pragma unroll
        for (int bit = 0; bit < 4; ++bit) pf[bit] = c_pattern_f[lane * 4 + bit];
        if (lane < 60) {
#pragma unroll
            for (int q = 0; q < 9; ++q) raw[(lr + 5 * q) * KP_RAW_DW + lc] = stage[q];
        }
    }
    __syncthreads();
    int m10 = 0, m01 = 0;
    {
        // ---- orb.cpp ICAngles: integer moments over the disc, reduced with wave shuffles
        // integer sums, so any summation order gives the oracle's moments: 4 disc pixels per packed-u8 dot product.
        // Item = (v + 15) * 8 + j = lane + 64 q: a lane keeps its dword j = lane % 8 and takes rows v0 + 8 q, v0 = lane / 8 - 15,
        // so the four items share one address and differ by constant offsets (the table's 32nd row is zero: row v = 16
        // of the patch is read and weighs nothing).  The dot products chain their sums: c[q] = s1_0 + .. + s1_q, and
        // sum_q (v0 + 8 q) s1_q = (v0 + 24) c[3] - 8 (c[0] + c[1] + c[2]).
        {
            const int bo = off0 + KP_R - 16;                                        // byte column of u = -16 (>= 6)
            const int sh = bo & 3;
            const unsigned *pw = raw + ((KP_R - 15) + (lane >> 3)) * KP_RAW_DW + ((bo >> 2) + (lane & 7));
            unsigned c[4], su = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned px = __builtin_amdgcn_alignbyte(pw[8 * q * KP_RAW_DW + 1], pw[8 * q * KP_RAW_DW], sh);
                c[q] = __builtin_amdgcn_udot4(px, wt[q].x, q ? c[q - 1] : 0u, false);
                su = __builtin_amdgcn_udot4(px, wt[q].y, su, false);
            }
            m10 = (int)su - 16 * (int)c[3];
            m01 = __mul24((lane >> 3) + 9, (int)c[3]) - 8 * (int)(c[0] + c[1] + c[2]);
        }
        // wave sums by DPP row shifts / broadcasts (total in lane 63, read back as a scalar): 12 + 2 instructions; six
        // rounds of __shfl_xor were 36 vector + 12 LDS (ds_bpermute) instructions
        m10 = wave_sum(m10);
        m01 = wave_sum(m01);
        // ---- horizontal pass of the descriptor blur.  cv2 blurs every pyramid level with GaussianBlur(7x7, sigma 2) before
        // computeOrbDescriptors; on a pyramid SUB-matrix that call takes sepFilter2D's f32 route (filter.simd.hpp
        // RowFilter<uchar, float>, SymmColumnFilter<Cast<float, uchar>>), whose AVX2-dispatched build fuses s += f * x: the
        // reference's own result rows single this out against every fixed-point variant (tests/test_reference_rows_cpu.py).
        // Row pass: s = g0 p[x-3]; s = fma(g_k, p[x-3+k], s), k = 1..6, in that order.  hbuf column j <-> x = x0 - 19 + j.
        // Item = (two patch rows r, r + 1, group of 8 columns), 2 x 20 raw bytes shared by the item's 2 x 8 outputs.  Round 0:
        // rows (0,1) .. (22,23), 12 pairs x 5 groups on 60 lanes; round 1: rows (23,24) .. (43,44), 11 pairs on 55 lanes, so
        // a lane's second item sits a constant 23 rows below its first and nothing is clamped (row 23 is computed twice, to
        // the same value).
        {
            const float g0 = c_gauss[0], g1 = c_gauss[1], g2 = c_gauss[2], g3 = c_gauss[3];
            const int rp = lane / 5, cg = lane - 5 * rp;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (lane < (q == 0 ? 60 : 55)) {
                    const int row = 2 * rp + (KP_ROWS / 2 + 1) * q;
                    const unsigned *pw = raw + row * KP_RAW_DW + 2 * cg;
                    unsigned qq[2][4];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const unsigned *ph = pw + h * KP_RAW_DW;
                        const unsigned d0 = ph[0], d1 = ph[1], d2 = ph[2], d3 = ph[3], d4 = ph[4];
                        qq[h][0] = __builtin_amdgcn_alignbyte(d1, d0, off0); qq[h][1] = __builtin_amdgcn_alignbyte(d2, d1, off0);
                        qq[h][2] = __builtin_amdgcn_alignbyte(d3, d2, off0); qq[h][3] = __builtin_amdgcn_alignbyte(d4, d3, off0);
                    }
                    // two outputs per v_pk_mul_f32 / v_pk_fma_f32 (each half an IEEE fma of its own: same bits as the scalar
                    // form).  A packed operand is an aligned register pair; pairing the two ROWS of a column, F[j] = (byte j
                    // of row r, byte j of row r + 1), lets each v_cvt_f32_ubyteN write its half in place and tap k of
                    // output column o read F[o + k] as it stands.  (Pairing two columns of one row needed every converted
                    // pixel twice, at even and at odd pair alignment, and register moves to build the second set.)
                    typedef float v2f_t __attribute__((ext_vector_type(2)));
                    v2f_t F[14];
#pragma unroll
                    for (int j = 0; j < 14; ++j)
                        F[j] = (v2f_t){(float)((qq[0][j >> 2] >> (8 * (j & 3))) & 255u), (float)((qq[1][j >> 2] >> (8 * (j & 3))) & 255u)};
                    float *dst = hb + (8 * cg) * KP_HSTRIDE + row;
                    const v2f_t G0 = {g0, g0}, G1 = {g1, g1}, G2 = {g2, g2}, G3 = {g3, g3};
#pragma unroll
                    for (int o = 0; o < 8; ++o) {
                        v2f_t sacc = G0 * F[o];
                        sacc = __builtin_elementwise_fma(G1, F[o + 1], sacc);
                        sacc = __builtin_elementwise_fma(G2, F[o + 2], sacc);
                        sacc = __builtin_elementwise_fma(G3, F[o + 3], sacc);
                        sacc = __builtin_elementwise_fma(G2, F[o + 4], sacc);      // the kernel is symmetric: g4 = g2, g5 = g1, g6 = g0 (same f32 values)
                        sacc = __builtin_elementwise_fma(G1, F[o + 5], sacc);
                        sacc = __builtin_elementwise_fma(G0, F[o + 6], sacc);
                        dst[o * KP_HSTRIDE] = sacc.x;                               // adjacent dwords: one ds_write2_b32
                        dst[o * KP_HSTRIDE + 1] = sacc.y;
                    }
                }
            }
        }
    }
    __syncthreads();
    // the angle, on wave-uniform values
    float a, b;
    {
        const float angle = fast_atan2_deg((float)m01, (float)m10);
        if (lane == 0) kp_angle[g] = angle;
        const float ang = angle * (float)(3.141592653589793238462643383279502884 / 180.0);
        double sn, cs;
        det_sincos((double)ang, sn, cs);
        a = (float)cs; b = (float)sn;
    }
    // ---- orb.cpp computeOrbDescriptors: lane = 4 consecutive bit tests, vertical pass at the samples
    const float2 pt = kp_pt[g];
    const float sc = L.inv_scale;                                 // 1.f / L.scale, divided once on the host
    const int cx = __float2int_rn(pt.x * sc), cy = __float2int_rn(pt.y * sc);
    const int dxo = cx - x0 + 19, dyo = cy - y0 + KP_R - 3;       // (cx,cy) == (x0,y0) in practice
    // the sample (0, 0), wave-uniform, in a scalar register.  The empty asm hides its value: left to itself the compiler moves the
    // constant part (19 columns + 19 rows = 3800 B) into the offset fields of the LDS reads, where it does not fit (ds_read2_b32
    // reaches 1020 B), and adds it back three times per sample
    int o00 = __builtin_amdgcn_readfirstlane(dxo * KP_HSTRIDE + dyo);
    asm volatile("" : "+s"(o00));
    const float *hb0 = hb + o00;
    const float g3 = c_gauss[3], g4 = c_gauss[4], g5 = c_gauss[5], g6 = c_gauss[6];
    unsigned nib = 0;
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) {
        const float p0 = pf[bit].x, p1 = pf[bit].y, p2 = pf[bit].z, p3 = pf[bit].w;
        float fx0 = p0 * a - p1 * b, fy0 = p0 * b + p1 * a;
        float fx1 = p2 * a - p3 * b, fy1 = p2 * b + p3 * a;
        float t01[2];
        // cvRound of both coordinates, then the sample's offset ix * KP_HSTRIDE + iy in f32: whole numbers below 2^24, so
        // the fused multiply-add is exact and one conversion gives the integer the two conversions and a multiply gave
        const float rxs[2] = {__builtin_rintf(fx0), __builtin_rintf(fx1)}, rys[2] = {__builtin_rintf(fy0), __builtin_rintf(fy1)};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            // vertical pass at the sample only: the 7 taps = rows iy + dyo .. + 6 of column ix + dxo, contiguous f32;
            // s = g3 c; s = fma(g_{3+k}, t[3+k] + t[3-k], s), k = 1..3 (SymmColumnFilter), then cvRound (saturate_cast<uchar>)
            const float *t = hb0 + (int)__builtin_fmaf(rxs[e], (float)KP_HSTRIDE, rys[e]);
            typedef float v2f_t __attribute__((ext_vector_type(2)));
            const v2f_t s45 = (v2f_t){t[4], t[5]} + (v2f_t){t[2], t[1]};     // two of the three tap sums in one v_pk_add_f32
            float sacc = g3 * t[3];
            sacc = __builtin_fmaf(g4, s45.x, sacc);
            sacc = __builtin_fmaf(g5, s45.y, sacc);
            sacc = __builtin_fmaf(g6, t[6] + t[0], sacc);
            t01[e] = __builtin_rintf(sacc);                           // 0 <= value <= 255 (convex combination of bytes): no saturation to apply
        }
        nib |= (unsigned)(t01[0] < t01[1]) << bit;
    }
    // 8 nibbles -> one dword (lanes 8m .. 8m+7), written by lane 8m
    unsigned v = nib << (4 * (lane & 7));
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);       // quad_perm [1,0,3,2]: lane ^ 1
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);       // quad_perm [2,3,0,1]: lane ^ 2
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);      // row_half_mirror: the other quad of the 8
    if ((lane & 7) == 0) *(unsigned *)(desc + g * 32 + (lane >> 3) * 4) = v;
}

void rpe_launch_orient_describe(rpe_handle *h, int n_img)
{
    const int nb = h->lay.kcap;                                       // workgroups per image
    hipLaunchKernelGGL(orient_describe_kernel, dim3(xcd_image_grid(nb, n_img)), dim3(64), 0, h->stream,
                       h->d_pyr, h->d_kp_xy, h->d_kp_pt, h->d_kp_count, h->d_kp_angle, h->d_desc, h->lay, nb, n_img);
}

// ------------------------------------------------------------------- blur
// GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) as ORB runs it (in place on a pyramid sub-matrix => cv2's
// sepFilter2D f32 route, see orient_describe_kernel): row pass s = g0 p[x-3], s = fma(g_k, p[x-3+k], s); column pass
// s = g3 c, s = fma(g_{3+k}, r[y+k] + r[y-k], s); result cvRound(s).  Whole levels, for rpe_orb_debug_fetch only.
__device__ __forceinline__ int refl101(int p, int n) { p = p < 0 ? -p : p; return p >= n ? 2 * n - 2 - p : p; }

__global__ __launch_bounds__(256) void blur_kernel(const uint8_t *__restrict__ pyr, uint8_t *__restrict__ dst,
                                                    RpeDeviceLayout lay, const RpeTile *__restrict__ tiles, int src_img)
{
    // 64x64 tile; input 70 rows x 72 bytes (x0-4 .. x0+67) loaded as aligned dwords; rows
    // are reflected at load time, the <=3 reflected columns per side are patched in LDS.
    constexpr int TH = 64;
    __shared__ unsigned s_in[(TH + 6) * 18];
    __shared__ float4 s_h[(TH + 6) * 16];          // horizontal pass: 4 x f32 per entry
    const int tid = threadIdx.x;
    const RpeTile t = tiles[blockIdx.x];
    const RpeLevel &L = lay.lv[t.level];
    const int w = L.w, hgt = L.h, pitch = L.pitch;
    const int x0 = t.tx, y0 = t.ty;
    const long long ibase = (long long)blockIdx.y * lay.stride + L.off;                 // destination: image slot blockIdx.y
    const uint8_t *src = pyr + (long long)(src_img + blockIdx.y) * lay.stride + L.off;
    for (int i = tid; i < (TH + 6) * 18; i += 256) {
        int r = i / 18, c = i - r * 18;
        int y = refl101(y0 - 3 + r, hgt);
        y = min(max(y, 0), hgt - 1);
        int x = min(max(x0 - 4 + 4 * c, 0), pitch - 4);
        s_in[i] = *(const unsigned *)(src + (long long)y * pitch + x);
    }
    __syncthreads();
    uint8_t *sb = (uint8_t *)s_in;
    if (x0 == 0) {               // columns -1,-2,-3 <- 1,2,3
        for (int i = tid; i < (TH + 6) * 3; i += 256) { int r = i / 3, k = i - r * 3 + 1; sb[r * 72 + 4 - k] = sb[r * 72 + 4 + k]; }
    }
    if (x0 + 64 + 3 >= w && x0 < w) {   // columns w, w+1, w+2 <- w-2, w-3, w-4
        for (int i = tid; i < (TH + 6) * 3; i += 256) {
            int r = i / 3, k = i - r * 3;
            int cd = w + k - x0 + 4, cs = w - 2 - k - x0 + 4;
            if (cd < 72 && cs >= 0) sb[r * 72 + cd] = sb[r * 72 + cs];
        }
    }
    __syncthreads();
    const float g0 = c_gauss[0], g1 = c_gauss[1], g2 = c_gauss[2], g3 = c_gauss[3];
    for (int i = tid; i < (TH + 6) * 16; i += 256) {
        int r = i >> 4, c = i & 15;
        unsigned a = s_in[r * 18 + c], b = s_in[r * 18 + c + 1], d = s_in[r * 18 + c + 2];
        float p[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) { p[k] = (float)((a >> (8 * k)) & 255u); p[4 + k] = (float)((b >> (8 * k)) & 255u); p[8 + k] = (float)((d >> (8 * k)) & 255u); }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float sacc = g0 * p[j + 1];
            sacc = __builtin_fmaf(g1, p[j + 2], sacc); sacc = __builtin_fmaf(g2, p[j + 3], sacc); sacc = __builtin_fmaf(g3, p[j + 4], sacc);
            sacc = __builtin_fmaf(g2, p[j + 5], sacc); sacc = __builtin_fmaf(g1, p[j + 6], sacc); sacc = __builtin_fmaf(g0, p[j + 7], sacc);
            o[j] = sacc;
        }
        s_h[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    const int tx = tid & 15, tyb = tid >> 4;
#pragma unroll
    for (int rr = 0; rr < TH / 16; ++rr) {
        const int ty = tyb + 16 * rr;
        float4 r[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) r[k] = s_h[(ty + k) * 16 + tx];
        auto col = [&](float c, float a1, float b1, float a2, float b2, float a3, float b3) -> unsigned {
            float sacc = g3 * c;
            sacc = __builtin_fmaf(g2, a1 + b1, sacc);
            sacc = __builtin_fmaf(g1, a2 + b2, sacc);
            sacc = __builtin_fmaf(g0, a3 + b3, sacc);
            return (unsigned)min(max(__float2int_rn(sacc), 0), 255);
        };
        unsigned out = col(r[3].x, r[4].x, r[2].x, r[5].x, r[1].x, r[6].x, r[0].x) |
                       (col(r[3].y, r[4].y, r[2].y, r[5].y, r[1].y, r[6].y, r[0].y) << 8) |
                       (col(r[3].z, r[4].z, r[2].z, r[5].z, r[1].z, r[6].z, r[0].z) << 16) |
                       (col(r[3].w, r[4].w, r[2].w, r[5].w, r[1].w, r[6].w, r[0].w) << 24);
        int px = x0 + 4 * tx, py = y0 + ty;
        if (py < hgt && px < pitch) *(unsigned *)(dst + ibase + (long long)py * pitch + px) = out;
    }
}

// whole-level blur of ONE image of the last run into the one-image debug buffer (rpe_orb_debug_fetch which = 3)
void rpe_launch_debug_blur(rpe_handle *h, int img)
{
    hipLaunchKernelGGL(blur_kernel, dim3(h->n_tiles_full, 1), dim3(256), 0, h->stream,
                       h->d_pyr, h->d_bufA, h->lay, h->d_tiles_full, img);
}
