// rpe_calibrate.hip -- roofline calibration of the device: the measured instruction-issue and HBM rates bench.py prices
// the kernels against.  Nothing of the pose path is in here.
#include "rpe_internal.h"

// ------------------------------------------------------------ roofline calibration
// The hot path is bound by vector-instruction ISSUE, not by HBM, so bench.py prices the
// dominant kernel and the matcher against a MEASURED issue rate: each kernel below runs a long stream of one
// instruction kind (inline asm: the count is exact, nothing is folded away) over independent register chains,
// at 1, 2, 4 or 8 resident waves per SIMD on every CU.  MI355X_MICROARCH.md: a wave64 VALU instruction takes
// 2 cycles on the 32-wide SIMD when >= 2 waves feed it, 4 cycles for one wave alone; f64 and transcendental
// instructions take longer.  Kinds: the instructions the ORB / matcher / RANSAC inner loops are made of.
#define CALIB_UNROLL 16
template <int KIND>
__global__ __launch_bounds__(256) void valu_calib_kernel(unsigned *sink, int iters)
{
    unsigned a[8];
    double d[8];
    float f[8];
    typedef float f2_t __attribute__((ext_vector_type(2)));
    f2_t f2[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        a[u] = threadIdx.x * 2654435761u + u * 40503u + blockIdx.x; d[u] = 1.0 + 1e-9 * (double)(a[u] & 1023u);
        f[u] = 1.0f + 1e-6f * (float)(a[u] & 1023u); f2[u].x = f[u]; f2[u].y = f[u] * 0.5f;
    }
    const float fk = 1.0000001f;
    const f2_t fk2 = {1.0000001f, 0.9999999f};
    const unsigned k0 = 0x9E3779B9u ^ threadIdx.x, k1 = 0x01010101u;
    const double dk = 1.0000000001;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < CALIB_UNROLL / 8; ++r) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (KIND == 0)       // the Hamming inner loop: v_xor_b32 + v_bcnt_u32_b32 (2 instructions)
                    asm volatile("v_xor_b32 %0, %0, %1\n\tv_bcnt_u32_b32 %0, %0, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 1)  // packed 16-bit min / max (2 instructions): the FAST pair test before it went to bytes (kind 16)
                    asm volatile("v_pk_min_i16 %0, %0, %1\n\tv_pk_max_i16 %0, %0, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 2)  // byte gather: v_perm_b32 (1 instruction)
                    asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 3)  // packed-u8 dot product: v_dot4_u32_u8 (1 instruction)
                    asm volatile("v_dot4_u32_u8 %0, %1, %2, %0" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 4)  // FAST ring score: v_min3_i32 + v_max3_i32 (2 instructions)
                    asm volatile("v_min3_i32 %0, %0, %1, %2\n\tv_max3_i32 %0, %0, %1, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 5)  // resize / blur taps: v_mad_u32_u24 (1 instruction)
                    asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a[u]) : "v"(k1), "v"(k0));
                else if (KIND == 6)  // RANSAC / pose: v_mul_f64 + v_add_f64 (2 instructions; the library compiles without contraction)
                    asm volatile("v_mul_f64 %0, %0, %1\n\tv_add_f64 %0, %0, %1" : "+v"(d[u]) : "v"(dk));
                else if (KIND == 7)  // v_fma_f64 (1 instruction), for reference
                    asm volatile("v_fma_f64 %0, %0, %1, %1" : "+v"(d[u]) : "v"(dk));
                else if (KIND == 8)  // v_fma_f32 (1 instruction): the guide's 2-cycle instruction
                    asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(f[u]) : "v"(fk));
                else if (KIND == 9)  // v_pk_fma_f32 (1 instruction, 2 FMAs per lane): the 157 TFLOP/s f32 vector peak
                    asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(f2[u]) : "v"(fk2));
                else if (KIND == 10) // pyramid / descriptor taps: v_dot2_u32_u16
                    asm volatile("v_dot2_u32_u16 %0, %1, %2, %0" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 11) // byte phase: v_alignbyte_b32
                    asm volatile("v_alignbyte_b32 %0, %0, %1, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 12) // 32-bit multiply: v_mul_lo_u32
                    asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a[u]) : "v"(k0));
                else if (KIND == 13) // 64-bit multiply-add (what 32-bit index arithmetic often compiles to): v_mad_u64_u32
                    asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(d[u]) : "v"(k0), "v"(k1) : "vcc");
                else if (KIND == 14) // SDWA operand select: v_mul_u32_u24_sdwa
                    asm volatile("v_mul_u32_u24_sdwa %0, %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "+v"(a[u]) : "v"(k0));
                else if (KIND == 15) // packed 16-bit multiply-add: v_pk_mad_u16
                    asm volatile("v_pk_mad_u16 %0, %0, %1, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else if (KIND == 16) // FAST pair test on four pixels per register: v_lerp_u8 (1 instruction, 4 byte compares)
                    asm volatile("v_lerp_u8 %0, %0, %1, %2" : "+v"(a[u]) : "v"(k0), "v"(k1));
                else                 // its pair logic: v_bitop3_b32, (a | b) & c
                    asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0xa8" : "+v"(a[u]) : "v"(k0), "v"(k1));
            }
        }
    }
    unsigned acc = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc ^= a[u] ^ (unsigned)__double_as_longlong(d[u]) ^ __float_as_uint(f[u]) ^ __float_as_uint(f2[u].x) ^ __float_as_uint(f2[u].y);
    if (acc == 0x12345679u) *sink = acc;
}

static const int kCalibInstPerSlot[18] = {2, 2, 1, 1, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
static const char *kCalibNames[18] = {"v_xor_b32+v_bcnt_u32_b32", "v_pk_min_i16+v_pk_max_i16", "v_perm_b32", "v_dot4_u32_u8",
                                      "v_min3_i32+v_max3_i32", "v_mad_u32_u24", "v_mul_f64+v_add_f64", "v_fma_f64", "v_fma_f32", "v_pk_fma_f32",
                                      "v_dot2_u32_u16", "v_alignbyte_b32", "v_mul_lo_u32", "v_mad_u64_u32", "v_mul_u32_u24_sdwa", "v_pk_mad_u16",
                                      "v_lerp_u8", "v_bitop3_b32"};
extern "C" const char *rpe_calibrate_valu_name(int kind) { return (kind >= 0 && kind < 18) ? kCalibNames[kind] : "?"; }

extern "C" int rpe_calibrate_valu(rpe_handle *h, int kind, int waves_per_simd, double *wave_insts_per_s)
{
    if (!h || !wave_insts_per_s || kind < 0 || kind > 17 || waves_per_simd < 1 || waves_per_simd > 8) return rpe_invalid(h, "rpe_calibrate_valu");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, h->cfg.device));
    DM_ONCE(h, h->d_calib_sink, 1);
    const int ncu = prop.multiProcessorCount;
    // one 256-thread block = 4 waves = one wave per SIMD of a CU; waves_per_simd blocks per CU
    const int blocks = ncu * waves_per_simd, iters = 20000;
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {                    // first repetition warms up
        HIPCHK(h, hipEventRecord(e0, h->stream));
        switch (kind) {
#define CALIB_CASE(K) case K: hipLaunchKernelGGL((valu_calib_kernel<K>), dim3(blocks), dim3(256), 0, h->stream, h->d_calib_sink, iters); break;
            CALIB_CASE(0) CALIB_CASE(1) CALIB_CASE(2) CALIB_CASE(3) CALIB_CASE(4) CALIB_CASE(5) CALIB_CASE(6) CALIB_CASE(7)
            CALIB_CASE(8) CALIB_CASE(9) CALIB_CASE(10) CALIB_CASE(11) CALIB_CASE(12) CALIB_CASE(13) CALIB_CASE(14) CALIB_CASE(15) CALIB_CASE(16) CALIB_CASE(17)
#undef CALIB_CASE
        }
        HIPCHK(h, hipEventRecord(e1, h->stream));
        HIPCHK(h, hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    const double insts = (double)blocks * 4.0 * (double)iters * CALIB_UNROLL * kCalibInstPerSlot[kind];
    *wave_insts_per_s = insts / ((double)best * 1e-3);
    return RPE_OK;
}

// HBM streaming rate of this device: 16-B-per-lane read of the handle's pyramid buffer (>= 256 MiB so the
// Infinity Cache cannot serve it) -- the "achievable" figure next to the 8 TB/s spec peak in the bench line.
__global__ __launch_bounds__(256) void calib_read16_kernel(const uint4 *__restrict__ p, size_t n, unsigned *sink)
{
    unsigned acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { uint4 v = p[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x12345679u) *sink = acc;
}
extern "C" int rpe_calibrate_hbm(rpe_handle *h, double *bytes_per_s)
{
    if (!h || !bytes_per_s) return rpe_invalid(h, "rpe_calibrate_hbm");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t NIo = h->cfg.feature_method == RPE_FEATURE_SIFT ? 1 : (size_t)h->n_img_cap;
    const size_t bytes = NIo * (size_t)h->lay.stride;
    if (bytes < ((size_t)256 << 20)) { h->err = "rpe_calibrate_hbm: the handle's pyramid buffer is smaller than the 256 MiB Infinity Cache"; return RPE_ERR_INVALID; }
    DM_ONCE(h, h->d_calib_sink, 1);
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {
        HIPCHK(h, hipEventRecord(e0, h->stream));
        hipLaunchKernelGGL(calib_read16_kernel, dim3(8192), dim3(256), 0, h->stream, (const uint4 *)h->d_pyr, bytes / 16, h->d_calib_sink);
        HIPCHK(h, hipEventRecord(e1, h->stream));
        HIPCHK(h, hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    *bytes_per_s = (double)bytes / ((double)best * 1e-3);
    return RPE_OK;
}
