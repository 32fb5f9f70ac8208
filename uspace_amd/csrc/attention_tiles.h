// What the attention kernels share (attention.hip: K and V of a head resident in LDS, L <= 336; attention_long.hip: K and V
// streamed through LDS in key tiles, any L): the LDS image of K / V rows with its bank-spreading swizzles, the LDS-DMA that stages
// eight rows per wave-instruction, the transposing V read and the cross-lane step of the row maximum.  head_dim 64: a row is 128 B;
// attention_wide.hip lays a wider head out as 64-column panels of this image.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;
constexpr int DH = 64;
constexpr int KROW_BYTES = 128;

__device__ __forceinline__ int k_off(int r, int c) { return r * KROW_BYTES + ((c ^ ((r >> 1) & 7)) << 4); }

// V rows are 128 B like K rows, but the transposing read fetches 32-byte pieces of 8 different rows per 32-lane
// half: 32-B chunk c of row r lives at chunk c ^ ((r >> 1) & 3), which puts those 8 pieces on 8 distinct
// 32-byte bank groups (row parity selects the 128-B half of the 256-B bank row, the XOR the piece inside it).
__device__ __forceinline__ int v_off(int r, int c32) { return r * KROW_BYTES + ((c32 ^ ((r >> 1) & 3)) << 5); }

typedef __attribute__((ext_vector_type(4))) short s16x4;
__device__ __forceinline__ uint2 lds_read_tr16(const char* p) {
    const s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
    union { s16x4 v; uint2 u; } c;
    c.v = r;
    return c.u;
}

// One LDS-DMA instruction (global_load_lds, 16 B per lane): rows rb .. rb + 7 of K (`g` = row 0 of the head's K, C3 elements from row
// to row) into the 1 KiB at `dst`.  The LDS image is lane-linear, so the swizzle of k_off is applied on the source address; it is keyed
// on the row's index, which must agree with the row's place in the image modulo 16.  Rows >= L re-read row L - 1: finite values whose
// scores the kernels mask.
__device__ __forceinline__ void att_dma_k8(const bf16_t* g, int C3, int rb, int L, char* dst, int lane) {
    const int r = rb + (lane >> 3), cpos = lane & 7;
    const int c = cpos ^ ((r >> 1) & 7);
    const int rr = r < L ? r : L - 1;
    __builtin_amdgcn_global_load_lds((const US_GLB void*)(g + (size_t)rr * C3 + c * 8), (US_LDS void*)dst, 16, 0, 0);
}
// ... of V (row-major; physical 16-B position cpos holds logical chunk (((cpos>>1) ^ ((r>>1)&3)) << 1) | (cpos&1): v_off); the row's
// index must agree with its place in the image modulo 8
__device__ __forceinline__ void att_dma_v8(const bf16_t* g, int C3, int rb, int L, char* dst, int lane) {
    const int r = rb + (lane >> 3), cpos = lane & 7;
    const int c = (((cpos >> 1) ^ ((r >> 1) & 3)) << 1) | (cpos & 1);
    const int rr = r < L ? r : L - 1;
    __builtin_amdgcn_global_load_lds((const US_GLB void*)(g + (size_t)rr * C3 + c * 8), (US_LDS void*)dst, 16, 0, 0);
}

// The transposing V read of the 32-key P.V step that starts `step_bytes` (a multiple of 16 rows) into the image `sV`: group fq of 16
// lanes points at V[4fq + 0..3][dt*16 .. +15] (lane a: key row a/4, dims 4(a%4)..+3) and receives, per lane, dim dt*16+fr of those 4
// keys; `hi` does the same 16 rows on (same swizzle key, +2048 B).  (step_bytes last: a constant there folds into the read's offset field.)
__device__ __forceinline__ void att_read_vt(const char* sV, int fq, int fr, int dt, int step_bytes, uint2& lo, uint2& hi) {
    const int vrow = fq * 4 + (fr >> 2);
    const char* pv = sV + v_off(vrow, dt) + ((fr & 3) << 3) + step_bytes;
    lo = lds_read_tr16(pv);
    hi = lds_read_tr16(pv + 16 * KROW_BYTES);
}

// max over the four 16-lane rows of a wave (a query's keys are spread over lanes fr, fr + 16, fr + 32, fr + 48): v_permlane16_swap /
// v_permlane32_swap on two copies of the value leave rows (0, 0, 2, 2) | (1, 1, 3, 3) resp. halves (lo, lo) | (hi, hi) -- one VALU
// instruction where __shfl_xor is a trip through the LDS crossbar
__device__ __forceinline__ float att_max_over_rows(float mx) {
    const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    mx = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
    const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    return fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}

}  // namespace
