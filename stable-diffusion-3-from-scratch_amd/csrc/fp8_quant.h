// Device code of the e4m3 quantisers, shared by the plain entry points (rowops.hip: mmdit_fp8_quantize, mmdit_fp8_quantize_delayed,
// mmdit_mxfp8_quantize) and the zero-padding ones (fp8_pad.hip, include/mmdit_hip_fp8pad.h): ONE spelling of the arithmetic, so that the two
// families write the same bytes for the same values.
#pragma once
#include "common.h"

// Quantisation factor 448 / a and dequantisation scale a / 448 of a per-tensor range a = max(amax, 1e-12).
__device__ __forceinline__ float fp8_range(float amax, float& dequant) {
  const float a = fmaxf(amax, 1e-12f);
  dequant = a / 448.f;
  return 448.f / a;
}
// 8 values -> 8 e4m3 codes: saturate(v * s) on the hardware converter.
__device__ __forceinline__ uint2 fp8_pack8(const float (&x)[8], float s) {
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; e++) v[e] = fminf(fmaxf(x[e] * s, -448.f), 448.f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
  return make_uint2((unsigned)lo, (unsigned)hi);
}
__device__ __forceinline__ float fp8_amax8(float m, const float (&x)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e++) m = fmaxf(m, fabsf(x[e]));
  return m;
}
// Maximum of the per-thread maxima of a 256-thread workgroup into *dst: one atomic per workgroup (they all hit the same address);
// non-negative floats order like their bit patterns.  sm: 4 floats of LDS.
__device__ __forceinline__ void fp8_wg_amax(float m, float* __restrict__ dst, float* sm) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax((unsigned int*)dst, __float_as_uint(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]))));
}

// MX quantisation of one 32-block: block t of the (rows, Kq / 32) blocks of the OUTPUT q[rows][Kq], Kq >= K a multiple of 32.  Blocks of
// columns [0, K) read x[row][blk * 32 ...] (leading dimension ldx); blocks of columns [K, Kq) -- the zero padding of fp8_pad.hip, none when
// Kq == K -- are quantised from zeros: codes 0x00 and the scale byte of an all-zero block.  The scale byte goes to its place in the GEMM's
// layout (mx_scale_index), which does not depend on the row width.
template <typename TI>
__device__ __forceinline__ void mx_quant_block(int64_t t, const TI* __restrict__ x, int rows, int K, int Kq, int64_t ldx, uint4* __restrict__ q,
                                               unsigned char* __restrict__ sc) {
  const int bpr = Kq >> 5;                                            // blocks per row
  if (t >= (int64_t)rows * bpr) return;
  const int row = (int)(t / bpr), blk = (int)(t - (int64_t)row * bpr);
  float v[32];
  if (blk * 32 < K) {
    const TI* src = x + (int64_t)row * ldx + blk * 32;
#pragma unroll
    for (int c = 0; c < 4; c++) ld8(src + c * 8, *(float(*)[8])(v + c * 8));
  } else {
#pragma unroll
    for (int e = 0; e < 32; e++) v[e] = 0.f;
  }
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 32; e++) amax = fmaxf(amax, fabsf(v[e]));
  float inv;
  const int ex = mx_exponent(amax, inv);
  unsigned w[8];
#pragma unroll
  for (int c = 0; c < 8; c++) w[c] = mx_pack4(v + 4 * c, inv);
  uint4* dst = q + ((int64_t)row * Kq + blk * 32) / 16;
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  sc[mx_scale_index(row, blk, rows)] = (unsigned char)(ex + 127);
}
